"""Facet counts: how many of the allowed rows hold each value of a metadata key (`arx_facet_count`, include/arx.h; INTEGRATION.md
"Facet counts").

    cols = MetadataColumns(metadata, lo, hi, device="cuda:0")
    res = count(cols, ["section", {"key": "quality_score", "edges": [0.9, 0.95, 1.0]}], bitmaps, top=10)     # res[filter][key]

The columns are those `where_device` keeps in HBM and the bitmaps those every row filter here produces, so nothing is rebuilt or
uploaded but a key's `cuts`.  A spec is resolved on the host into what the kernel takes:
  strings   mode CODE over the string codes, one bin per entry of `cols.strings(key)`
  bools     mode CODE, two bins (False, True)
  numbers   mode EXACT, `cuts = cols.numbers(key)`, one bin per distinct number
  edges     mode INTERVAL over numbers, `cuts = edges`, bin i = [edges[i], edges[i + 1]) and the last bin closed
Per (filter, key) the kernel leaves n_bins + 2 int32 counters on the device: the bins, `missing` (an allowed row whose value is of
another kind, or absent) and `unbinned` (the right kind and no bin: a NaN, a number outside the edges).  The best `top` bins are taken
there with `torch.topk` over the int64 key `(count << 32) | (0xFFFFFFFF - bin)`: the keys of a (filter, key) are distinct, so the
order is count descending, then value ascending (bins are numbered in ascending value), and deterministic.  One device-to-host read
per `count` call brings the winners, `missing`, `unbinned`, the number of non-zero bins and the totals.

`count_host` interprets exactly the arrays the kernel reads with numpy (the counterpart of `where_device.run_program_host`, for the CPU
tests); `oracle` counts with `collections.Counter` over the metadata dicts themselves and touches none of the column code.
"""
from __future__ import annotations

import math
from bisect import bisect_right
from collections import Counter
from typing import Dict, List, Optional, Sequence

import numpy as np

CODE, EXACT, INTERVAL = 0, 1, 2                      # ARX_FACET_*
MAX_KEYS, MAX_FILTERS, MAX_BINS, MAX_COUNTERS = 16, 64, 1 << 20, 1 << 27
_NUM, _STR, _BOOL = 1, 2, 3
_KINDS = {"number": _NUM, "string": _STR, "bool": _BOOL}
_LOW32 = 0xFFFFFFFF


# ---- specs -----------------------------------------------------------------------------------------------------------------------
def parse_spec(spec) -> Dict:
    """A facet spec -> {"key", "kind" (None: decided by the column), "edges" (None or a tuple of floats)}.  Reads no column: every
    malformed spec is a ValueError before anything is built or launched."""
    if isinstance(spec, str):
        return {"key": spec, "kind": None, "edges": None}
    if not isinstance(spec, dict):
        raise ValueError(f"facet spec must be a key name or a dict with \"key\", got {type(spec).__name__}")
    extra = set(spec) - {"key", "kind", "edges"}
    if extra:
        raise ValueError(f"facet spec {spec!r}: unknown field(s) {sorted(extra)} (a spec has \"key\" and \"kind\" or \"edges\")")
    key = spec.get("key")
    if not isinstance(key, str):
        raise ValueError(f"facet spec {spec!r}: \"key\" must be a metadata key name")
    kind, edges = spec.get("kind"), spec.get("edges")
    if kind is not None and kind not in _KINDS:
        raise ValueError(f"facet spec for {key!r}: kind={kind!r} is not one of {sorted(_KINDS)}")
    if edges is not None:
        if kind not in (None, "number"):
            raise ValueError(f"facet spec for {key!r}: edges bin numbers and cannot be combined with kind={kind!r}")
        if not isinstance(edges, (list, tuple)) or len(edges) < 2:
            raise ValueError(f"facet spec for {key!r}: edges must be a list of at least two numbers")
        for e in edges:
            if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, float, np.integer, np.floating)) or not math.isfinite(float(e)):
                raise ValueError(f"facet spec for {key!r}: edges must be finite numbers, got {e!r}")
        edges = tuple(float(e) for e in edges)
        if any(b <= a for a, b in zip(edges, edges[1:])):
            raise ValueError(f"facet spec for {key!r}: edges must ascend strictly, got {list(edges)}")
        if len(edges) - 1 > MAX_BINS:
            raise ValueError(f"facet spec for {key!r}: {len(edges) - 1} intervals, at most {MAX_BINS} are supported")
        kind = "number"
    return {"key": key, "kind": kind, "edges": edges}


class Facet:
    """One resolved spec: what the kernel takes for it (`mode`, `want_kind`, `n_bins`, `cuts`) and the value of every bin (`values`).
    `n_bins == 0`: no row of the shard has a value of the kind, the result is empty and the kernel is not entered."""

    def __init__(self, key, kind, mode, want_kind, values, cuts=None, interval=False):
        self.key, self.kind, self.mode, self.want_kind = key, kind, mode, want_kind
        self.values, self.n_bins, self.interval = values, len(values), interval
        self.cuts = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.float64)
        self._cuts_dev = None

    def cuts_device(self, device):
        import torch
        if self.cuts is not None and self._cuts_dev is None:
            self._cuts_dev = torch.from_numpy(self.cuts).to(device)
        return self._cuts_dev


def resolve(cols, spec) -> Facet:
    """A spec -> its `Facet` over the columns `cols` (a `where_device.MetadataColumns`).  A bare key is faceted over strings if any
    row has a string there, else over numbers, else over bools.  ValueError: a malformed spec; more than 2^20 distinct values."""
    p = parse_spec(spec)
    cached = (p["key"], p["kind"], p["edges"])                   # (the columns keep what was resolved until they are dropped)
    if cached not in cols._facets:
        cols._facets[cached] = _resolve(cols, p)
    return cols._facets[cached]


def _resolve(cols, p: Dict) -> Facet:
    key, kind = p["key"], p["kind"]
    if p["edges"] is not None:
        e = p["edges"]
        return Facet(key, "number", INTERVAL, _NUM, [(a, b) for a, b in zip(e, e[1:])], cuts=e, interval=True)
    if cols.n_rows == 0:
        return Facet(key, kind, CODE, _KINDS.get(kind, _STR), [])
    present = cols.kinds(key)
    if kind is None:
        kind = "string" if _STR in present else ("number" if _NUM in present else ("bool" if _BOOL in present else None))
    if kind is None or _KINDS[kind] not in present:              # no row has the key, or none a value of the kind asked for
        return Facet(key, kind, CODE, _KINDS.get(kind, _STR), [])
    if kind == "string":
        f = Facet(key, kind, CODE, _STR, cols.strings(key))
    elif kind == "bool":
        f = Facet(key, kind, CODE, _BOOL, [False, True])
    else:
        nums = cols.numbers(key)
        if len(nums) == 0:                                       # (only NaNs: one bin nothing falls into, so the rows count as unbinned)
            nums = np.zeros(1, dtype=np.float64)
        f = Facet(key, kind, EXACT, _NUM, nums.tolist(), cuts=nums)
    if f.n_bins > MAX_BINS:
        raise ValueError(f"facet key {key!r} has {f.n_bins} distinct values, at most {MAX_BINS} (2^20) are supported (there is no host path)")
    return f


# ---- results ---------------------------------------------------------------------------------------------------------------------
def _result(f: Facet, pairs, distinct: int, missing: int, unbinned: int, total: int) -> Dict:
    """`pairs`: (bin, count) in the order they are listed."""
    return {"key": f.key, "values": [f.values[b] for b, _ in pairs], "counts": [int(c) for _, c in pairs], "distinct": int(distinct),
            "missing": int(missing), "unbinned": int(unbinned), "total": int(total)}


def order_keys(counts: np.ndarray) -> np.ndarray:
    """int64 `(count << 32) | (0xFFFFFFFF - bin)` of every bin: descending, it is count descending then bin ascending."""
    c = np.asarray(counts, dtype=np.int64)
    return (c << 32) | (_LOW32 - np.arange(c.shape[-1], dtype=np.int64))


def _pairs_from_keys(keys) -> List:
    """Ordering keys (descending) -> (bin, count), the zero counts dropped."""
    return [(int(_LOW32 - (k & _LOW32)), int(k >> 32)) for k in (int(x) for x in keys) if (k >> 32) > 0]


def _from_counters(f: Facet, ctr: np.ndarray, top: Optional[int]) -> Dict:
    """The result of one (filter, key) from its n_bins + 2 counters."""
    nb = f.n_bins
    bins, missing, unbinned = ctr[:nb], int(ctr[nb]), int(ctr[nb + 1])
    if f.interval:
        pairs = [(b, int(c)) for b, c in enumerate(bins)]
    else:
        keys = np.sort(order_keys(bins))[::-1]
        pairs = _pairs_from_keys(keys if top is None else keys[:top])
    return _result(f, pairs, int((bins > 0).sum()), missing, unbinned, int(bins.sum()) + missing + unbinned)


def _check_top(top):
    if top is not None and (isinstance(top, bool) or not isinstance(top, (int, np.integer)) or top < 1):
        raise ValueError(f"top={top!r} must be a positive integer or None (every non-zero bin)")
    return None if top is None else int(top)


# ---- the host interpreter of the kernel's arrays -----------------------------------------------------------------------------------
def bin_counts_host(mode: int, want_kind: int, n_bins: int, cuts, kind: np.ndarray, val: np.ndarray, mask=None) -> np.ndarray:
    """int64 [n_bins + 2]: what `arx_facet_count` leaves for one (filter, key), from the same arrays (`mask`: bool [n] or None)."""
    kind, val = np.asarray(kind), np.asarray(val, dtype=np.float64)
    n = kind.shape[0]
    allowed = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[:n]
    right = allowed & (kind == want_kind)
    v = val[right]
    with np.errstate(invalid="ignore"):
        if mode == CODE:
            ok = (v >= 0.0) & (v < float(n_bins))
            idx = np.where(ok, v, 0.0).astype(np.int64)
            ok &= idx.astype(np.float64) == v
        elif mode == EXACT:
            s = np.asarray(cuts, dtype=np.float64)[:n_bins]
            idx = np.minimum(np.searchsorted(s, v, side="left"), n_bins - 1)
            ok = s[idx] == v
        else:
            s = np.asarray(cuts, dtype=np.float64)[:n_bins + 1]
            ok = (v >= s[0]) & (v <= s[n_bins])
            idx = np.clip(np.searchsorted(s, v, side="right") - 1, 0, n_bins - 1)
    out = np.zeros(n_bins + 2, dtype=np.int64)
    out[:n_bins] = np.bincount(idx[ok], minlength=n_bins)
    out[n_bins] = int(allowed.sum()) - int(right.sum())
    out[n_bins + 1] = int((~ok).sum())
    return out


def count_host(columns, specs: Sequence, masks=None, top: Optional[int] = 10) -> List[List[Dict]]:
    """`count` with numpy in the kernel's place: `columns` a `MetadataColumns` (its host columns are read), `masks` None (every row,
    one filter) or bool [F, n].  -> result[filter][key].  For the CPU tests; the product path never calls it."""
    top = _check_top(top)
    fs = [resolve(columns, s) for s in specs]
    n = columns.n_rows
    masks = [None] if masks is None else [np.asarray(m, dtype=bool) for m in masks]
    out = []
    for m in masks:
        total = n if m is None else int(m[:n].sum())
        row = []
        for f in fs:
            if f.n_bins == 0:
                row.append(_result(f, [], 0, total, 0, total))
                continue
            kind, val = columns.host_column(f.key)
            row.append(_from_counters(f, bin_counts_host(f.mode, f.want_kind, f.n_bins, f.cuts, kind, val, m), top))
        out.append(row)
    return out


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def _oracle_kind(v) -> Optional[str]:
    if isinstance(v, (bool, np.bool_)):
        return "bool"
    if isinstance(v, (int, float, np.integer, np.floating)):
        return "number"
    return "string" if isinstance(v, str) else None


def oracle(metadata: Sequence[Dict], lo: int, hi: int, specs: Sequence, masks=None, top: Optional[int] = 10) -> List[List[Dict]]:
    """The definition, row by row over the metadata dicts of rows [lo, hi) with `collections.Counter`: no columns, no codes, no bins.
    `masks`: None or one bool sequence over the rows [lo, hi) per filter.  -> result[filter][key]."""
    top = _check_top(top)
    rows = [metadata[r] if isinstance(metadata[r], dict) else {} for r in range(lo, hi)]
    masks = [None] if masks is None else list(masks)
    out = []
    for m in masks:
        allowed = [md for j, md in enumerate(rows) if m is None or bool(m[j])]
        res = []
        for spec in specs:
            p = parse_spec(spec)
            key, kind, edges = p["key"], p["kind"], p["edges"]
            if kind is None:
                seen = {_oracle_kind(md.get(key)) for md in rows}
                kind = next((k for k in ("string", "number", "bool") if k in seen), None)
            ctr, missing, unbinned = Counter(), 0, 0
            for md in allowed:
                v = md.get(key)
                if kind is None or _oracle_kind(v) != kind:
                    missing += 1
                elif kind == "string":
                    ctr[v] += 1
                elif kind == "bool":
                    ctr[bool(v)] += 1
                else:
                    x = float(v)
                    if x != x or (edges is not None and not (edges[0] <= x <= edges[-1])):
                        unbinned += 1
                    elif edges is not None:
                        ctr[min(bisect_right(edges, x) - 1, len(edges) - 2)] += 1
                    else:
                        ctr[0.0 if x == 0.0 else x] += 1
            if edges is not None:
                values = [(a, b) for a, b in zip(edges, edges[1:])]
                counts = [ctr[i] for i in range(len(values))]
            else:
                listed = sorted(ctr.items(), key=lambda kv: (-kv[1], kv[0]))
                listed = listed if top is None else listed[:top]
                values, counts = [k for k, _ in listed], [c for _, c in listed]
            res.append({"key": key, "values": values, "counts": counts, "distinct": sum(1 for c in ctr.values() if c > 0),
                        "missing": missing, "unbinned": unbinned, "total": len(allowed)})
        out.append(res)
    return out


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def launch(keys: Sequence, n_rows: int, allow, allow_stride: int, n_filters: int, out, out_stride: int, tuned=None, device=None) -> None:
    """One `arx_facet_count` (or, with `tuned = (block_threads, blocks_x, lds_bins)`, `arx_facet_count_tuned`) on the current stream.
    `keys`: (kind tensor, val tensor, cuts tensor or None, mode, want_kind, n_bins, out_off) each; `allow`: None or an int64 device
    tensor; `out`: int32 device tensor.  The library checks the limits; a refusal is an `ArxError` naming the field."""
    import torch
    from . import _lib
    lib = _lib.load()
    arr = (_lib.FacetKeyC * len(keys))()
    for a, (kind, val, cuts, mode, want, nb, off) in zip(arr, keys):
        a.kind, a.val, a.cuts = kind.data_ptr(), val.data_ptr(), None if cuts is None else cuts.data_ptr()
        a.mode, a.want_kind, a.n_bins, a.reserved, a.out_off = mode, want, nb, 0, off
    device = out.device if device is None else device
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        head = (arr, len(keys), n_rows, None if allow is None else allow.data_ptr(), allow_stride, n_filters, out.data_ptr(), out_stride)
        if tuned is None:
            _lib.check(lib.arx_facet_count(*head, stream), "arx_facet_count")
        else:
            _lib.check(lib.arx_facet_count_tuned(*head, *tuned, stream), "arx_facet_count_tuned")


def _as_bitmaps(bitmaps, n_words: int, device):
    """None | tensor [W] | tensor [F, W] | list of [W] tensors -> (None or contiguous int64 [F, W], F)."""
    import torch
    if bitmaps is None:
        return None, 1
    t = bitmaps if torch.is_tensor(bitmaps) else torch.stack(list(bitmaps))
    t = t[None] if t.dim() == 1 else t
    if not (t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == n_words and t.shape[0] >= 1):
        raise ValueError(f"bitmaps must be int64 device tensors of {n_words} words each")
    return t.contiguous(), int(t.shape[0])


def count(cols, specs: Sequence, bitmaps=None, top: Optional[int] = 10) -> List[List[Dict]]:
    """-> result[filter][key], each `{key, values, counts, distinct, missing, unbinned, total}`: the facet counts of `specs` over the
    device columns `cols` under every row bitmap of `bitmaps` (None: every row, one filter; an int64 device tensor [W] or [F, W], or a
    list of [W] tensors, W = ceil(n_rows / 64), in the convention of `where.pack_bitmap`).  One `arx_facet_count` per 16 keys and 64
    filters (fewer filters where 64 slices of counters would exceed 2^27); the counters stay on the device, where the best `top` bins
    of every (filter, key) are taken (`top=None`: every bin goes to the host and the non-zero ones are listed; an `edges` facet lists
    every bin in order and ignores `top`).  One device-to-host read per call."""
    import torch
    from . import _lib
    top = _check_top(top)
    parsed = [parse_spec(s) for s in specs]                     # (every malformed spec is refused before a column is built)
    if cols.device is None:
        raise ValueError("MetadataColumns was built without a device: facets.count needs one (there is no host fallback)")
    dev, n = cols.device, cols.n_rows
    bits, nf = _as_bitmaps(bitmaps, cols.n_words, dev)
    fs = [resolve(cols, p) for p in parsed]
    if n == 0:
        return [[_result(f, [], 0, 0, 0, 0) for f in fs] for _ in range(nf)]
    live = [j for j, f in enumerate(fs) if f.n_bins > 0]
    pieces, layout = [], []                                     # int64 device tensors [Fc, w]; (what, key j, filter lo, Fc, w)
    if not live:                                                # only the totals are needed: the rows each bitmap allows
        if bits is not None:
            tot = torch.empty(nf, dtype=torch.int64, device=dev)
            lib = _lib.load()
            with torch.cuda.device(dev):
                for f in range(nf):
                    _lib.check(lib.arx_bitmap_count(bits[f].data_ptr(), n, tot[f:f + 1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                               "arx_bitmap_count")
            pieces.append(tot[:, None])
            layout.append(("total", -1, 0, nf, 1))
    for k0 in range(0, len(live), MAX_KEYS):
        chunk = live[k0:k0 + MAX_KEYS]
        offs, stride = [], 0
        for j in chunk:
            offs.append(stride)
            stride += fs[j].n_bins + 2
        per_call = max(1, min(MAX_FILTERS, MAX_COUNTERS // stride))
        keys = [(*cols.device_column(fs[j].key), fs[j].cuts_device(dev), fs[j].mode, fs[j].want_kind, fs[j].n_bins, off)
                for j, off in zip(chunk, offs)]
        for f0 in range(0, nf, per_call):
            fc = min(per_call, nf - f0)
            out = torch.empty((fc, stride), dtype=torch.int32, device=dev)
            launch(keys, n, None if bits is None else bits[f0:f0 + fc], 0 if bits is None else cols.n_words, fc, out, stride, device=dev)
            for j, off in zip(chunk, offs):
                f, nb = fs[j], fs[j].n_bins
                cnt = out[:, off:off + nb].to(torch.int64)
                tail = out[:, off + nb:off + nb + 2].to(torch.int64)
                stats = torch.cat([tail, (cnt > 0).sum(1, keepdim=True), cnt.sum(1, keepdim=True) + tail.sum(1, keepdim=True)], dim=1)
                if f.interval:
                    best = cnt
                else:
                    key64 = (cnt << 32) | (_LOW32 - torch.arange(nb, dtype=torch.int64, device=dev))
                    best = torch.topk(key64, nb if top is None else min(top, nb), dim=1).values
                pieces += [stats, best]
                layout += [("stats", j, f0, fc, 4), ("best", j, f0, fc, int(best.shape[1]))]
    host = torch.cat([p.reshape(-1) for p in pieces]).cpu().numpy() if pieces else np.zeros(0, np.int64)      # the one read
    got, at = {}, 0
    for what, j, f0, fc, w in layout:
        block = host[at:at + fc * w].reshape(fc, w)
        at += fc * w
        for i in range(fc):
            got[(what, j, f0 + i)] = block[i]
    res = []
    for fi in range(nf):
        if live:
            total = int(got[("stats", live[0], fi)][3])
        else:
            total = n if bits is None else int(got[("total", -1, fi)][0])
        row = []
        for j, f in enumerate(fs):
            if f.n_bins == 0:
                row.append(_result(f, [], 0, total, 0, total))
                continue
            missing, unbinned, distinct, tot = (int(x) for x in got[("stats", j, fi)])
            best = got[("best", j, fi)]
            pairs = [(b, int(c)) for b, c in enumerate(best)] if f.interval else _pairs_from_keys(best)
            row.append(_result(f, pairs, distinct, missing, unbinned, tot))
        res.append(row)
    return res
