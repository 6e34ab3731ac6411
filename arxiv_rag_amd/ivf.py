"""IVF probe search: score a query against the rows of its `nprobe` nearest topics only (`arx_ivf_search`, include/arx.h;
INTEGRATION.md "IVF probe search").

    ivf = IvfIndex.build(index, n_lists=4096)                 # index: a ShardIndex; k-means on a sample, every row labelled
    scores, ids, scanned = ivf.search(q, k=10, nprobe=32)     # q: fp16 device [nq, dim]

The coarse quantiser is `topics.kmeans`, the labels come from `topics.predict`, the lists are `topics.members`' `order` / `start`.
`probe` is the exact top-`nprobe` centroids of every query (a `ShardIndex` over the fp16 centroids), and `search` is the exact top-k of
the rows of those lists: which rows a query may see is the approximation, everything after that has the score bits and the order of
every other search here (`exact_row_score`, score desc, row asc), so the answer equals `ShardIndex.search(allow=...)` over the
bitmap of the probed lists' rows, bit for bit.  `nprobe = n_lists` is the exact search.

`search_many` is `search` with a row filter per query and a score threshold per query (`arx_ivf_search_multi`): one call per batch
whatever the number of distinct filters, and `hits`, the exact number of rows at or above the threshold, as a fourth result.  Both
reach the library through `_launch`, the one place that calls it (`ivf_search` and `ivf_search_multi` name the entry point).

`check_probe_args`, `probe_bitmaps_host`, `search_host` and `search_many_host` restate the refusals and the definitions with numpy (for
the tests; the product path never calls the last three).  The rows are ranked in one loop, `search_many_host`'s: `search_host` is that
function with one filter for every query and no threshold.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np

MAX_PROBE, MAX_LISTS, MAX_K = 128, 4096, 32
PREDICT_ROWS = 1 << 22          # rows per `topics.predict` call of a build (bounds the assign's workspace)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_probe_args(k, nprobe, n_lists: int) -> None:
    """The refusals of `IvfIndex.search` / `probe` about k and nprobe, each a ValueError before anything is launched."""
    if not _is_int(k) or not (1 <= k <= MAX_K):
        raise ValueError(f"k={k!r} must be an integer in [1, {MAX_K}] (the search's k limit)")
    if not _is_int(nprobe) or not (1 <= nprobe <= MAX_PROBE):
        raise ValueError(f"nprobe={nprobe!r} must be an integer in [1, {MAX_PROBE}]")
    if nprobe > n_lists:
        raise ValueError(f"nprobe={nprobe} exceeds the index's n_lists={n_lists}")


def check_build_args(n_rows: int, dim: int, n_lists, iters, train_rows) -> int:
    """The refusals of `IvfIndex.build`, each a ValueError before anything is launched -> the number of training rows."""
    from .topics import check_args
    if n_rows >= 1 << 31:
        raise ValueError(f"n_rows={n_rows} must be below 2^31 (the lists hold int32 rows)")
    check_args(max(n_rows, 1), dim, n_lists, iters)
    if train_rows is None:
        return min(n_rows, 256 * int(n_lists))
    if not _is_int(train_rows) or not (int(n_lists) <= train_rows <= n_rows):
        raise ValueError(f"train_rows={train_rows!r} must be an integer in [n_lists, rows] = [{int(n_lists)}, {n_rows}], or None")
    return int(train_rows)


def check_query_with_nprobe(nprobe, *, has_index: bool, n_lists: int = 0, per_query_filters: bool = False, hybrid_alpha=None, group_by=None,
                            min_score=None, world: int = 1, n_width: int = 1, allow_per_query_filters: bool = False,
                            allow_min_score: bool = False) -> None:
    """The refusals of `query(nprobe=...)`, `retrieve` and `search_queries`, each a ValueError naming the part, before any launch.
    `allow_per_query_filters` / `allow_min_score` (default off): `retrieve` and `search_queries`, which route such a batch through
    `IvfIndex.search_many`, pass them, and per-query filter lists / `min_score` are then let through; everything else is refused as
    without them (`HipCollection.query` does not pass them)."""
    from .modes import check_mode
    check_mode("nprobe", nprobe, has_index=has_index, per_query=per_query_filters, hybrid_alpha=hybrid_alpha, group_by=group_by,
               min_score=min_score, world=world, n_width=n_width, n_lists=n_lists,
               let_through=("per_query",) * bool(allow_per_query_filters) + ("min_score",) * bool(allow_min_score))


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def _visible_rows(order, start, probe_row, n_rows: int, max_list_rows=None) -> np.ndarray:
    """The rows one query sees, in list order: the distinct valid lists of `probe_row` in probe order, `start` as `clamp_starts`
    reads it, each list cut at its first `max_list_rows` entries (None: whole), `order` entries outside [0, n_rows) dropped (after the
    cut: such an entry keeps its place inside it)."""
    from .topics import clamp_starts
    order = np.asarray(order, dtype=np.int64)
    s = clamp_starts(start, order.shape[0])
    n_lists, seen, rows = s.shape[0] - 1, set(), []
    for c in np.asarray(probe_row, dtype=np.int64).tolist():
        if 0 <= c < n_lists and c not in seen:
            seen.add(c)
            end = int(s[c + 1]) if max_list_rows is None else min(int(s[c + 1]), int(s[c]) + int(max_list_rows))
            rows.append(order[int(s[c]):end])
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return rows[(rows >= 0) & (rows < n_rows)]


def probe_bitmaps_host(order, start, probes, n_rows: int, max_list_rows=None) -> np.ndarray:
    """int64 [nq, ceil(n_rows / 64)]: per query the bitmap (`where.pack_bitmap`'s convention) of the rows it sees (`max_list_rows`:
    as `_visible_rows` cuts the lists)."""
    from .where import pack_bitmap
    probes = np.asarray(probes)
    out = np.zeros((probes.shape[0], (n_rows + 63) // 64), np.int64)
    for q in range(probes.shape[0]):
        mask = np.zeros(n_rows, bool)
        mask[_visible_rows(order, start, probes[q], n_rows, max_list_rows)] = True
        out[q] = pack_bitmap(mask).view(np.int64)
    return out


def search_host(X, order, start, probes, Q, k: int, allow=None, max_list_rows=None):
    """(scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq]): what `arx_ivf_search` returns with idx_base = 0, bit for bit, from
    `topics.exact_scores_host`.  `X` fp16 [n_rows, dim], `Q` fp16 [nq, dim], `probes` int [nq, nprobe]; `allow`: None, a bool mask
    [n_rows] or bitmap words (int64 / uint64 [ceil(n_rows / 64)]).  `search_many_host` with that one filter for every query."""
    nq = np.asarray(Q).shape[0]
    allows = None if allow is None else np.asarray(allow)[None]
    return search_many_host(X, order, start, probes, Q, k, allows=allows, filter_of=np.zeros(nq, np.int64), max_list_rows=max_list_rows)[:3]


def _thresholds(min_score, nq: int) -> np.ndarray:
    """f32 [nq] from a float or one value per query."""
    from .ranging import thresholds
    return thresholds(min_score, nq, each="entry")


def search_many_host(X, order, start, probes, Q, k: int, allows=None, filter_of=None, min_score=None, max_list_rows=None):
    """(scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq], hits int64 [nq]): what `arx_ivf_search_multi` returns with
    idx_base = 0, bit for bit.  `allows`: None (no filter; `filter_of` is ignored), bool masks [F, n_rows] or bitmap words (int64 /
    uint64 [F, ceil(n_rows / 64)]); `filter_of` int [nq]: query q sees the rows of `search_host` under `allows[filter_of[q]]`, and no
    row when `filter_of[q]` lies outside [0, F).  `scanned` counts the visible rows.  `min_score`: None, a float or one per query; a
    visible row qualifies when its f32 score `>=` the query's f32 threshold (a NaN on either side: not), and with None every visible
    row qualifies.  `hits` counts the qualifying rows (with None: `hits == scanned`); the list is their best k by (score desc, row
    asc), `lexsort`ed from `topics.exact_scores_host`.  `max_list_rows`: None, or the entries a list is read up to (the library's
    argument of that name): `scanned` and `hits` count rows inside the cut alone."""
    from .mutation import unpack_rows
    from .topics import exact_scores_host
    X, Q, probes = np.asarray(X), np.asarray(Q), np.asarray(probes)
    n_rows, nq = X.shape[0], Q.shape[0]
    masks = None
    if allows is not None:
        allows = np.asarray(allows)
        assert allows.ndim == 2 and filter_of is not None
        masks = allows if allows.dtype == bool else np.stack([unpack_rows(a, n_rows) for a in allows]) if allows.shape[0] else np.zeros((0, n_rows), bool)
        filter_of = np.asarray(filter_of, dtype=np.int64)
        assert filter_of.shape == (nq,)
    thr = None if min_score is None else _thresholds(min_score, nq)
    scores = np.full((nq, k), -np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    scanned, hits = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        rows = _visible_rows(order, start, probes[q], n_rows, max_list_rows)
        if masks is not None:
            f = int(filter_of[q])
            rows = rows[masks[f][rows]] if 0 <= f < masks.shape[0] else rows[:0]
        scanned[q] = hits[q] = rows.shape[0]
        if rows.shape[0] == 0:
            continue
        sc = exact_scores_host(X[rows], Q[q:q + 1])[:, 0].astype(np.float32, copy=False)
        if thr is not None:
            ok = sc >= thr[q]                                    # the f32 compare: False where either side is NaN
            rows, sc = rows[ok], sc[ok]
            hits[q] = rows.shape[0]
        best = np.lexsort((rows, -sc))[:k]                       # score desc, row asc (-0.0 and +0.0 tie, as the kernel compares them)
        scores[q, :best.shape[0]], ids[q, :best.shape[0]] = sc[best], rows[best]
    return scores, ids, scanned, hits


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def _launch(corpus, order, start, max_list_rows, q, probes, k, allow, per_query, idx_base, rows_per_block, ws, n_rows):
    """The one call into the library.  `per_query` None: `arx_ivf_search[_tuned]`, `allow` one bitmap or None -> (scores, ids, scanned).
    `per_query` (n_filters, filter_of, min_score): `arx_ivf_search_multi[_tuned]`, `allow` [n_filters, words] or None -> (scores, ids,
    scanned, hits).  Checks the tensors, allocates the outputs, uses `ws` if it holds the entry's workspace and a new one if not."""
    import torch
    from . import _lib
    lib = _lib.load()
    name, ws_bytes = ("arx_ivf_search", lib.arx_ivf_workspace_bytes) if per_query is None else ("arx_ivf_search_multi", lib.arx_ivf_multi_workspace_bytes)
    n_rows = int(corpus.shape[0]) if n_rows is None else int(n_rows)
    dim, nq, n_probe = int(corpus.shape[1]), int(q.shape[0]), int(probes.shape[1])
    n_members, n_lists = int(order.shape[0]), int(start.shape[0]) - 1
    assert corpus.is_cuda and corpus.dtype == torch.float16 and corpus.is_contiguous()
    assert q.is_cuda and q.dtype == torch.float16 and q.dim() == 2 and q.shape[1] == dim and q.is_contiguous()
    assert order.is_cuda and order.dtype == torch.int32 and order.dim() == 1 and order.is_contiguous()
    assert start.is_cuda and start.dtype == torch.int64 and start.dim() == 1 and start.is_contiguous()
    assert probes.is_cuda and probes.dtype == torch.int32 and probes.shape == (nq, n_probe) and probes.is_contiguous()
    if allow is not None:
        assert allow.is_cuda and allow.dtype in (torch.int64, torch.uint64) and allow.is_contiguous()
        assert allow.dim() == (1 if per_query is None else 2) and allow.shape[-1] == (n_rows + 63) // 64
    n_filters, filter_of, min_score = per_query or (None, None, None)
    if filter_of is not None:
        assert filter_of.is_cuda and filter_of.dtype == torch.int32 and filter_of.shape == (nq,) and filter_of.is_contiguous()
    if min_score is not None:
        assert min_score.is_cuda and min_score.dtype == torch.float32 and min_score.shape == (nq,) and min_score.is_contiguous()
    out =[torch.empty((nq, k), dtype=torch.float32, device=q.device), torch.empty((nq, k), dtype=torch.int64, device=q.device)]
    out += [torch.empty((nq,), dtype=torch.int64, device=q.device) for _ in range(1 if per_query is None else 2)]      # scanned[, hits]
    if nq == 0:
        return tuple(out)
    need = ws_bytes(n_members, n_lists, nq, n_probe, dim, k)
    if need < 0:
        raise _lib.ArxError(f"{name}: unsupported shape n_members={n_members} n_lists={n_lists} nq={nq} n_probe={n_probe} dim={dim} k={k}")
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)

    def ptr(t):
        return None if t is None else t.data_ptr()
    args = [corpus.data_ptr(), n_rows, dim, order.data_ptr() if n_members else None, n_members, start.data_ptr(), n_lists, int(max_list_rows),
            q.data_ptr(), nq, probes.data_ptr(), n_probe, ptr(allow)]
    if per_query is not None:
        args += [n_filters, ptr(filter_of), ptr(min_score)]
    args += [int(k)] + [t.data_ptr() for t in out] + [int(idx_base), ws.data_ptr(), ws.numel() * ws.element_size()]
    if rows_per_block is not None:
        name, args = name + "_tuned", args + [int(rows_per_block)]
    with torch.cuda.device(q.device):
        _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream(q.device).cuda_stream), name)
    return tuple(out)


def ivf_search(corpus, order, start, max_list_rows: int, q, probes, k: int, allow=None, idx_base: int = 0, rows_per_block: Optional[int] = None,
               ws=None, n_rows: Optional[int] = None):
    """`arx_ivf_search` (or, with `rows_per_block` given, `arx_ivf_search_tuned`) on the current stream.  `corpus` fp16 device
    [n_rows, dim], `order` int32 device [n_members], `start` int64 device [n_lists + 1], `q` fp16 device [nq, dim], `probes` int32 device
    [nq, nprobe], `allow` int64 / uint64 device words or None -> (scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq]) on the
    device.  `ws`: a device uint8 tensor to use as the workspace if it is large enough.  The library checks the contract; a refusal
    is an `ArxError` naming the field."""
    return _launch(corpus, order, start, max_list_rows, q, probes, k, allow, None, idx_base, rows_per_block, ws, n_rows)


def ivf_search_multi(corpus, order, start, max_list_rows: int, q, probes, k: int, allows=None, filter_of=None, min_score=None, idx_base: int = 0,
                     rows_per_block: Optional[int] = None, ws=None, n_rows: Optional[int] = None, _n_filters: Optional[int] = None):
    """`arx_ivf_search_multi` (or, with `rows_per_block` given, `arx_ivf_search_multi_tuned`) on the current stream: `ivf_search` with
    a bitmap per query and a threshold per query.  `allows` int64 / uint64 device [n_filters, ceil(n_rows / 64)] or None, `filter_of`
    int32 device [nq] (query q is restricted by `allows[filter_of[q]]`; outside [0, n_filters): the query sees no row), `min_score`
    float32 device [nq] or None -> (scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq], hits int64 [nq]) on the device; `hits`
    is the exact number of visible rows with score >= the query's threshold (without `min_score`: `scanned`), the lists hold the best k
    of those.  The library checks the contract; a refusal is an `ArxError` naming the field (`_n_filters`: a test hook, the n_filters
    the library is told instead of `allows.shape[0]`)."""
    n_filters = (0 if allows is None else int(allows.shape[0])) if _n_filters is None else int(_n_filters)
    return _launch(corpus, order, start, max_list_rows, q, probes, k, allows, (n_filters, filter_of, min_score), idx_base, rows_per_block, ws, n_rows)


class IvfIndex:
    """The inverted lists of a `ShardIndex`: `centroids` (a `ShardIndex` over the fp16 centroids, for the coarse step), `labels` (int32
    device, one per row), `order` / `start` (`topics.members`), `sizes` and `max_list_rows` (read once when the lists are set)."""

    def __init__(self, index, centroids_f16, labels, info: Optional[Dict] = None):
        from .index import ShardIndex
        self.index = index
        self.centroids_f16 = centroids_f16.contiguous()
        self.n_lists = int(self.centroids_f16.shape[0])
        self.centroids = ShardIndex(self.centroids_f16, prefilter=None)
        self.info = dict(info or {})
        self._ws = None
        self.set_labels(labels)

    def set_labels(self, labels) -> None:
        """The lists of these labels (int32 device, one per row of the index, each in [0, n_lists)): `order`, `start`, `sizes`, and the
        longest list (one host read)."""
        from .topics import members
        self.labels = labels
        self.order, self.start, self.sizes = members(labels.long(), self.n_lists)
        self.max_list_rows = int(self.sizes.max().item()) if labels.shape[0] else 0

    def rows_added(self, lo: int, hi: int, rows, index=None) -> None:
        """The shard grew by `rows` (fp16 device [hi - lo, dim]): they are labelled against the kept centroids and the lists rebuilt;
        `index`: the `ShardIndex` over the grown shard, where the caller made a new one."""
        import torch
        if index is not None:
            self.index = index
        self.set_labels(torch.cat([self.labels, label_rows(rows, self.centroids_f16)]))

    def rows_compacted(self, keep_words, word_rank, count: int, index=None) -> None:
        """The labels move as the shard's rows moved (`arx_compact_rows`, 4-byte rows) and the lists are rebuilt."""
        import torch
        from .mutation import compact_rows_device
        moved = torch.zeros_like(self.labels)
        compact_rows_device(self.labels.contiguous(), moved, int(self.labels.shape[0]), keep_words, word_rank)
        if index is not None:
            self.index = index
        self.set_labels(moved[:count].contiguous())

    @classmethod
    def build(cls, index, n_lists: int, iters: int = 10, seed: int = 0, train_rows: Optional[int] = None) -> "IvfIndex":
        """k-means (`topics.kmeans`) on a sample of the shard's rows (`numpy.random.default_rng(seed).choice`, sorted ascending;
        `train_rows=None`: min(n_rows, 256 n_lists) rows; a sample equal to the shard is the shard itself, without a gather), then
        `topics.predict` over all rows in slices and `topics.members`.  Deterministic: two builds with one seed give the same lists.
        ValueError before any launch: the refusals of `topics.check_args` about dim, n_lists and iters; `train_rows` outside
        [n_lists, n_rows]; n_rows >= 2^31."""
        import torch
        from . import topics as T
        n = int(index.n_rows)
        m = check_build_args(n, int(index.dim), n_lists, iters, train_rows)
        t0 = time.perf_counter()
        X = index.corpus[:n]
        if m == n:
            sample = X
        else:
            rows = np.sort(np.random.default_rng(seed).choice(n, m, replace=False)).astype(np.int64)
            sample = T.gather(index, torch.from_numpy(rows).to(X.device))
        res = T.kmeans(sample, int(n_lists), iters=int(iters), seed=seed)
        c16 = res["centroids_f16"].contiguous()
        labels = label_rows(X, c16)
        self = cls(index, c16, labels, {"iterations": res["iterations"], "train_rows": m})
        torch.cuda.synchronize(X.device)
        self.info["seconds"] = time.perf_counter() - t0
        return self

    def summary(self) -> Dict:
        """{n_lists, list_rows_min / median / max, iterations, train_rows, seconds}."""
        sizes = self.sizes.cpu().numpy()
        return {"n_lists": self.n_lists, "list_rows_min": int(sizes.min()), "list_rows_median": float(np.median(sizes)),
                "list_rows_max": int(sizes.max()), **self.info}

    def probe(self, q, nprobe: int):
        """int32 device [nq, nprobe]: the exact top-`nprobe` centroids of every query, by (score desc, centroid asc): up to 32 the
        centroid index's `search`, beyond it `search_range(-inf, nprobe)` (the same score bits and order)."""
        import torch
        check_probe_args(1, nprobe, self.n_lists)
        if nprobe <= 32:
            _, ids = self.centroids.search(q, int(nprobe))
        else:
            _, ids, _ = self.centroids.search_range(q, float("-inf"), int(nprobe))
        return ids.to(torch.int32).contiguous()

    def _prepare(self, q, k: int, nprobe: int, probes, workspace_bytes):
        """What `search` and `search_many` do first -> the probes: the refusals about k and nprobe, `probe(q, nprobe)` unless `probes`
        is given, and `_ws` (a uint8 device tensor that only grows) made to hold `workspace_bytes` (the entry point's own) of the call."""
        check_probe_args(k, nprobe, self.n_lists)
        if probes is None:
            probes = self.probe(q, nprobe)
        need = workspace_bytes(int(self.order.shape[0]), self.n_lists, max(int(q.shape[0]), 1), int(nprobe), self.index.dim, int(k))
        if need > 0 and (self._ws is None or self._ws.numel() < need):
            import torch
            self._ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        return probes

    def search(self, q, k: int, nprobe: int, allow=None, probes=None, rows_per_block: Optional[int] = None):
        """(scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq]) on the device: the exact top-k of the rows of every query's
        `nprobe` nearest lists (`probes`: int32 device [nq, nprobe] to use instead of `probe(q, nprobe)`), restricted by the bitmap
        `allow` as `ShardIndex.search(allow=...)` restricts; ids = local row + the index's idx_base; `scanned` the rows scored."""
        probes = self._prepare(q, k, nprobe, probes, self.index.lib.arx_ivf_workspace_bytes)
        if allow is not None:
            self.index._check_allow(allow)
        return ivf_search(self.index.corpus, self.order, self.start, self.max_list_rows, q, probes, int(k), allow=allow, idx_base=self.index.idx_base,
                          rows_per_block=rows_per_block, ws=self._ws, n_rows=self.index.n_rows)

    def search_many(self, q, k: int, nprobe: int, allows=None, filter_of=None, min_score=None, probes=None, rows_per_block: Optional[int] = None):
        """(scores f32 [nq, k], ids int64 [nq, k], scanned int64 [nq], hits int64 [nq]) on the device: `search` with a bitmap per
        query and a threshold per query, in one call whatever the number of distinct filters (`arx_ivf_search_multi`).  `allows`:
        int64 / uint64 device [n_filters, ceil(n_rows / 64)] with `filter_of` int32 device [nq] (a value outside [0, n_filters): that
        query sees no row), or None.  `min_score`: None, a float, or a sequence or tensor of one per query; a visible row qualifies
        when its f32 score is >= the threshold (NaN on either side: not).  `hits` is the exact number of qualifying rows (without
        `min_score`: `scanned`), the lists their best k.  Reuses the index's cached workspace."""
        import torch
        from .ranging import device_thresholds
        probes = self._prepare(q, k, nprobe, probes, self.index.lib.arx_ivf_multi_workspace_bytes)
        if allows is not None:
            if not (torch.is_tensor(allows) and allows.dim() == 2 and allows.shape[0] >= 1):
                raise ValueError("allows must be a 2-d device tensor [n_filters >= 1, ceil(n_rows / 64)]")
            if filter_of is None:
                raise ValueError("allows needs filter_of: one filter index per query")
        if min_score is not None:
            min_score = device_thresholds(min_score, int(q.shape[0]), q.device)
        return ivf_search_multi(self.index.corpus, self.order, self.start, self.max_list_rows, q, probes, int(k), allows=allows, filter_of=filter_of,
                                min_score=min_score, idx_base=self.index.idx_base, rows_per_block=rows_per_block, ws=self._ws,
                                n_rows=self.index.n_rows)


def label_rows(X, centroids_f16):
    """int32 device [n]: `topics.predict` of the rows of `X` (fp16 device, dense) against the fp16 centroids, in slices of at most
    `PREDICT_ROWS` rows; the norm bound is measured once."""
    import torch
    from . import topics as T
    n = int(X.shape[0])
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    if n == 0:
        return labels
    with torch.cuda.device(X.device):
        bound = T.centroid_norm_bound(centroids_f16)
    for a in range(0, n, PREDICT_ROWS):
        b = min(n, a + PREDICT_ROWS)
        labels[a:b] = T.predict(X[a:b], centroids_f16, norm_bound=bound)[0]
    return labels
