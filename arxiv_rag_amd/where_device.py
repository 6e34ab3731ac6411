"""Chroma `where` filters evaluated on the GPU from metadata columns that stay in HBM (`arx_where_eval`, include/arx.h).

    cols = MetadataColumns(metadata, lo, hi, device="cuda:0")            # this rank's rows [lo, hi); nothing is built yet
    bits, counts = cols.allow_many([compile_where(f) for f in filters])  # int64 [F, ceil(n / 64)] on the device, list of F ints

The host path (`where.evaluate` + `where.pack_bitmap` + an upload per filter) stays what it was and is this module's oracle: the device
path produces the same bits.

Columns.  One column per metadata key, built over the rows [lo, hi) on first use and cached (like the host cache it is a snapshot of
the metadata at that moment).  A column costs 9 bytes per row and key in HBM:
  kind  uint8 [n]    0 = the key is absent or holds a value of another type, 1 = number, 2 = string, 3 = bool (`where._kind`)
  val   float64 [n]  float(v) for a number; the string's code for a string; 0.0 / 1.0 for a bool; 0.0 otherwise
A string's code is its rank in sorted(set(strings of this key in [lo, hi))): Python compares `str` by code point, and so does the host
evaluator, so `s < t` <=> `code(s) < code(t)`.  The sorted list stays on the host, where the operands are translated.

Lowering.  A compiled filter (`where.compile_where`) becomes a postfix program over leaves
  (column, want_kind, op, operand f64, negate, set_off, set_len),   op in EQ GT GE LT LE IN NEVER
a leaf being true for row r when `(kind[r] == want_kind and cmp(val[r], operand)) != negate`.  `$ne` / `$nin` are the negation of
"has the kind and equals / is in", so a row that lacks the key passes them, as on the host.  A string operand x becomes, with
lo = bisect_left(D, x) and hi = bisect_right(D, x) on the key's sorted list D:  $eq -> EQ lo (NEVER if x is not in D), $gt -> GE hi,
$gte -> GE lo, $lt -> LT lo, $lte -> LT hi.  `$in` / `$nin` become an ascending list of distinct f64 (numbers through float, -0.0 folded
into 0.0, NaN dropped; strings as codes, absent strings dropped; an empty list is NEVER); the lists of all leaves of a call lie in one
device array.  The tree becomes int32 tokens `(arg << 2) | code`: LEAF i, AND n, OR n (n-ary).

Limits.  A filter has at most 32 leaves, 96 tokens, 32 nested `$and` / `$or` levels and stack depth 32; a call holds at most 64 filters and
2^20 set values.  A filter beyond a limit is evaluated by the host path instead (same bits; `MetadataColumns.paths` counts them): never
an error.
"""
from __future__ import annotations

from bisect import bisect_left, bisect_right
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .where import _kind

EQ, GT, GE, LT, LE, IN, NEVER = range(7)
LEAF, AND, OR = 0, 1, 2
MAX_LEAVES, MAX_TOKENS, MAX_DEPTH, MAX_FILTERS, MAX_SET_VALS = 32, 96, 32, 64, 1 << 20
BYTES_PER_ROW_AND_KEY = 9
# arx_where_leaf (include/arx.h): 32 bytes, no padding
LEAF_DTYPE = np.dtype([("operand", "<f8"), ("column", "<i4"), ("want_kind", "<i4"), ("op", "<i4"), ("negate", "<i4"), ("set_off", "<i4"),
                       ("set_len", "<i4")])
_NUM, _STR, _BOOL = 1, 2, 3
_ORDER = {"$gt": GT, "$gte": GE, "$lt": LT, "$lte": LE}


class BeyondLimits(ValueError):
    """The filter is past a limit of the device path (the caller evaluates it on the host)."""


class Program:
    """The arrays one `arx_where_eval` call takes, on the host.  `keys[c]` is the metadata key of column c."""

    def __init__(self, keys, leaves, leaf_off, tokens, token_off, set_vals):
        self.keys: List[str] = list(keys)
        self.leaves = np.ascontiguousarray(leaves, dtype=LEAF_DTYPE)
        self.leaf_off = np.ascontiguousarray(leaf_off, dtype=np.int32)
        self.tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        self.token_off = np.ascontiguousarray(token_off, dtype=np.int32)
        self.set_vals = np.ascontiguousarray(set_vals, dtype=np.float64)

    @property
    def n_filters(self) -> int:
        return int(self.leaf_off.shape[0]) - 1


def _set_values(vals, strings: Optional[List[str]]) -> List[float]:
    kind = _kind(vals[0])
    if kind == _STR:
        out = set()
        for x in vals:
            i = bisect_left(strings, x)
            if i < len(strings) and strings[i] == x:
                out.add(float(i))
        return sorted(out)
    if kind == _BOOL:
        return sorted({1.0 if x else 0.0 for x in vals})
    out = set()
    for x in vals:
        x = float(x)
        if x != x:
            continue
        out.add(0.0 if x == 0.0 else x)
    return sorted(out)


def lower_filter(tree: Tuple, strings_of: Callable[[str], List[str]]):
    """One compiled filter -> (leaves, tokens, set values): leaves as tuples (key, want_kind, op, operand, negate, set_off, set_len) with
    set_off counted within this filter.  BeyondLimits names the limit it is past."""
    leaves, tokens, sets = [], [], []

    def leaf(key, want, op, operand=0.0, negate=0, vals=()):
        if len(leaves) >= MAX_LEAVES:
            raise BeyondLimits(f"more than {MAX_LEAVES} leaves")
        leaves.append((key, want, op, float(operand), int(negate), len(sets) if len(vals) else 0, len(vals)))
        sets.extend(vals)
        tokens.append(((len(leaves) - 1) << 2) | LEAF)

    def go(node, depth):
        if node[0] in ("and", "or"):
            if depth >= MAX_DEPTH:
                raise BeyondLimits(f"more than {MAX_DEPTH} nested levels")
            for child in node[1]:
                go(child, depth + 1)
            tokens.append((len(node[1]) << 2) | (AND if node[0] == "and" else OR))
            return
        what, key, op, val = node
        if what == "set":
            kind = _kind(val[0])
            vals = _set_values(val, strings_of(key) if kind == _STR else None)
            leaf(key, kind, IN if vals else NEVER, 0.0, op == "$nin", vals)
            return
        kind = _kind(val)
        negate = op == "$ne"
        if kind == _BOOL:
            leaf(key, kind, EQ, 1.0 if val else 0.0, negate)
        elif kind == _NUM:
            leaf(key, kind, EQ if op in ("$eq", "$ne") else _ORDER[op], float(val), negate)
        else:
            d = strings_of(key)
            lo, hi = bisect_left(d, val), bisect_right(d, val)
            if op in ("$eq", "$ne"):
                leaf(key, kind, EQ if lo < hi else NEVER, lo, negate)
            else:
                leaf(key, kind, *{"$gt": (GE, hi), "$gte": (GE, lo), "$lt": (LT, lo), "$lte": (LT, hi)}[op])

    go(tree, 0)
    if len(tokens) > MAX_TOKENS:
        raise BeyondLimits(f"more than {MAX_TOKENS} tokens")
    depth = most = 0
    for t in tokens:
        depth = depth + 1 if (t & 3) == LEAF else depth - (t >> 2) + 1
        most = max(most, depth)
    if most > MAX_DEPTH:
        raise BeyondLimits(f"stack depth above {MAX_DEPTH}")
    if len(sets) > MAX_SET_VALS:
        raise BeyondLimits(f"more than {MAX_SET_VALS} set values")
    return leaves, tokens, sets


def assemble(pieces: Sequence) -> Program:
    """The `lower_filter` results of one call -> its Program: columns numbered in order of first use, set slices made absolute."""
    if not (1 <= len(pieces) <= MAX_FILTERS):
        raise ValueError(f"{len(pieces)} filters in one call, 1..{MAX_FILTERS} are supported")
    keys: Dict[str, int] = {}
    leaves, tokens, sets, leaf_off, token_off = [], [], [], [0], [0]
    for lv, tk, st in pieces:
        for key, want, op, operand, negate, off, ln in lv:
            leaves.append((operand, keys.setdefault(key, len(keys)), want, op, negate, off + len(sets) if ln else 0, ln))
        tokens.extend(tk)
        sets.extend(st)
        leaf_off.append(len(leaves))
        token_off.append(len(tokens))
    if len(sets) > MAX_SET_VALS:
        raise ValueError(f"{len(sets)} set values in one call, at most {MAX_SET_VALS} are supported")
    return Program(list(keys), np.array(leaves, dtype=LEAF_DTYPE), leaf_off, tokens, token_off, sets)


def lower(compiled_filters: Sequence[Tuple], strings_of: Callable[[str], List[str]]) -> Program:
    """Compiled filters (at most 64, each within the limits: BeyondLimits otherwise) -> the Program of one call."""
    return assemble([lower_filter(t, strings_of) for t in compiled_filters])


def validate_program(p: Program, n_cols: int) -> None:
    """What the kernel takes on trust, checked on the host before the upload.  ValueError names the field."""
    nf = p.n_filters
    if not (1 <= nf <= MAX_FILTERS):
        raise ValueError(f"where program: n_filters={nf} out of range 1..{MAX_FILTERS}")
    if n_cols < 1:
        raise ValueError(f"where program: n_cols={n_cols} must be at least 1")
    for name, off, total in (("leaf_off", p.leaf_off, len(p.leaves)), ("token_off", p.token_off, len(p.tokens))):
        if off.shape != (nf + 1,) or off[0] != 0 or off[-1] != total or np.any(np.diff(off) < 0):
            raise ValueError(f"where program: {name}={off.tolist()} must ascend from 0 to {total} in {nf + 1} entries")
    if len(p.set_vals) > MAX_SET_VALS:
        raise ValueError(f"where program: n_set_vals={len(p.set_vals)} above {MAX_SET_VALS}")
    for i, L in enumerate(p.leaves):
        if not (0 <= L["column"] < n_cols):
            raise ValueError(f"where program: leaves[{i}].column={L['column']} outside [0, {n_cols})")
        if L["want_kind"] not in (_NUM, _STR, _BOOL):
            raise ValueError(f"where program: leaves[{i}].want_kind={L['want_kind']} is not 1, 2 or 3")
        if not (EQ <= L["op"] <= NEVER):
            raise ValueError(f"where program: leaves[{i}].op={L['op']} outside {EQ}..{NEVER}")
        if L["negate"] not in (0, 1):
            raise ValueError(f"where program: leaves[{i}].negate={L['negate']} is not 0 or 1")
        if L["op"] == IN:
            a, n = int(L["set_off"]), int(L["set_len"])
            if not (n >= 1 and 0 <= a and a + n <= len(p.set_vals)):
                raise ValueError(f"where program: leaves[{i}] set slice [{a}, {a + n}) outside the {len(p.set_vals)} set values")
            s = p.set_vals[a:a + n]
            if np.isnan(s).any() or np.any(np.diff(s) <= 0):
                raise ValueError(f"where program: leaves[{i}] set values must ascend strictly and hold no NaN")
    for f in range(nf):
        n_leaf, depth = int(p.leaf_off[f + 1] - p.leaf_off[f]), 0
        toks = p.tokens[p.token_off[f]:p.token_off[f + 1]]
        if not (1 <= n_leaf <= MAX_LEAVES and 1 <= len(toks) <= MAX_TOKENS):
            raise ValueError(f"where program: filter {f} has {n_leaf} leaves and {len(toks)} tokens, 1..{MAX_LEAVES} and 1..{MAX_TOKENS} are supported")
        for j, t in enumerate(toks.tolist()):
            code, arg = t & 3, t >> 2
            if code == LEAF:
                if not (0 <= arg < n_leaf):
                    raise ValueError(f"where program: tokens[{int(p.token_off[f]) + j}] names leaf {arg} of filter {f}, which has {n_leaf}")
                depth += 1
            elif code in (AND, OR):
                if not (1 <= arg <= depth):
                    raise ValueError(f"where program: tokens[{int(p.token_off[f]) + j}] pops {arg} of {depth} stack entries")
                depth -= arg - 1
            else:
                raise ValueError(f"where program: tokens[{int(p.token_off[f]) + j}]={t} has no known code")
            if depth > MAX_DEPTH:
                raise ValueError(f"where program: filter {f} needs stack depth {depth}, at most {MAX_DEPTH}")
        if depth != 1:
            raise ValueError(f"where program: the tokens of filter {f} leave {depth} stack entries, not 1")


def run_program_host(p: Program, columns: Sequence[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
    """bool [n_filters, n]: a numpy interpreter of exactly the arrays the kernel reads (`columns[c]` = (kind uint8 [n], val f64 [n]) of
    `p.keys[c]`).  For the CPU tests of the lowering; the product path never calls it."""
    validate_program(p, len(columns))
    n = int(columns[0][0].shape[0])
    out = np.zeros((p.n_filters, n), dtype=bool)
    for f in range(p.n_filters):
        stack: List[np.ndarray] = []
        base = int(p.leaf_off[f])
        for t in p.tokens[p.token_off[f]:p.token_off[f + 1]].tolist():
            code, arg = t & 3, t >> 2
            if code == LEAF:
                L = p.leaves[base + arg]
                kind, val = columns[int(L["column"])]
                op, x = int(L["op"]), float(L["operand"])
                with np.errstate(invalid="ignore"):
                    if op == EQ:
                        hit = np.equal(val, x)
                    elif op == GT:
                        hit = np.greater(val, x)
                    elif op == GE:
                        hit = np.greater_equal(val, x)
                    elif op == LT:
                        hit = np.less(val, x)
                    elif op == LE:
                        hit = np.less_equal(val, x)
                    elif op == IN:
                        s = p.set_vals[int(L["set_off"]):int(L["set_off"]) + int(L["set_len"])]
                        at = np.minimum(np.searchsorted(s, val, side="left"), len(s) - 1)
                        hit = np.equal(s[at], val)
                    else:
                        hit = np.zeros(n, dtype=bool)
                stack.append(np.logical_xor(np.logical_and(kind == L["want_kind"], hit), bool(L["negate"])))
            else:
                args, stack = stack[len(stack) - arg:], stack[:len(stack) - arg]
                stack.append(np.logical_and.reduce(args) if code == AND else np.logical_or.reduce(args))
        out[f] = stack[0]
    return out


class MetadataColumns:
    """The metadata of this rank's rows [lo, hi) as columns in HBM — 9 bytes per row and key: kind uint8 + val float64 — with the `where`
    evaluation over them.  `device=None`: columns stay numpy (the CPU tests of the lowering; `allow_many` then raises)."""

    def __init__(self, metadata: Sequence[Dict], lo: int = 0, hi: Optional[int] = None, device=None):
        hi = len(metadata) if hi is None else hi
        if not (0 <= lo <= hi <= len(metadata)):
            raise ValueError(f"rows [{lo}, {hi}) outside the metadata's {len(metadata)} rows")
        self.metadata, self.lo, self.hi, self.n_rows = metadata, lo, hi, hi - lo
        self.n_words = (self.n_rows + 63) // 64
        self.device = device
        self._strings: Dict[str, List[str]] = {}
        self._numbers: Dict[str, np.ndarray] = {}
        self._kinds: Dict[str, frozenset] = {}
        self._facets: Dict = {}                                 # `facets.resolve`'s results, by spec
        self._host: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self._dev: Dict[str, Tuple] = {}
        self._host_cache: Dict = {}                             # `where.evaluate`'s columns, for the filters past the limits
        self.paths = {"device": 0, "host": 0}

    # ---- columns ---------------------------------------------------------------------------------------------------------------
    def _build(self, key: str) -> Tuple[np.ndarray, np.ndarray]:
        n = self.n_rows
        vals = [m.get(key) if isinstance(m, dict) else None for m in (self.metadata[r] for r in range(self.lo, self.hi))]
        kind = np.fromiter((_kind(v) for v in vals), dtype=np.uint8, count=n)
        strings = sorted({v for v, k in zip(vals, kind) if k == _STR})
        code = {s: float(i) for i, s in enumerate(strings)}
        val = np.zeros(n, dtype=np.float64)
        for r, (v, k) in enumerate(zip(vals, kind)):
            if k == _NUM:
                val[r] = float(v)
            elif k == _STR:
                val[r] = code[v]
            elif k == _BOOL:
                val[r] = 1.0 if v else 0.0
        self._strings[key] = strings
        self._kinds[key] = frozenset(np.unique(kind).tolist())
        return kind, val

    def strings(self, key: str) -> List[str]:
        """The sorted distinct strings of `key` in [lo, hi): a string's code is its position in this list."""
        if key not in self._strings:
            if self.device is None:
                self.host_column(key)
            else:
                self.device_column(key)
        return self._strings[key]

    def numbers(self, key: str) -> np.ndarray:
        """The sorted distinct non-NaN numbers of `key` in [lo, hi), float64, -0.0 folded into 0.0: the `cuts` of an exact facet
        (`facets.resolve`).  Computed on first use and cached next to `strings(key)`."""
        if key not in self._numbers:
            kind, val = self.host_column(key)
            v = val[(kind == _NUM) & ~np.isnan(val)]
            self._numbers[key] = np.unique(np.where(v == 0.0, 0.0, v))
        return self._numbers[key]

    def kinds(self, key: str) -> frozenset:
        """The kinds (0 absent or another type, 1 number, 2 string, 3 bool) the rows [lo, hi) hold under `key`."""
        self.strings(key)
        return self._kinds[key]

    def drop(self) -> None:
        """Forget every column and what was derived from it (the string and number lists, the host evaluator's cache): the metadata
        changed, everything is rebuilt on its next use."""
        self._strings, self._numbers, self._kinds, self._facets = {}, {}, {}, {}
        self._host, self._dev, self._host_cache = {}, {}, {}

    def host_column(self, key: str) -> Tuple[np.ndarray, np.ndarray]:
        """(kind uint8 [n], val float64 [n]) as numpy."""
        if key not in self._host:
            if key in self._dev:
                return tuple(t.cpu().numpy() for t in self._dev[key])
            self._host[key] = self._build(key)
        return self._host[key]

    def device_column(self, key: str) -> Tuple:
        """(kind uint8 [n], val float64 [n]) as device tensors, built and uploaded on first use."""
        import torch
        if key not in self._dev:
            kind, val = self._host.pop(key, None) or self._build(key)
            self._dev[key] = (torch.from_numpy(kind).to(self.device), torch.from_numpy(val).to(self.device))
        return self._dev[key]

    def column_bytes(self, keys) -> int:
        """HBM bytes of the columns of `keys`: what one evaluation reads at least."""
        return BYTES_PER_ROW_AND_KEY * self.n_rows * len(set(keys))

    # ---- lowering --------------------------------------------------------------------------------------------------------------
    def lower(self, compiled_filters: Sequence[Tuple]) -> Program:
        return lower(compiled_filters, self.strings)

    def plan(self, compiled_filters: Sequence[Tuple]):
        """-> (pieces, calls, host): `pieces[i]` is filter i lowered or None where it is past a limit; `calls` lists the filter indices of
        every `arx_where_eval` call (at most 64 filters and 2^20 set values each); `host` the indices left to the host path."""
        pieces, calls, host, cur, cur_sets = [], [], [], [], 0
        for i, tree in enumerate(compiled_filters):
            try:
                piece = lower_filter(tree, self.strings)
            except BeyondLimits:
                piece = None
                host.append(i)
            pieces.append(piece)
            if piece is None:
                continue
            if cur and (len(cur) == MAX_FILTERS or cur_sets + len(piece[2]) > MAX_SET_VALS):
                calls.append(cur)
                cur, cur_sets = [], 0
            cur.append(i)
            cur_sets += len(piece[2])
        if cur:
            calls.append(cur)
        return pieces, calls, host

    def _host_mask(self, tree: Tuple) -> np.ndarray:
        from .where import evaluate
        return evaluate(tree, self.metadata, self.lo, self.hi, cache=self._host_cache)

    def allow_many_host(self, compiled_filters: Sequence[Tuple]) -> np.ndarray:
        """bool [F, n]: `allow_many` with `run_program_host` in the kernel's place, same planning, same `paths`.  For the CPU tests."""
        pieces, calls, host = self.plan(compiled_filters)
        out = np.zeros((len(compiled_filters), self.n_rows), dtype=bool)
        for call in calls:
            prog = assemble([pieces[i] for i in call])
            out[call] = run_program_host(prog, [self.host_column(k) for k in prog.keys])
        for i in host:
            out[i] = self._host_mask(compiled_filters[i])
        self.paths = {"device": sum(len(c) for c in calls), "host": len(host)}
        return out

    # ---- the device path -------------------------------------------------------------------------------------------------------
    def run_program(self, prog: Program, out, counts, and_with=None, and_stride: int = 0):
        """One `arx_where_eval` on the current stream: `prog` validated, packed into one host buffer and uploaded in one copy; `out` int64
        [n_filters, n_words] and `counts` int64 [n_filters] on the device are written.  No synchronisation beyond that upload."""
        import torch
        from . import _lib
        lib = _lib.load()
        validate_program(prog, len(prog.keys))
        nf = prog.n_filters
        assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (nf, self.n_words)
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and tuple(counts.shape) == (nf,)
        cols = [self.device_column(k) for k in prog.keys]
        table = np.array([[kd.data_ptr(), vd.data_ptr()] for kd, vd in cols], dtype=np.int64)
        sets = prog.set_vals if len(prog.set_vals) else np.zeros(1, dtype=np.float64)      # (a valid pointer for a call without sets)
        parts, at, offs = (table, sets, prog.leaves, prog.leaf_off, prog.tokens, prog.token_off), 0, []
        for a in parts:
            offs.append(at)
            at += (a.nbytes + 7) // 8 * 8
        buf = np.zeros(at, dtype=np.uint8)
        for a, o in zip(parts, offs):
            buf[o:o + a.nbytes] = np.frombuffer(a.tobytes(), dtype=np.uint8)
        with torch.cuda.device(self.device):
            blob = torch.from_numpy(buf).to(self.device)
            base = blob.data_ptr()
            rc = lib.arx_where_eval(base + offs[0], len(cols), self.n_rows, base + offs[2], base + offs[3], base + offs[4], base + offs[5],
                                    base + offs[1], len(prog.set_vals), nf, None if and_with is None else and_with.data_ptr(), and_stride,
                                    out.data_ptr(), counts.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "arx_where_eval")

    def allow_many(self, compiled_filters: Sequence[Tuple], and_with=None):
        """-> (int64 [F, ceil(n / 64)] on the device, list of F counts): bit r & 63 of word [f, r >> 6] <=> row lo + r satisfies filter f;
        bits at or beyond n are 0; the layout `ShardIndex.search_filtered_many` takes.  `and_with`: None, one device bitmap int64
        [ceil(n / 64)] and-ed into every filter's, or one per filter int64 [F, ceil(n / 64)] (the dedup keep-bitmap, a folded
        `where_document` bitmap); the counts are those of the and-ed bitmaps.  One `arx_where_eval` per 64 filters, one device-to-host
        read (the counts) per call of this method.  `paths` then says how many filters the kernel took and how many, past the limits,
        the host path."""
        import torch
        from . import _lib
        if self.device is None:
            raise ValueError("MetadataColumns was built without a device: allow_many needs one (there is no host fallback)")
        nf, nw, dev = len(compiled_filters), self.n_words, self.device
        out = torch.empty((nf, nw), dtype=torch.int64, device=dev)
        if and_with is not None:
            if not (torch.is_tensor(and_with) and and_with.is_cuda and and_with.dtype == torch.int64 and and_with.is_contiguous()
                    and tuple(and_with.shape) in ((nw,), (nf, nw))):
                raise ValueError(f"and_with must be a contiguous int64 device tensor [{nw}] or [{nf}, {nw}]")
        if nf == 0 or self.n_rows == 0:
            self.paths = {"device": 0, "host": 0}
            return out, [0] * nf
        pieces, calls, host = self.plan(compiled_filters)
        per_filter = and_with is not None and and_with.dim() == 2
        counts = torch.empty(nf, dtype=torch.int64, device=dev)
        straight = not host                                      # the calls' filters are consecutive rows of `out`
        for call in calls:
            prog = assemble([pieces[i] for i in call])
            if straight:
                o, c = out[call[0]:call[0] + len(call)], counts[call[0]:call[0] + len(call)]
                aw = and_with[call[0]:call[0] + len(call)] if per_filter else and_with
            else:
                o, c = torch.empty((len(call), nw), dtype=torch.int64, device=dev), torch.empty(len(call), dtype=torch.int64, device=dev)
                aw = and_with[torch.tensor(call, device=dev)].contiguous() if per_filter else and_with
            self.run_program(prog, o, c, aw, nw if per_filter else 0)
            if not straight:
                at = torch.tensor(call, device=dev)
                out[at], counts[at] = o, c
        if host:
            from .where import pack_bitmap
            lib = _lib.load()
            with torch.cuda.device(dev):
                for i in host:
                    words = torch.from_numpy(pack_bitmap(self._host_mask(compiled_filters[i])).view(np.int64)).to(dev)
                    if and_with is not None:
                        words &= and_with[i] if per_filter else and_with
                    out[i] = words
                    _lib.check(lib.arx_bitmap_count(out[i].data_ptr(), self.n_rows, counts[i:i + 1].data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream), "arx_bitmap_count")
        self.paths = {"device": nf - len(host), "host": len(host)}
        return out, counts.cpu().tolist()
