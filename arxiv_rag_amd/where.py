"""Chroma `where` filters over the chunk metadata, evaluated column-wise on the host and packed into the row bitmap the filtered
search takes (`arx_topk_search_filtered`, include/arx.h).

    compiled = compile_where({"$and": [{"section": "abstract"}, {"quality_score": {"$gte": 0.95}}]})
    mask = evaluate(compiled, metadata, lo, hi)          # bool [hi - lo]
    words = pack_bitmap(mask)                            # uint64 [ceil((hi - lo) / 64)], bit r & 63 of word r >> 6 = row r

Operators: implicit `$eq` (`{"section": "abstract"}`), `$eq $ne $gt $gte $lt $lte $in $nin`, `$and` / `$or` with nesting; several keys in
one dict are and-ed.  Strings compare with strings and numbers with numbers (bool is its own type, as in Chroma); a row that lacks the
key, or holds a value of the other type, fails every operator except `$ne` / `$nin`.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

_CMP = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte")
_SET = ("$in", "$nin")
_NUM, _STR, _BOOL = 1, 2, 3


def _kind(v) -> int:
    if isinstance(v, (bool, np.bool_)):
        return _BOOL
    if isinstance(v, (int, float, np.integer, np.floating)):
        return _NUM
    if isinstance(v, str):
        return _STR
    return 0


def _scalar(v, where: str):
    if not _kind(v):
        raise ValueError(f"where: operand of {where} must be a string, a number or a bool, got {v!r}")
    return v


def _compile_field(key: str, cond) -> Tuple:
    if not isinstance(key, str) or not key or key.startswith("$"):
        raise ValueError(f"where: unknown operator {key!r}")
    if not isinstance(cond, dict):
        return ("cmp", key, "$eq", _scalar(cond, f"{key!r}"))
    if not cond:
        raise ValueError(f"where: empty condition for {key!r}")
    parts = []
    for op, val in cond.items():
        if op in _CMP:
            val = _scalar(val, f"{key!r}: {op}")
            if op not in ("$eq", "$ne") and _kind(val) == _BOOL:
                raise ValueError(f"where: {op} of {key!r} needs a number or a string, got {val!r}")
            parts.append(("cmp", key, op, val))
        elif op in _SET:
            if not isinstance(val, (list, tuple)) or not val:
                raise ValueError(f"where: {op} of {key!r} needs a non-empty list, got {val!r}")
            vals = [_scalar(v, f"{key!r}: {op}") for v in val]
            if len({_kind(v) for v in vals}) != 1:
                raise ValueError(f"where: the values of {op} of {key!r} must share one type, got {val!r}")
            parts.append(("set", key, op, tuple(vals)))
        else:
            raise ValueError(f"where: unknown operator {op!r} for {key!r}")
    return parts[0] if len(parts) == 1 else ("and", tuple(parts))


def compile_where(where: Dict) -> Tuple:
    """Validate a Chroma filter and return its tree: ("and" | "or", children), ("cmp", key, op, value), ("set", key, op, values).
    ValueError names the offending part."""
    if not isinstance(where, dict) or not where:
        raise ValueError(f"where: expected a non-empty dict, got {where!r}")
    parts = []
    for key, val in where.items():
        if key in ("$and", "$or"):
            if not isinstance(val, (list, tuple)) or not val:
                raise ValueError(f"where: {key} needs a non-empty list of filters, got {val!r}")
            parts.append((key[1:], tuple(compile_where(v) for v in val)))
        else:
            parts.append(_compile_field(key, val))
    return parts[0] if len(parts) == 1 else ("and", tuple(parts))


def keys_of(compiled: Tuple) -> set:
    if compiled[0] in ("and", "or"):
        return set().union(*(keys_of(c) for c in compiled[1]))
    return {compiled[1]}


class _Column:
    """One metadata key over all rows: the numbers, the strings and the bools it holds, each with the mask of the rows that hold one."""

    def __init__(self, metadata: Sequence[Dict], key: str):
        n = len(metadata)
        vals = [m.get(key) if isinstance(m, dict) else None for m in metadata]
        kinds = np.fromiter((_kind(v) for v in vals), dtype=np.int8, count=n)
        self.is_num, self.is_str, self.is_bool = kinds == _NUM, kinds == _STR, kinds == _BOOL
        self.num = np.array([float(v) if k == _NUM else 0.0 for v, k in zip(vals, kinds)], dtype=np.float64)
        self.str = np.array([v if k == _STR else "" for v, k in zip(vals, kinds)], dtype=object)
        self.bool = np.array([bool(v) if k == _BOOL else False for v, k in zip(vals, kinds)], dtype=bool)

    def of_kind(self, kind: int, lo: int, hi: int):
        if kind == _NUM:
            return self.is_num[lo:hi], self.num[lo:hi]
        if kind == _STR:
            return self.is_str[lo:hi], self.str[lo:hi]
        return self.is_bool[lo:hi], self.bool[lo:hi]


_CACHE: Dict[Tuple[int, str], Tuple[object, _Column]] = {}


def _column(metadata, key: str, cache) -> _Column:
    cache = _CACHE if cache is None else cache
    ck = (id(metadata), key)
    hit = cache.get(ck)
    if hit is not None and hit[0] is metadata and len(metadata) == len(hit[1].num):
        return hit[1]
    col = _Column(metadata, key)
    cache[ck] = (metadata, col)
    return col


def _eval(node, metadata, lo, hi, cache) -> np.ndarray:
    kind = node[0]
    if kind in ("and", "or"):
        out = _eval(node[1][0], metadata, lo, hi, cache)
        for child in node[1][1:]:
            m = _eval(child, metadata, lo, hi, cache)
            out = (out & m) if kind == "and" else (out | m)
        return out
    _, key, op, val = node
    col = _column(metadata, key, cache)
    if kind == "set":
        has, v = col.of_kind(_kind(val[0]), lo, hi)
        vals = [float(x) for x in val] if _kind(val[0]) == _NUM else list(val)
        hit = np.zeros(hi - lo, dtype=bool)
        for x in vals:
            hit |= (v == x)
        hit &= has
        return hit if op == "$in" else ~hit
    has, v = col.of_kind(_kind(val), lo, hi)
    x = float(val) if _kind(val) == _NUM else val
    if op == "$eq":
        return has & (v == x)
    if op == "$ne":
        return ~(has & (v == x))
    if _kind(val) == _STR:                                   # object arrays: ordered comparison row by row on the rows that hold a string
        out = np.zeros(hi - lo, dtype=bool)
        idx = np.nonzero(has)[0]
        f = {"$gt": lambda a: a > x, "$gte": lambda a: a >= x, "$lt": lambda a: a < x, "$lte": lambda a: a <= x}[op]
        out[idx] = [f(a) for a in v[idx]]
        return out
    with np.errstate(invalid="ignore"):
        r = {"$gt": v > x, "$gte": v >= x, "$lt": v < x, "$lte": v <= x}[op]
    return has & r


def evaluate(compiled: Tuple, metadata: Sequence[Dict], lo: int = 0, hi: int = None, cache: Dict = None) -> np.ndarray:
    """bool [hi - lo]: which of the rows [lo, hi) of `metadata` (a sequence of dicts) satisfy the compiled filter.  One numpy column per
    referenced key is built over the whole sequence on first use and cached (by the identity of `metadata`; `cache`: the caller's own
    dict instead of the module's)."""
    hi = len(metadata) if hi is None else hi
    if not (0 <= lo <= hi <= len(metadata)):
        raise ValueError(f"rows [{lo}, {hi}) outside the metadata's {len(metadata)} rows")
    return np.asarray(_eval(compiled, metadata, lo, hi, cache), dtype=bool)


def pack_bitmap(mask) -> np.ndarray:
    """bool [n] -> uint64 [ceil(n / 64)]: bit (r & 63) of word (r >> 6) = mask[r]; the last word's unused bits are zero."""
    mask = np.asarray(mask, dtype=bool).ravel()
    n = mask.shape[0]
    padded = np.zeros((n + 63) // 64 * 64, dtype=bool)
    padded[:n] = mask
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64, copy=False)
