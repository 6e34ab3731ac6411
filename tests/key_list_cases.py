"""The bookkeeping of one LDS key list of a candidate scan block (csrc/key_lists.h; binary.hip and pq.hip), restated for the tests of
both scans: which rounds a list is cut before, and how many keys a non-zero threshold turns away.  A key is
high word << 32 | (0xffffffff - row): larger is better, distinct for distinct rows.  Host arithmetic only.

KEY_NT (rows of a round), KEY_CAP (slots of a list), KEY_QBATCH (queries of a slice) and KEY_SLOTS_MAX (partial lists of the workspace)
are read out of the header: if one changes, the tests that derive their shapes from them fail instead of silently covering less."""
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parents[1] / "arxiv_rag_amd" / "csrc"


def constexpr(source, name):
    """The value of `constexpr <type> ... NAME = <integer expression>` in csrc/<source>: integers, `ll` suffixes, * + - << and names
    already known from key_lists.h."""
    m = re.search(rf"\bconstexpr\b[^;]*?\b{name}\s*=\s*([^;,]+)[;,]", (CSRC / source).read_text())
    assert m, f"{source} no longer defines constexpr {name}"
    expr = re.sub(r"\b(\d+)(?:ll|LL|u|U)\b", r"\1", m.group(1).strip())
    assert re.fullmatch(r"[\w\s*+\-<>()/]+", expr), (name, expr)
    known = {k: v for k, v in globals().items() if k.startswith("KEY_") and isinstance(v, int)}
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, known))


KEY_NT = constexpr("key_lists.h", "KEY_NT")
KEY_CAP = constexpr("key_lists.h", "KEY_CAP")
KEY_R_MAX = constexpr("key_lists.h", "KEY_R_MAX")
KEY_QBATCH = constexpr("key_lists.h", "KEY_QBATCH")
KEY_SLOTS_MAX = constexpr("key_lists.h", "KEY_SLOTS_MAX")


def binary_keys(d):
    """int64 keys of Hamming distances d[row] (binary.hip): (0x7fffffff - d) << 32 | (0xffffffff - row)"""
    d = np.asarray(d)
    return ((0x7fffffff - d.astype(np.int64)) << 32) | (0xffffffff - np.arange(d.shape[0], dtype=np.int64))


def pq_keys(s):
    """int64 keys of table sums s[row] (pq.hip): s << 32 | (0xffffffff - row)"""
    s = np.asarray(s)
    return (s.astype(np.int64) << 32) | (0xffffffff - np.arange(s.shape[0], dtype=np.int64))


def schedule(keys, visible, lo, hi, R):
    """One query's list in the block of rows [lo, hi): -> (rounds before which it was cut, keys turned away by a non-zero threshold).
    `keys[row]`: larger is better.  The list is cut to its R best before a round when count + KEY_NT > KEY_CAP; a list that has held R
    keys at a cut has its R-th best as threshold from then on, and only keys above it are appended."""
    held, thr, cuts, turned = np.zeros(0, np.int64), None, [], 0
    for r, a in enumerate(range(lo, hi, KEY_NT)):
        if held.shape[0] + KEY_NT > KEY_CAP:
            held = np.sort(held)[::-1][:R]
            thr = held[R - 1] if held.shape[0] >= R else None
            cuts.append(r)
        rows = np.arange(a, min(a + KEY_NT, hi))
        k = keys[rows[visible[rows]]]
        if thr is not None:
            turned += int((k <= thr).sum())
            k = k[k > thr]
        held = np.concatenate([held, k])
        assert held.shape[0] <= KEY_CAP
    return cuts, turned


def schedule_distances(d, visible, lo, hi, R):
    """`schedule` for the binary scan: keys order as (distance asc, row asc)"""
    return schedule(binary_keys(d), visible, lo, hi, R)


def key_slots(n_rows, n_queries):
    """key_layout's `slots`: the (part, query) lists the workspace of a call holds"""
    qb = min(n_queries, KEY_QBATCH)
    parts = max((n_rows + 63) // 64, 1)
    return max(min(parts * qb, KEY_SLOTS_MAX), qb)


def rows_per_block(n_rows, n_queries, tile, rpb=0, blocks_target=1024, rpb_min_default=2048):
    """Per slice of a call: (queries, rows_per_block as the host picks or raises it, parts).  `tile`: queries of a scan tile; `rpb`: the
    caller's rows_per_block, 0 = default (arx_binary_candidates_tuned and arx_pq_candidates_tuned hold the same arithmetic)."""
    up = lambda v, m: (v + m - 1) // m * m
    slots, out = key_slots(n_rows, n_queries), []
    for q0 in range(0, n_queries, KEY_QBATCH):
        nq = min(n_queries - q0, KEY_QBATCH)
        tiles = (nq + tile - 1) // tile
        b = rpb
        if b == 0:
            want = max(blocks_target // tiles, 1)
            b = max(up((n_rows + want - 1) // want, 256), rpb_min_default)
        max_parts = slots // nq
        if (n_rows + b - 1) // b > max_parts:
            b = up((n_rows + max_parts - 1) // max_parts, 64)
        out.append((nq, b, (n_rows + b - 1) // b))
    return out
