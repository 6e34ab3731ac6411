"""The IVF probe search (csrc/ivf.hip: `arx_ivf_search[_tuned]`, `arx_ivf_search_multi[_tuned]`) where tests/test_gpu_ivf.py and
tests/test_gpu_ivf_multi.py stop: the capped workspace and the forced raise of rows_per_block (1 024 queries over 10 000 members), 128
probes over 4 096 lists with plateaus in the cumulative lengths and damaged `start` at hundreds of places, lists cut by max_list_rows,
idx_base != 0, no members at all, `order` that is no permutation of the rows (the layout of the binary and PQ rescore among them), NULL
count outputs, dims 1536 / 4096, and a shard of 2^20 + 197 rows held to float64.

Sections 1, 2, 3 and 5 compare bit for bit with the numpy restatement (`ivf.search_host` / `search_many_host`, now with
`max_list_rows`), with the filtered search over the probe bitmaps and with calls of other shapes.  Section 4 compares with float64
(tests/helpers.py: scores_fp64, pass_b_budget) the way tests/test_gpu_range_grouped_large.py does: float64 decides the row at a position
when the gaps to both neighbours exceed 2 B(D) |q| max|c|; there the id must be equal, every returned score lies within B |q| |c| of
float64, every position that holds a planted visible row must be decided (a fixture error otherwise, never a skip), the thresholds lie
clear of every visible score by more than the budget, so `hits` is exact from float64.

Every input is drawn by numpy, so the CPU tests of section 0 see the very data the GPU tests search and assert every precondition -
which branch of `ivf_layout` / `ivf_run` a case lands on, from the constants of the sources, and the fixtures of section 4 from float64 -
without a GPU.

Figures printed (profiles/ivf_large.md): the launch shape of every capped case, and the worst score error over its budget per case of
section 4."""
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.where import pack_bitmap
from tests.helpers import pass_b_budget, scores_fp64
from tests.test_gpu_masked_search_large import CSRC, DIM, LINE, N_A, _define, hip  # noqa: F401  (`hip`: the module's fixture)

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
DEV = "cuda:0"
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
INF = float("inf")
BASE = 1 << 33


# ---- the constants the shapes below are derived from, read from the sources: if one changes, the CPU tests below fail ---------------------
def _constant(name):
    """`constexpr int / int64_t NAME = <digits>[ll][ << <digits>]` of csrc/ivf.hip"""
    m = re.search(rf"\bconstexpr\s+(?:int64_t|int)\s[^;]*?\b{name}\s*=\s*(\d+)(?:ll)?(?:\s*<<\s*(\d+))?\s*[,;]", (CSRC / "ivf.hip").read_text())
    assert m, f"ivf.hip no longer defines {name}"
    return int(m.group(1)) << int(m.group(2) or 0)


SLOTS_MAX = _constant("IVF_SLOTS_MAX")
PROBE_MAX = _constant("IVF_PROBE_MAX")
LISTS_MAX = _constant("IVF_LISTS_MAX")
RPB_DEFAULT = _constant("IVF_RPB_DEFAULT")
RPB_WIDE = _constant("IVF_RPB_WIDE")
BLOCKS_ENOUGH = _constant("IVF_BLOCKS_ENOUGH")
RPB_LIMIT = _constant("IVF_RPB_LIMIT")
QBATCH = _define("search_consts.h", "QBATCH_MAX")
KMAX = _define("search_consts.h", "KMAX")


def _cdiv(a, b):
    return -(-a // b)


def _slots(n_members, n_queries):
    """ivf_layout: the (part, query) partial lists the workspace of a call holds"""
    qb = min(n_queries, QBATCH)
    return max(min(max(_cdiv(n_members, 64), 1) * qb, SLOTS_MAX), qb)


def _cap_binds(n_members, n_queries):
    return max(_cdiv(n_members, 64), 1) * min(n_queries, QBATCH) > SLOTS_MAX


def _launches(n_members, n_queries, n_probe, max_list_rows, rows_per_block=None):
    """ivf_run: per internal batch (queries, the rows_per_block asked for or chosen by default, the rows_per_block used)"""
    slots, P = _slots(n_members, n_queries), min(n_probe * max_list_rows, n_members)
    out = []
    for q0 in range(0, n_queries, QBATCH):
        nq = min(n_queries - q0, QBATCH)
        rpb = rows_per_block
        if rpb is None:
            rpb = RPB_DEFAULT
            while rpb < RPB_WIDE and _cdiv(P, rpb) * nq > BLOCKS_ENOUGH:
                rpb *= 2
        asked, max_parts = rpb, slots // nq
        if _cdiv(P, rpb) > max_parts:
            rpb = _cdiv(_cdiv(P, max_parts), 64) * 64
        assert max(_cdiv(P, rpb), 1) <= max_parts
        out.append((nq, asked, rpb))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def same(got, want):
    """(scores, ids[, scanned[, hits]]) device or numpy tuples equal bit for bit."""
    got, want = [_np(g) for g in got], [_np(w) for w in want]
    return len(got) == len(want) and np.array_equal(bits(got[0]), bits(want[0])) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def words_of(masks, garbage=False):
    """bool [F, n] -> int64 [F, ceil(n / 64)]; `garbage`: the last word's bits beyond n are SET"""
    w = np.stack([pack_bitmap(m) for m in masks])
    n = masks.shape[1]
    if garbage and n % 64:
        w[:, -1] |= ~np.uint64(0) << np.uint64(n % 64)
    return w.view(np.int64)


def _based(want, base):
    """a host answer (idx_base = 0) as the library returns it with idx_base = base"""
    return (want[0], np.where(want[1] >= 0, want[1] + base, -1)) + tuple(want[2:])


def _tiled(want, idx):
    return tuple(a[idx] for a in want)


# ---- 1. the shard of the capped workspace: 10 000 rows in 12 lists on wave edges, one of 6 000 ---------------------------------------------------
CAP_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 300, 1000, 2123, 6000)
CAP_N, CAP_LONG, CAP_PAIRS, CAP_NPROBE, CAP_NF = sum(CAP_SIZES), 11, 70, 3, 4
CAP_KS = (10, 32)
CAP_BAD_FILTER = {7: -1, 33: CAP_NF, 50: INT32_MAX, 61: INT32_MIN}              # pair -> its filter_of outside [0, n_filters)
CUTS = (0, 1, 63, 64, 65, 1000)
CUT_KS = (1, 31, 32)
# (queries, rows_per_block): every launch of section 1
CAP_LAUNCHES = [(1024, None), (1025, None), (1024, 64), (1024, 128), (1025, 64), (64, 64)]


@functools.lru_cache(maxsize=None)
def _cap():
    """The shard, 70 distinct (query, probes) pairs, 4 filters with a filter index and a threshold per pair; numpy alone."""
    rng = np.random.default_rng(2101)
    X = (rng.standard_normal((CAP_N, DIM), dtype=np.float32) / 8).astype(np.float16)
    labels = rng.permutation(np.repeat(np.arange(len(CAP_SIZES)), CAP_SIZES)).astype(np.int32)
    order, start, sizes = T.members_host(labels, len(CAP_SIZES))
    Q = (rng.standard_normal((CAP_PAIRS, DIM), dtype=np.float32) / 8).astype(np.float16)
    probes = rng.integers(0, len(CAP_SIZES), (CAP_PAIRS, CAP_NPROBE)).astype(np.int32)
    for j in range(0, CAP_PAIRS, 3):                               # every third pair probes the long list, at each of the three places
        probes[j, (j // 3) % CAP_NPROBE] = CAP_LONG
    masks = np.stack([np.ones(CAP_N, bool), rng.random(CAP_N) < 0.5, rng.random(CAP_N) < 0.05, np.zeros(CAP_N, bool)])
    fo = rng.integers(0, CAP_NF, CAP_PAIRS).astype(np.int32)
    fo[0] = 0
    for j, f in CAP_BAD_FILTER.items():
        fo[j] = f
    w = SimpleNamespace(X=X, labels=labels, order=order, start=start, sizes=sizes, Q=Q, probes=probes, masks=masks, fo=fo, mlr=int(sizes.max()))
    # thresholds: per pair -inf, 0, its own 5th best visible score (a tie at the threshold is kept), +inf, NaN, 0.0625 in turn
    s5 = I.search_many_host(X, order, start, probes, Q, 5, allows=masks, filter_of=fo)[0][:, 4]
    kinds = np.stack([np.full(CAP_PAIRS, -INF), np.zeros(CAP_PAIRS), np.where(np.isfinite(s5), s5, 0.03125), np.full(CAP_PAIRS, INF),
                      np.full(CAP_PAIRS, np.nan), np.full(CAP_PAIRS, 0.0625)]).astype(np.float32)
    w.thr = kinds[np.arange(CAP_PAIRS) % 6, np.arange(CAP_PAIRS)]
    return w


@functools.lru_cache(maxsize=None)
def _cap_host(k, cut=None):
    """-> (`search_host`, `search_many_host` without filters, `search_many_host` under the filters and thresholds) of the 70 pairs"""
    w = _cap()
    plain = I.search_many_host(w.X, w.order, w.start, w.probes, w.Q, k, max_list_rows=cut)
    multi = I.search_many_host(w.X, w.order, w.start, w.probes, w.Q, k, allows=w.masks, filter_of=w.fo, min_score=w.thr, max_list_rows=cut)
    return plain[:3], plain, multi


# ---- 2. the shard of 4 096 lists ------------------------------------------------------------------------------------------------------------------------------
WIDE_LONG, WIDE_LONG_ROWS, WIDE_NQ = 1777, 3000, 14
WIDTHS = (128, 127, 65, 33)
WIDE_KS = (10, 32)


def _edges(w):
    """the places of a probe row that hold its non-empty lists in the edge rows: the binary search's first steps land on them"""
    return sorted({0, 63, 64, w - 1} if w > 64 else {0, w - 2, w - 1})


@functools.lru_cache(maxsize=None)
def _wide():
    rng = np.random.default_rng(2202)
    sizes = rng.integers(0, 13, LISTS_MAX)
    sizes[rng.random(LISTS_MAX) < 0.3] = 0
    sizes[0], sizes[LISTS_MAX - 1], sizes[WIDE_LONG] = 5, 7, WIDE_LONG_ROWS
    n = int(sizes.sum())
    labels = rng.permutation(np.repeat(np.arange(LISTS_MAX), sizes)).astype(np.int32)
    order, start, sizes2 = T.members_host(labels, LISTS_MAX)
    assert np.array_equal(sizes, sizes2)
    X = (rng.standard_normal((n, DIM), dtype=np.float32) / 8).astype(np.float16)
    Q = (rng.standard_normal((WIDE_NQ, DIM), dtype=np.float32) / 8).astype(np.float16)
    # `start` damaged at 300 places and at 0, 1, 1024, 4000, 4095, 4096: negative, decreasing, ahead of its successors, beyond n_members
    bad = start.copy()
    places = np.sort(rng.choice(np.setdiff1d(np.arange(2, 3990), [1024]), 300, replace=False))
    for j, p in enumerate(places.tolist()):
        bad[p] = (-1 - j, start[max(p - 40, 0)], start[p + 9])[j % 3]
    bad[0], bad[1], bad[1024], bad[4000], bad[LISTS_MAX - 1], bad[LISTS_MAX] = -7, -2, start[1000], n + 5, n + 1000, 1 << 40
    return SimpleNamespace(X=X, Q=Q, n=n, sizes=sizes, order=order, start=start, bad_start=bad, damaged=places.shape[0] + 6,
                           mlr=int(sizes.max()), bad_mlr=int(np.diff(T.clamp_starts(bad, n)).max()))


@functools.lru_cache(maxsize=None)
def _wide_probes(w):
    """int32 [14, w], each row built on purpose: 0 all distinct; 1 - 3 all distinct with the long list first, in the middle, last; 4 - 6
    non-empty lists at `_edges(w)` alone, between them empty, invalid and repeated entries (4), empty and repeated lists (5), invalid
    entries (6); 7 - 9 w copies of a short, the long, an empty list; 10 nothing valid; 11 list 4095 first and list 0 last; 12 non-empty
    lists alone; 13 nine lists over and over."""
    sh = _wide()
    rng = np.random.default_rng(2300 + w)
    small = np.setdiff1d(np.nonzero(sh.sizes > 0)[0], [0, LISTS_MAX - 1, WIDE_LONG])
    empty = np.nonzero(sh.sizes == 0)[0]
    others = np.setdiff1d(np.arange(LISTS_MAX), [WIDE_LONG])
    rows = np.zeros((WIDE_NQ, w), np.int64)
    rows[0] = rng.choice(LISTS_MAX, w, replace=False)                                   # all distinct
    for r, place in ((1, 0), (2, w // 2), (3, w - 1)):                                 # all distinct, the long list first / in the middle / last
        rows[r] = rng.choice(others, w, replace=False)
        rows[r, place] = WIDE_LONG
    ed = _edges(w)
    junk = (-1, LISTS_MAX, INT32_MAX, INT32_MIN)
    for r, at_edges in ((4, [0, LISTS_MAX - 1] + small[:2].tolist()), (5, [int(small[2]), WIDE_LONG] + small[3:5].tolist()),
                        (6, [LISTS_MAX - 1, 0, WIDE_LONG] + small[5:6].tolist())):
        vals = dict(zip(ed, at_edges))
        for p in range(w):
            if p in vals:
                rows[r, p] = vals[p]
            elif r == 4:                                           # empty lists, invalid entries and repeats of the first list in turn
                rows[r, p] = (empty[p], junk[(p // 4) % 4], vals[0], empty[p % 7])[p % 4]
            elif r == 5:                                           # plateaus of empty and repeated lists alone
                rows[r, p] = (empty[p], max(v for q, v in vals.items() if q < p), empty[3])[p % 3]
            else:                                                  # invalid entries alone
                rows[r, p] = junk[p % 4]
    rows[7], rows[8], rows[9] = LISTS_MAX - 1, WIDE_LONG, empty[0]                      # w copies of one list: short, long, empty
    rows[10] = np.resize(junk, w)                                                       # nothing valid
    rows[11] = rng.choice(small, w, replace=False)
    rows[11, 0], rows[11, w - 1] = LISTS_MAX - 1, 0                                     # the last list first, the first list last
    rows[12] = rng.choice(small, w, replace=False)                                      # non-empty lists alone
    rows[13] = np.resize(np.concatenate([rng.choice(small, 5, replace=False), empty[:3], [WIDE_LONG]]), w)      # nine lists over and over
    return rows.astype(np.int32)


def _narrowed(row):
    """a probe row narrowed to its distinct valid entries, in order (one invalid entry where none is left)"""
    keep = list(dict.fromkeys(c for c in row.tolist() if 0 <= c < LISTS_MAX))
    return np.array([keep or [-1]], np.int32)


@functools.lru_cache(maxsize=None)
def _wide_host(w, k, damaged):
    sh = _wide()
    return I.search_host(sh.X, sh.order, sh.bad_start if damaged else sh.start, _wide_probes(w), sh.Q, k)


# ---- 3. lists that are no permutation of the rows -----------------------------------------------------------------------------------------------------------
RESCORE_NQ, RESCORE_R = 1024, 256


@functools.lru_cache(maxsize=None)
def _subset():
    """The section-1 shard with about half of its rows in no list: `order` is shorter than n_rows."""
    w = _cap()
    rng = np.random.default_rng(2303)
    rows = np.nonzero(rng.random(CAP_N) < 0.5)[0]
    order = rows[np.argsort(w.labels[rows], kind="stable")].astype(np.int32)
    sizes = np.bincount(w.labels[rows], minlength=len(CAP_SIZES))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return SimpleNamespace(order=order, start=start, mlr=int(sizes.max()),
                           want=I.search_many_host(w.X, order, start, w.probes, w.Q, 10, allows=w.masks, filter_of=w.fo, min_score=w.thr))


@functools.lru_cache(maxsize=None)
def _rescore():
    """The binary / PQ rescore's layout over the section-1 shard: one list of R = 256 places per query, the query's candidates (distinct rows)
    with -1 holes: none, one, R - 1 or R candidates or a random number; trailing holes (as the candidate kernels pad) or scattered ones."""
    w = _cap()
    rng = np.random.default_rng(2304)
    nq, R = RESCORE_NQ, RESCORE_R
    Q = (rng.standard_normal((nq, DIM), dtype=np.float32) / 8).astype(np.float16)
    order = np.full((nq, R), -1, np.int32)
    counts = np.where(np.arange(nq) % 8 < 4, np.array([0, 1, R - 1, R])[np.arange(nq) % 4], rng.integers(2, R - 1, nq))
    for q in range(nq):
        cand = rng.choice(CAP_N, int(counts[q]), replace=False)
        places = np.arange(counts[q]) if q % 2 else np.sort(rng.choice(R, int(counts[q]), replace=False))
        order[q, places] = cand
    start = (np.arange(nq + 1) * R).astype(np.int64)
    probes = np.arange(nq, dtype=np.int32)[:, None]
    return SimpleNamespace(Q=Q, order=order.ravel(), start=start, probes=probes, counts=counts,
                           want={k: I.search_host(w.X, order.ravel(), start, probes, Q, k) for k in (10, 32)})


# ---- 4. the shard of 2^20 + 197 rows, held to float64 -------------------------------------------------------------------------------------------------------
BIG_NQ, BIG_PLANTED, BIG_LISTS, BIG_NPROBE, BIG_K = 8, 40, 40, 8, 32
BIG_SPECIAL = (LINE - 1, LINE, N_A - 1, LINE + 1, LINE - 2, N_A - 2, LINE + 63, LINE - 64)     # rank 0 of query j: the best row of its list
BIG_STATUS = ("vis", "vis", "clr", "clr", "vis", "vis", "unp", "unp")                           # of rank i: BIG_STATUS[i % 8]
BIG_CASES = ("plain", "bitmap", "multi")
BIG_RPBS = (64, None, 1 << 20)
BIG_THR = ("-inf", 5, "low", "nan", 19, "+inf", "low", 12)                                      # of query j


@functools.lru_cache(maxsize=None)
def _big():
    """Unit rows at the masked suite's shard-A size in 40 lists, 8 unit queries probing 8 lists each.  For query j, 40 rows
    a q + sqrt(1 - a^2) noise, a = 0.95 - 0.25 i / 39: rank 0 is BIG_SPECIAL[j], the even ranks lie at or beyond row 2^20, the odd ones
    below; by BIG_STATUS a rank sits in a probed list with its bit set in every filter (vis), in a probed list with its bit cleared in
    the random filters (clr), or in a list the query does not probe (unp).  A chance row scores below 0.125 sqrt(2 ln N) = 0.66."""
    n = N_A
    rng = np.random.default_rng(2404)
    C = rng.standard_normal((n, DIM), dtype=np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    C = C.astype(np.float16)
    Q = rng.standard_normal((BIG_NQ, DIM), dtype=np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float16)
    probes = np.stack([rng.permutation(BIG_LISTS)[:BIG_NPROBE] for _ in range(BIG_NQ)]).astype(np.int32)
    labels = rng.integers(0, BIG_LISTS, n).astype(np.int32)
    above = rng.permutation(np.setdiff1d(np.arange(LINE, n), BIG_SPECIAL)).tolist()
    below = rng.permutation(np.setdiff1d(rng.choice(LINE - 100, 400, replace=False), BIG_SPECIAL)).tolist()
    rows = np.zeros((BIG_NQ, BIG_PLANTED), np.int64)
    for j in range(BIG_NQ):
        unprobed = np.setdiff1d(np.arange(BIG_LISTS), probes[j])
        for i in range(BIG_PLANTED):
            rows[j, i] = BIG_SPECIAL[j] if i == 0 else (above.pop() if i % 2 == 0 else below.pop())
            labels[rows[j, i]] = unprobed[i % unprobed.shape[0]] if BIG_STATUS[i % 8] == "unp" else probes[j, i % BIG_NPROBE]
    assert np.unique(rows).shape[0] == rows.size and rows.max() == n - 1
    a = (0.95 - 0.25 * np.arange(BIG_PLANTED) / (BIG_PLANTED - 1)).astype(np.float32)[None, :, None]
    qh = Q.astype(np.float32)
    qh /= np.linalg.norm(qh, axis=1, keepdims=True)
    noise = rng.standard_normal((BIG_NQ, BIG_PLANTED, DIM), dtype=np.float32)
    noise -= (noise * qh[:, None, :]).sum(2, keepdims=True) * qh[:, None, :]
    noise /= np.linalg.norm(noise, axis=2, keepdims=True)
    C[rows.ravel()] = (a * qh[:, None, :] + np.sqrt(1 - a * a) * noise).astype(np.float16).reshape(-1, DIM)
    status = np.array([BIG_STATUS[i % 8] for i in range(BIG_PLANTED)])
    masks = np.stack([rng.random(n) < 0.5, np.ones(n, bool), rng.random(n) < 0.5])
    for f in (0, 2):
        masks[f][rows[:, status == "vis"].ravel()] = True
        masks[f][rows[:, status == "clr"].ravel()] = False
    order, start, sizes = T.members_host(labels, BIG_LISTS)
    return SimpleNamespace(n=n, C=C, Q=Q, probes=probes, labels=labels, rows=rows, status=status, masks=masks, order=order, start=start,
                           mlr=int(sizes.max()), fo=(np.arange(BIG_NQ) % 3).astype(np.int32))


_BIG_REF = {}


def _big_ref(device):
    """float64 scores of the 8 queries over the whole shard (numpy [8, n]), computed once per device and left unchanged, with the norms
    of the budget: `tol` [8] = 2 B(D) |q| max|c| (and a part in a thousand), `qn` [8], `cn` [n]."""
    if device not in _BIG_REF:
        sh = _big()
        C, Q = torch.from_numpy(sh.C).to(device), torch.from_numpy(sh.Q).to(device)
        e = scores_fp64(Q, C).cpu().numpy()
        qn = np.linalg.norm(sh.Q.astype(np.float64), axis=1)
        cn = np.concatenate([np.linalg.norm(sh.C[a:a + (1 << 18)].astype(np.float64), axis=1) for a in range(0, sh.n, 1 << 18)])
        probe = np.random.default_rng(5).choice(sh.n, 64, replace=False)                 # the device's float64 product against numpy's
        assert np.allclose(e[:, probe], sh.Q.astype(np.float64) @ sh.C[probe].astype(np.float64).T, rtol=0, atol=1e-12)
        _BIG_REF[device] = SimpleNamespace(e=e, qn=qn, cn=cn, tol=2 * pass_b_budget(DIM) * (1 + 1e-3) * qn * cn.max())
    return _BIG_REF[device]


def _big_filter(case, j):
    """the filter query j is under in a case: None or an index into the shard's masks"""
    sh = _big()
    return None if case == "plain" else 0 if case == "bitmap" else int(sh.fo[j])


@functools.lru_cache(maxsize=None)
def _big_expected(case, device):
    """The float64 definition per query: the visible rows (the probed lists' rows under the query's filter) ranked by (float64 score desc,
    row asc), cut at the threshold and at k -> per query a namespace: `n_visible`, `thr` (f32), `hits`, `ids` [k] (-1 padding), `sv` [k]
    (the float64 scores behind them, -inf padding), `decided` [k], `hidden` (the planted rows the query must not return).  Fixture
    errors: a visible score within the budget of the threshold; a planted visible row at a position float64 does not decide."""
    sh, ref = _big(), _big_ref(device)
    out = []
    for j in range(BIG_NQ):
        rows = I._visible_rows(sh.order, sh.start, sh.probes[j], sh.n)
        f = _big_filter(case, j)
        if f is not None:
            rows = rows[sh.masks[f][rows]]
        v = ref.e[j, rows]
        by = np.lexsort((rows, -v))
        sr, sv = rows[by], v[by]
        kind = BIG_THR[j] if case == "multi" else "-inf"
        if kind == "low":                                          # thousands of hits: the widest gap among 100 places from the 3 000th on
            p = 3000 + int(np.argmax(sv[3000:3100] - sv[3001:3101]))
            thr = np.float32((sv[p] + sv[p + 1]) / 2)
        elif isinstance(kind, int):                                # exactly `kind` hits
            thr = np.float32((sv[kind - 1] + sv[kind]) / 2)
        else:
            thr = np.float32(kind)
        with np.errstate(invalid="ignore"):
            qual = sv >= np.float64(thr)                           # (NaN: none)
            assert (qual[1:] <= qual[:-1]).all()
            if np.isfinite(thr):
                assert np.abs(sv - np.float64(thr)).min() > ref.tol[j] / 2, (case, j, "fixture: a visible row within the budget of the threshold")
        hits = int(qual.sum())
        m = min(hits, BIG_K)
        ids = np.full(BIG_K, -1, np.int64); ids[:m] = sr[:m]
        vq = np.full(BIG_K + 1, -INF); vq[:min(hits, BIG_K + 1)] = sv[:min(hits, BIG_K + 1)]
        with np.errstate(invalid="ignore"):
            gap_ok = (vq[:-1] - vq[1:] > ref.tol[j]) | (vq[1:] == -INF)
        decided = np.concatenate([[True], gap_ok[:-1]]) & gap_ok & (ids >= 0)
        planted = np.isin(ids, sh.rows[j])
        assert decided[planted].all(), (case, j, "fixture: float64 does not decide the place of a planted row")
        visible = np.zeros(sh.n, bool); visible[rows] = True
        out.append(SimpleNamespace(n_visible=rows.shape[0], thr=thr, hits=hits, ids=ids, sv=vq[:BIG_K], decided=decided, planted=planted,
                                   visible=visible, hidden=sh.rows[j][~visible[sh.rows[j]]]))
    return out


# ---- 0. CPU only: the shapes cross the lines, by the constants of the sources -------------------------------------------------------------------------------------
def test_the_cases_cross_the_lines_by_the_constants_of_the_sources():
    assert (SLOTS_MAX, PROBE_MAX, LISTS_MAX, RPB_DEFAULT, RPB_WIDE, BLOCKS_ENOUGH, RPB_LIMIT, QBATCH, KMAX) == \
        (1 << 17, 128, 4096, 128, 1024, 2048, 1 << 20, 1024, 32)
    assert (I.MAX_PROBE, I.MAX_LISTS, I.MAX_K) == (PROBE_MAX, LISTS_MAX, KMAX)
    # the existing 1 025-query tests (1 000 rows) never reach the cap; 1 024 queries do from 8 193 members on
    assert not _cap_binds(1000, 1025) and _slots(1000, 1025) == 16 * 1024 and not _cap_binds(8192, 1024) and _cap_binds(8193, 1024)
    # -- section 1 --
    w = _cap()
    assert CAP_N == 10000 and w.sizes.tolist() == list(CAP_SIZES) and w.mlr == 6000 and len(CAP_SIZES) == 12
    P = min(CAP_NPROBE * w.mlr, CAP_N)
    assert P == CAP_N > 8192
    assert len({(w.Q[j].tobytes(), w.probes[j].tobytes()) for j in range(CAP_PAIRS)}) == CAP_PAIRS
    assert sum(CAP_LONG in p for p in w.probes.tolist()) >= 24 and {p.index(CAP_LONG) for p in w.probes.tolist() if CAP_LONG in p} == {0, 1, 2}
    L = {key: _launches(CAP_N, key[0], CAP_NPROBE, w.mlr, key[1]) for key in CAP_LAUNCHES}
    assert all(_cap_binds(CAP_N, nq) == (nq >= 1024) for nq, _ in CAP_LAUNCHES) and _slots(CAP_N, 1024) == SLOTS_MAX and SLOTS_MAX // 1024 == 128
    # the default: rows_per_block grows to IVF_RPB_WIDE for 1 024 queries (10 parts: no raise), and is IVF_RPB_DEFAULT for the query that
    # runs in a batch of its own (79 parts of the 2^17 the workspace then holds for it)
    assert L[(1024, None)] == [(1024, 1024, 1024)] and L[(1025, None)] == [(1024, 1024, 1024), (1, 128, 128)]
    # rows_per_block = 64 is not honoured: 157 parts > 128 -> raised to round_up64(ceil(10000 / 128)) = 128; in the batch of one it is
    assert L[(1024, 64)] == [(1024, 64, 128)] and _cdiv(P, 64) == 157 > 128 and L[(1025, 64)] == [(1024, 64, 128), (1, 64, 64)]
    # rows_per_block = 128 is honoured as asked (79 parts <= 128): the value the raise of 64 lands on.  The raise would take P > 16 384.
    assert L[(1024, 128)] == [(1024, 128, 128)] and _cdiv(P, 128) == 79
    assert L[(64, 64)] == [(64, 64, 64)] and _slots(CAP_N, 64) == 157 * 64 < SLOTS_MAX                     # no cap, no raise
    for cut in CUTS:                                               # section 3's cuts lie below the long list; none is raised
        assert cut < w.mlr and all(a == u for _, a, u in _launches(CAP_N, CAP_PAIRS, CAP_NPROBE, cut))
    # the filters and thresholds bite: queries without a row, hits below scanned, hits above k, every bad filter index
    for k in CAP_KS:
        one, plain, multi = _cap_host(k)
        assert np.array_equal(plain[2], plain[3]) and same(one, plain[:3]) and plain[2].max() > 6000
        assert (multi[3] < multi[2]).any() and (multi[3] > k).any() and all(multi[2][j] == 0 for j in CAP_BAD_FILTER)
        assert (multi[3][np.isnan(w.thr) | (w.thr == INF)] == 0).all() and not np.array_equal(multi[1], plain[1])
    # -- section 2 --
    sh = _wide()
    assert sh.start.shape[0] == LISTS_MAX + 1 == 4097 and 19000 < sh.n < 22000 and sh.sizes.max() == sh.sizes[WIDE_LONG] == WIDE_LONG_ROWS
    assert sh.sizes[0] > 0 and sh.sizes[-1] > 0 and (sh.sizes == 0).sum() > 1000 and np.delete(sh.sizes, WIDE_LONG).max() == 12
    assert max(WIDTHS) == PROBE_MAX and WIDTHS == (128, 127, 65, 33) and _edges(128) == [0, 63, 64, 127] and _edges(33) == [0, 31, 32]
    for wd in WIDTHS:
        pr = _wide_probes(wd)
        assert pr.shape == (WIDE_NQ, wd)
        assert all(a == u for _, a, u in _launches(sh.n, WIDE_NQ, wd, sh.mlr)) and not _cap_binds(sh.n, WIDE_NQ)
        for r in (0, 1, 2, 3):
            assert len(set(pr[r].tolist())) == wd
        assert pr[1, 0] == pr[2, wd // 2] == pr[3, wd - 1] == WIDE_LONG
        for r in (4, 5, 6):                                        # the lengths as ivf_prepare_kernel has them: non-zero at the edges alone
            first = [p for p, c in enumerate(pr[r].tolist()) if 0 <= c < LISTS_MAX and c not in pr[r, :p].tolist()]
            assert [p for p in first if sh.sizes[pr[r, p]] > 0] == _edges(wd), (wd, r)
        assert {-1, LISTS_MAX, INT32_MAX, INT32_MIN} <= set(pr[4].tolist()) and len(set(pr[4].tolist())) < wd
        assert len(set(pr[7].tolist())) == len(set(pr[8].tolist())) == 1 and pr[8, 0] == WIDE_LONG and len(set(pr[13].tolist())) == 9
        clean, damaged = _wide_host(wd, 10, False), _wide_host(wd, 10, True)
        assert clean[2][8] == WIDE_LONG_ROWS and clean[2][7] == 7 and clean[2][9] == clean[2][10] == 0 and clean[2][0] > 0
        assert clean[2][4] == sum(sh.sizes[pr[4, p]] for p in _edges(wd)) and all(clean[2][r] != damaged[2][r] for r in (0, 1, 2, 3, 7, 11, 12))
    cs = T.clamp_starts(sh.bad_start, sh.n)
    assert sh.damaged == 306 and (sh.bad_start < 0).sum() >= 100 and (np.diff(sh.bad_start) < 0).sum() >= 200 and (sh.bad_start > sh.n).sum() == 3
    assert all(sh.bad_start[p] != sh.start[p] for p in (0, 1, 1024, 4000, 4095, 4096)) and cs[-1] == cs[4000] == sh.n and cs[0] == cs[1] == 0
    assert sh.bad_mlr >= sh.mlr and (np.diff(cs) == 0).sum() > (sh.sizes == 0).sum() + 300
    # -- section 3 --
    r = _rescore()
    assert _cap_binds(RESCORE_NQ * RESCORE_R, RESCORE_NQ) and _launches(RESCORE_NQ * RESCORE_R, RESCORE_NQ, 1, RESCORE_R) == [(1024, 128, 128)]
    assert RESCORE_NQ <= LISTS_MAX and r.order.shape[0] == RESCORE_NQ * RESCORE_R != CAP_N and (r.order == -1).sum() > 50000
    assert np.array_equal(r.want[32][2], r.counts) and {0, 1, RESCORE_R - 1, RESCORE_R} <= set(r.counts.tolist())
    holes_inside = [(r.order[q * RESCORE_R:(q + 1) * RESCORE_R][:-1] < 0).any() and r.order[(q + 1) * RESCORE_R - 1] >= 0 for q in range(RESCORE_NQ)]
    assert sum(holes_inside) > 50
    s = _subset()
    assert 4000 < s.order.shape[0] < 6000 and s.start[-1] == s.order.shape[0] and (s.want[2] > 0).sum() > 30
    # -- section 4 --
    b = _big()
    assert b.n == N_A == LINE + 64 * 3 + 5 and b.n % 64 == 5 and BIG_K == KMAX and RPB_LIMIT in BIG_RPBS
    assert {LINE - 1, LINE, b.n - 1} <= set(b.rows[:, 0].tolist()) and (b.rows[:, 2::2] >= LINE).all() and (b.rows[:, 1::2] < LINE).all()
    P_big = min(BIG_NPROBE * b.mlr, b.n)
    assert P_big > 200000 and [u for rpb in BIG_RPBS for _, _, u in _launches(b.n, BIG_NQ, BIG_NPROBE, b.mlr, rpb)] == [64, 1024, 1 << 20]
    for j in range(BIG_NQ):
        lab = b.labels[b.rows[j]]
        assert np.array_equal(np.isin(lab, b.probes[j]), b.status != "unp")
        assert b.masks[0][b.rows[j][b.status == "vis"]].all() and not b.masks[2][b.rows[j][b.status == "clr"]].any()
    # -- section 5 --
    assert all(64 * 12 < d < 8192 and d % 64 == 0 for d in LARGE_DIMS)


@pytest.mark.parametrize("case", BIG_CASES)
def test_big_fixtures_by_fp64_alone(case):
    """CPU only, the reference alone.  `_big_expected` raises where float64 does not decide a planted row or a threshold.  Beyond that: every
    visible planted row of a query is in its expected list wherever the threshold lets it, in the order it was planted; the hidden ones
    (unprobed list, cleared bit) are not; the lists hold rows on both sides of 2^20, rows 2^20 - 1, 2^20 and the shard's last among them;
    and the case bites: the float64 ranking of ALL rows, and of the probed rows without the filter, give other lists."""
    sh, ref = _big(), _big_ref("cpu")
    exp = _big_expected(case, "cpu")
    tops = set()
    for j, x in enumerate(exp):
        vis_planted = sh.rows[j][x.visible[sh.rows[j]]]
        m = min(x.hits, BIG_K)
        assert x.ids[:min(m, vis_planted.shape[0])].tolist() == vis_planted[:m].tolist(), (case, j)
        assert not np.isin(x.hidden, x.ids).any() and x.hidden.shape[0] == {None: 10, 0: 20, 1: 10, 2: 20}[_big_filter(case, j)]
        assert x.decided[:min(m, vis_planted.shape[0])].all() and x.n_visible > 50000
        if m >= 12:
            assert (x.ids[:m] >= LINE).sum() >= 4 and ((x.ids[:m] >= 0) & (x.ids[:m] < LINE)).sum() >= 4
        if m:
            tops.add(int(x.ids[0]))
        if m >= 8:
            everything = np.argsort(-ref.e[j], kind="stable")[:m]
            assert everything.tolist() != x.ids[:m].tolist(), (case, j, "the exact search gives the same list")
        if case == "multi":
            kind = BIG_THR[j]
            assert (x.hits == kind if isinstance(kind, int) else 3000 < x.hits <= 3100 if kind == "low" else
                    x.hits == (x.n_visible if kind == "-inf" else 0)), (j, kind, x.hits)
    assert case == "multi" or {LINE - 1, LINE, sh.n - 1} <= tops
    if case != "plain":
        plain = _big_expected("plain", "cpu")
        assert all(not np.array_equal(a.ids, b.ids) for j, (a, b) in enumerate(zip(exp, plain)) if _big_filter(case, j) != 1 and a.hits)


# ---- the GPU side -------------------------------------------------------------------------------------------------------------------------------------------------
_DEV = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_shards():
    """the device copies and the large host arrays go with the module"""
    yield
    _DEV.clear()
    _BIG_REF.clear()
    _big_expected.cache_clear()
    _big.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _on_device(name):
    """the device copies of a shard, made on first use and shared"""
    if name not in _DEV:
        if name == "cap":
            w = _cap()
            _DEV[name] = SimpleNamespace(X=dev(w.X, np.float16), order=dev(w.order, np.int32), start=dev(w.start, np.int64), Q=dev(w.Q, np.float16),
                                         probes=dev(w.probes, np.int32), words=dev(words_of(w.masks, garbage=True), np.int64))
        elif name == "wide":
            sh = _wide()
            _DEV[name] = SimpleNamespace(X=dev(sh.X, np.float16), order=dev(sh.order, np.int32), start=dev(sh.start, np.int64),
                                         bad_start=dev(sh.bad_start, np.int64), Q=dev(sh.Q, np.float16))
        else:
            b = _big()
            _DEV[name] = SimpleNamespace(C=dev(b.C, np.float16), order=dev(b.order, np.int32), start=dev(b.start, np.int64), Q=dev(b.Q, np.float16),
                                         probes=dev(b.probes, np.int32), words=dev(words_of(b.masks, garbage=True), np.int64), fo=dev(b.fo, np.int32))
    return _DEV[name]


def _cap_run(idx, k, rpb, cut=None, base=0, order=None, start=None, mlr=None):
    """The three calls of a section-1 case over the pairs `idx` -> (`ivf_search`, `ivf_search_multi` without filters, `ivf_search_multi`
    under the filters and thresholds), device tensors."""
    w, d = _cap(), _on_device("cap")
    sel = dev(idx, np.int64)
    Q, probes = d.Q[sel].contiguous(), d.probes[sel].contiguous()
    args = (d.X, d.order if order is None else order, d.start if start is None else start, (w.mlr if mlr is None else mlr) if cut is None else cut,
            Q, probes, k)
    kw = dict(idx_base=base, rows_per_block=rpb)
    return (I.ivf_search(*args, **kw), I.ivf_search_multi(*args, **kw),
            I.ivf_search_multi(*args, allows=d.words, filter_of=dev(w.fo[idx], np.int32), min_score=dev(w.thr[idx], np.float32), **kw))


def _assert_cap(got, k, idx, what, cut=None, base=0):
    for name, g, want in zip(("ivf_search", "ivf_search_multi", "ivf_search_multi, filters and thresholds"), got, _cap_host(k, cut)):
        assert same(g, _based(_tiled(want, idx), base)), (what, name)


# ---- 1. the capped workspace --------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nq,rpb", CAP_LAUNCHES, ids=[f"{nq}q-rpb{rpb}" for nq, rpb in CAP_LAUNCHES])
def test_the_capped_workspace_and_the_forced_raise_give_the_definition(hip, nq, rpb):
    """The 70 pairs tiled to nq queries over the 10 000-row shard, k = 10 and 32, both entry points (the multi entry also under four
    filters, `filter_of` outside [0, n_filters) and every kind of threshold: part_m sits behind the other arrays of the capped layout):
    scores, ids, `scanned` and `hits` are `search_host` / `search_many_host` of the 70 pairs, tiled, bit for bit.  Which of these
    launches the workspace caps and which rows_per_block the host raises is asserted by the CPU test of section 0."""
    idx = np.arange(nq) % CAP_PAIRS
    shape = _launches(CAP_N, nq, CAP_NPROBE, _cap().mlr, rpb)
    for k in CAP_KS:
        _assert_cap(_cap_run(idx, k, rpb), k, idx, (nq, rpb, k))
    print(f"capped {nq} queries, rows_per_block {rpb}: slots {_slots(CAP_N, nq)} (cap binds: {_cap_binds(CAP_N, nq)}); per internal batch "
          f"(queries, asked or default, used) = {shape}")


# ---- 2. 4 096 lists and 128 probes --------------------------------------------------------------------------------------------------------------------------------
def _wide_run(pr, k, damaged, Q=None):
    sh, d = _wide(), _on_device("wide")
    return I.ivf_search(d.X, d.order, d.bad_start if damaged else d.start, sh.bad_mlr if damaged else sh.mlr, d.Q if Q is None else Q,
                        dev(pr, np.int32), k)


@gpu
@pytest.mark.parametrize("damaged", [False, True], ids=["clean-start", "damaged-start"])
@pytest.mark.parametrize("width", WIDTHS)
def test_wide_probe_rows_over_4096_lists(hip, width, damaged):
    """14 probe rows of the width, built on purpose (`_wide_probes`), over 4 096 lists - with `start` as built, and damaged at 306 places
    (max_list_rows from `clamp_starts`): `search_host` bit for bit at k = 10 and 32; the multi entry the same with hits = scanned; every
    query alone with its row narrowed to the distinct valid entries gives the same bits; and so does the filtered search over
    `probe_bitmaps_host` of the batch."""
    from arxiv_rag_amd.index import ShardIndex
    sh, d = _wide(), _on_device("wide")
    pr = _wide_probes(width)
    start = sh.bad_start if damaged else sh.start
    for k in WIDE_KS:
        got, want = _wide_run(pr, k, damaged), _wide_host(width, k, damaged)
        assert same(got, want), (width, damaged, k)
        multi = I.ivf_search_multi(d.X, d.order, d.bad_start if damaged else d.start, sh.bad_mlr if damaged else sh.mlr, d.Q, dev(pr, np.int32), k)
        assert same(multi, want + (want[2],)), (width, damaged, k, "multi")
    for q in range(WIDE_NQ):
        alone = _wide_run(_narrowed(pr[q]), 32, damaged, Q=d.Q[q:q + 1].contiguous())
        assert same(alone, _tiled(want, [q])), (width, damaged, q, "narrowed to the distinct valid probes")
    maps = I.probe_bitmaps_host(sh.order, start, pr, sh.n)
    s, i = ShardIndex(d.X, prefilter=None).search_filtered_many(d.Q, dev(maps, np.int64), torch.arange(WIDE_NQ, dtype=torch.int32, device=DEV), 32, path=2)
    assert same((got[0], got[1]), (s, i)), (width, damaged, "filtered search over the probe bitmaps")


# ---- 3. cut lists, empty input, id base, subsets, NULL outputs -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cut", CUTS)
def test_cut_lists_with_an_id_base(hip, cut):
    """max_list_rows below the long list's 6 000 entries (0: nothing is read), idx_base = 1 << 33, k = 1, 31, 32, both entry points: the
    host with `max_list_rows`, bit for bit; `scanned` and `hits` count the rows inside the cut; ids are row + idx_base, the padding -1."""
    idx = np.arange(CAP_PAIRS)
    whole = _cap_host(32)[1]
    for k in CUT_KS:
        got = _cap_run(idx, k, None, cut=cut, base=BASE)
        _assert_cap(got, k, idx, (cut, k), cut=cut, base=BASE)
        ids, scanned = _np(got[1][1]), _np(got[1][2])
        assert ((ids == -1) | (ids >= BASE)).all() and (scanned <= CAP_NPROBE * cut).all() and (scanned <= whole[2]).all()
        assert cut == 0 or (scanned < whole[2]).any()
    if cut == 0:
        assert all((_np(g[2]) == 0).all() and (_np(g[1]) == -1).all() and np.isneginf(_np(g[0])).all() for g in got)


@gpu
def test_no_members_at_all(hip):
    """n_members = 0 with an empty `order` tensor (the library gets NULL) and max_list_rows = 0: everything is (-inf, -1), no row scanned."""
    w, d = _cap(), _on_device("cap")
    order, start = torch.empty(0, dtype=torch.int32, device=DEV), torch.zeros(len(CAP_SIZES) + 1, dtype=torch.int64, device=DEV)
    for k in (1, 32):
        for got in _cap_run(np.arange(CAP_PAIRS), k, None, base=BASE, order=order, start=start, mlr=0):
            assert all((_np(c) == 0).all() for c in got[2:]) and (_np(got[1]) == -1).all() and np.isneginf(_np(got[0])).all()
    wild = dev(np.array([5, -3, 1 << 40] + [9] * (len(CAP_SIZES) - 2)), np.int64)                  # `start` is clamped into [0, 0]
    got = I.ivf_search(d.X, order, wild, 0, d.Q, d.probes, 10, rows_per_block=64)
    assert (_np(got[2]) == 0).all() and (_np(got[1]) == -1).all() and np.isneginf(_np(got[0])).all()


@gpu
def test_lists_that_hold_a_subset_of_the_rows(hip):
    """`order` shorter than n_rows (half of the rows are in no list), and the rescore's layout of the binary and PQ searches: n_lists =
    n_queries = 1 024, start[q] = 256 q, probes[q] = {q}, `order` the candidates with -1 holes in irregular patterns (n_members = 262 144
    over a shard of 10 000 rows: the workspace cap binds).  `search_host` / `search_many_host`, bit for bit."""
    w, d, s, r = _cap(), _on_device("cap"), _subset(), _rescore()
    for rpb in (None, 64):
        got = I.ivf_search_multi(d.X, dev(s.order, np.int32), dev(s.start, np.int64), s.mlr, d.Q, d.probes, 10, allows=d.words,
                                 filter_of=dev(w.fo, np.int32), min_score=dev(w.thr, np.float32), idx_base=BASE, rows_per_block=rpb)
        assert same(got, _based(s.want, BASE)), ("subset", rpb)
    args = (d.X, dev(r.order, np.int32), dev(r.start, np.int64), RESCORE_R, dev(r.Q, np.float16), dev(r.probes, np.int32))
    for k in (10, 32):
        for rpb in (None, 64, RPB_LIMIT):
            assert same(I.ivf_search(*args, k, rows_per_block=rpb), r.want[k]), ("rescore layout", k, rpb)
    multi = I.ivf_search_multi(*args, 32, idx_base=BASE)
    assert same(multi, _based(r.want[32] + (r.want[32][2],), BASE))


@gpu
def test_null_count_outputs_leave_the_other_outputs_unchanged(hip):
    """The library called directly with out_scanned and / or out_hits NULL: scores, ids and the count that is asked for are those of the
    call with every output."""
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    w, d = _cap(), _on_device("cap")
    k, nq = 10, CAP_PAIRS
    fo, thr = dev(w.fo, np.int32), dev(w.thr, np.float32)
    want_one, _, want_multi = _cap_host(k)
    ws = torch.empty(lib.arx_ivf_multi_workspace_bytes(CAP_N, len(CAP_SIZES), nq, CAP_NPROBE, DIM, k), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(multi, scanned, hits):
        s, i = torch.full((nq, k), 7.0, dtype=torch.float32, device=DEV), torch.full((nq, k), 7, dtype=torch.int64, device=DEV)
        n, h = torch.full((nq,), -7, dtype=torch.int64, device=DEV), torch.full((nq,), -7, dtype=torch.int64, device=DEV)
        head = (d.X.data_ptr(), CAP_N, DIM, d.order.data_ptr(), CAP_N, d.start.data_ptr(), len(CAP_SIZES), w.mlr, d.Q.data_ptr(), nq,
                d.probes.data_ptr(), CAP_NPROBE)
        tail = (BASE, ws.data_ptr(), ws.numel(), stream)
        if multi:
            rc = lib.arx_ivf_search_multi(*head, d.words.data_ptr(), CAP_NF, fo.data_ptr(), thr.data_ptr(), k, s.data_ptr(), i.data_ptr(),
                                          n.data_ptr() if scanned else None, h.data_ptr() if hits else None, *tail)
        else:
            rc = lib.arx_ivf_search(*head, None, k, s.data_ptr(), i.data_ptr(), n.data_ptr() if scanned else None, *tail)
        _lib.check(rc, "arx_ivf_search_multi" if multi else "arx_ivf_search")
        torch.cuda.synchronize()
        return s, i, n, h

    for scanned in (True, False):
        s, i, n, h = call(False, scanned, False)
        assert same((s, i), _based(want_one, BASE)[:2]) and (_np(h) == -7).all()
        assert np.array_equal(_np(n), want_one[2]) if scanned else (_np(n) == -7).all()
        for hits in (True, False):
            s, i, n, h = call(True, scanned, hits)
            assert same((s, i), _based(want_multi, BASE)[:2]), (scanned, hits)
            assert np.array_equal(_np(n), want_multi[2]) if scanned else (_np(n) == -7).all()
            assert np.array_equal(_np(h), want_multi[3]) if hits else (_np(h) == -7).all()


# ---- 4. rows past 2^20, held to float64 -------------------------------------------------------------------------------------------------------------------------------
def _big_run(case, rpb):
    sh, d = _big(), _on_device("big")
    args = (d.C, d.order, d.start, sh.mlr, d.Q, d.probes, BIG_K)
    if case == "multi":
        thr = np.array([x.thr for x in _big_expected(case, DEV)], np.float32)
        return I.ivf_search_multi(*args, allows=d.words, filter_of=d.fo, min_score=dev(thr, np.float32), idx_base=BASE, rows_per_block=rpb)
    got = I.ivf_search(*args, allow=d.words[0] if case == "bitmap" else None, idx_base=BASE, rows_per_block=rpb)
    return got + (got[2],)


@gpu
@pytest.mark.parametrize("case", BIG_CASES)
def test_rows_past_2_20_are_the_fp64_definition_at_every_launch_shape(hip, case):
    """2^20 + 197 unit rows in 40 lists, 8 queries probing 8 lists each, k = 32, idx_base = 1 << 33; `plain` (`ivf_search`, no filter),
    `bitmap` (`ivf_search` under a random half whose last word has its spare bits set) and `multi` (three filters and every kind of
    threshold).  Per query against float64 over its visible rows: `scanned` and `hits` are exact, the padding starts where the hits end,
    the id is equal wherever float64 decides (every planted row: rows on both sides of 2^20, rows 2^20 - 1, 2^20 and the shard's last),
    every returned row is visible, qualifies and is returned once, its score lies within B(D) |q| |c| of float64, the score at every
    position within B(D) |q| max|c| of the float64 score of that rank, and no planted row of an unprobed list or under a cleared bit
    appears.  rows_per_block = 64, the default and 2^20 return the same bits."""
    sh, ref, exp = _big(), _big_ref(DEV), _big_expected(case, DEV)
    runs = [tuple(_np(t) for t in _big_run(case, rpb)) for rpb in BIG_RPBS]
    s, i, scanned, hits = runs[0]
    for rpb, other in zip(BIG_RPBS[1:], runs[1:]):
        assert same(other, runs[0]), (case, rpb, "not the bits of rows_per_block = 64")
    worst, n_decided, n_held = 0.0, 0, 0
    for j, x in enumerate(exp):
        what = (case, j)
        assert scanned[j] == x.n_visible and hits[j] == x.hits, (what, "counts", int(scanned[j]), x.n_visible, int(hits[j]), x.hits)
        m = min(x.hits, BIG_K)
        assert (i[j, :m] >= BASE).all() and (i[j, m:] == -1).all() and np.isneginf(s[j, m:]).all(), (what, "padding")
        loc = i[j, :m] - BASE
        assert np.array_equal(loc[x.decided[:m]], x.ids[:m][x.decided[:m]]), (what, "ids differ from the float64 definition")
        assert x.visible[loc].all() and np.unique(loc).shape[0] == m and not np.isin(x.hidden, loc).any(), (what, "a row the query cannot see")
        assert (s[j, :m] >= x.thr).all() if m else True, (what, "a row below the threshold")
        a, b = slice(0, max(m - 1, 0)), slice(1, max(m, 1))
        assert ((s[j, a] > s[j, b]) | ((s[j, a] == s[j, b]) & (loc[a] < loc[b]))).all(), (what, "order")
        err = np.abs(s[j, :m].astype(np.float64) - ref.e[j, loc]) / (pass_b_budget(DIM) * ref.qn[j] * ref.cn[loc])
        assert (err <= 1).all(), (what, "a score outside the pass-B budget", float(err.max()))
        assert (np.abs(s[j, :m].astype(np.float64) - x.sv[:m]) <= ref.tol[j] / 2).all(), (what, "the score of a rank outside the budget")
        worst, n_decided, n_held = max(worst, float(err.max()) if m else 0.0), n_decided + int(x.decided[:m].sum()), n_held + m
    print(f"big {case}: visible rows per query {[x.n_visible for x in exp]}; hits {[x.hits for x in exp]}; positions float64 decides "
          f"{n_decided} of {n_held}; worst error / budget {worst:.3f}")


# ---- 5. dims between 768 and 8192 ---------------------------------------------------------------------------------------------------------------------------------------
LARGE_DIMS = (1536, 4096)


@gpu
@pytest.mark.parametrize("d", LARGE_DIMS)
def test_dims_1536_and_4096(hip, d):
    """300 rows in 3 lists, as the first suites' test_dim_8192: both entry points, the host bit for bit."""
    rs = np.random.RandomState(d)
    X = (rs.randn(300, d) / np.sqrt(d)).astype(np.float16)
    labels = rs.randint(0, 3, 300).astype(np.int32)
    order, start, sizes = T.members_host(labels, 3)
    Q = (rs.randn(3, d) / np.sqrt(d)).astype(np.float16)
    probes = np.array([[0, 2], [1, 1], [2, 0]], np.int32)
    masks = np.stack([rs.rand(300) < 0.5, rs.rand(300) < 0.2])
    fo, thr = np.array([0, 1, 2], np.int32), np.array([0.0, -np.inf, 0.0], np.float32)
    args = (dev(X, np.float16), dev(order, np.int32), dev(start, np.int64), int(sizes.max()), dev(Q, np.float16), dev(probes, np.int32))
    for k in (10, 32):
        for rpb in (None, 64):
            assert same(I.ivf_search(*args, k, idx_base=BASE, rows_per_block=rpb), _based(I.search_host(X, order, start, probes, Q, k), BASE)), (d, k, rpb)
            got = I.ivf_search_multi(*args, k, allows=dev(words_of(masks), np.int64), filter_of=dev(fo, np.int32), min_score=dev(thr, np.float32),
                                     idx_base=BASE, rows_per_block=rpb)
            want = I.search_many_host(X, order, start, probes, Q, k, allows=masks, filter_of=fo, min_score=thr)
            assert same(got, _based(want, BASE)) and want[3][0] > 0 and want[3][2] == 0, (d, k, rpb)
