"""The score-threshold search (`ShardIndex.search_range`, csrc/range.hip) and the grouped search (`search_grouped`, csrc/grouped.hip) where
their own suites stop: shards of more than FILT_REG_GROUPS * FILT_TAIL_NT = 16 384 groups (2^20 rows), whose further group maxima
`tail_kth_key` and `tail_candidates` (csrc/masked_topk.h) re-read from memory in loops of their own, with ksel = M + 1 up to 1 025 and
K = P S up to 512; and dims 1536 / 4096 / 8192, up to the dynamic-LDS sizes at which the hosts raise their kernels' limits.
tests/test_gpu_masked_search_large.py crosses the same lines for masked_tail_kernel, which carries an inline COPY of tail_kth_key: the
function itself is called by range_tail_kernel and grouped_tail_kernel alone.

Every reference is float64 (tests/helpers.py: scores_fp64, pass_b_budget) or an independent path of the library (`search` over a
bitmap of the returned rows); neither search is compared with itself alone.

The two shards have the shapes, seeds and planted layout (`_planted_layout`) of the masked suite -
  A  64 * 16384 + 64 * 3 + 5 rows: four spilled groups, the last ragged (only lanes 0 ... 3 of wave 0 work in the spill loops)
  B  256 * 4369 rows: 17 476 groups, 1 092 spilled (every wave one spill iteration, waves 0 and 1 a second)
- but are drawn by numpy, not by the device's generator, so that the CPU tests of this file see the very rows the GPU tests search and
can assert every precondition from float64 without a GPU.  For each of the first 32 queries q, 64 rows a q + sqrt(1 - a^2) noise with
a from 0.95 down to 0.70 are planted in 64 distinct groups, the ranks alternating between the spilled groups and the first 16 384
(groups 16383, 16384 and the shard's last among them); a chance row scores below 0.125 sqrt(2 ln N) = 0.66.

How an answer is held to float64.  The expected list of a query is the float64 order of its visible rows, cut at the threshold and at
M.  float64 decides the row at a position when the gaps to both neighbours exceed twice B(D) |q| max|c| (B = pass_b_budget: a returned
f32 score lies within B |q| |c| of float64, so rows further apart than 2 B |q| |c| cannot swap): there the id must be equal.  Every
position that holds a planted row must be decided - a fixture error otherwise, never a skip - as must the threshold (no listed row
within B |q| |c| of it) and with it the count.  Where two chance rows lie closer than that (a list of 1 024 out of 10^6 rows has a few
such pairs), check_range_fp64's budgeted conditions hold the position.  The grouped answers are held the same way to `_fold` (of
tests/test_gpu_grouped_search.py) fed float64.

Figures printed (profiles/range_grouped_large_fp64.md): allowed rows, overflowed queries, candidate groups per query and the worst
score error over its budget, per case."""
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import pass_b_budget, scores_fp64
from tests.range_cases import check_range_fp64
from tests.test_gpu_grouped_search import _check_fp64 as _grouped_check_fp64, _fold
from tests.test_gpu_masked_search_large import (BASE, CAP_DEFAULT, CAP_MAX, CSRC, DIM, GROUP, LINE, LINE_G, N_A, N_B, N_PLANTED, PLANTED_ROWS,
                                                REG_GROUPS, TAIL_NT, _define, _planted_layout, hip)  # noqa: F401  (`hip`: the module's fixture)

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

# ---- the constants the shapes below are derived from, read from the sources: if one changes, the CPU tests below fail ---------------------
PARTS_MAX = _define("masked_topk.h", "FILT_PARTS_MAX")
RANGE_CAP = _define("range.hip", "RANGE_CAP")
RANGE_PART_KEYS = _define("range.hip", "RANGE_PART_KEYS")
RANGE_MAX = _define("range.hip", "RANGE_MAX_RESULTS")
KSEL_MAX = _define("grouped.hip", "GRP_KSEL_MAX")
KMAX = _define("search_consts.h", "KMAX")
QBATCH = _define("search_consts.h", "QBATCH_MAX")
NQ_ALL = QBATCH + 1                                               # two internal slices
NS = {"A": N_A, "B": N_B}
SEEDS = {"A": 1101, "B": 1102}                                    # the masked suite's
RANGE_BASE = {"A": 7, "B": BASE}                                  # idx_base of the range cases (BASE = 1 << 33)
MS = (1, 32, 33, 1024)
INF = float("inf")


def _groups(n):
    return (n + GROUP - 1) // GROUP


def _range_cand_cap(M):
    """arx_range_search_tuned: the default capacity of the candidate list"""
    return 2 * (M + 1) + CAP_DEFAULT


def _range_parts(n, M):
    """range_layout: the parts of the exhaustive path"""
    return min((n + 255) // 256, PARTS_MAX, RANGE_PART_KEYS // M)


def _tail_dyn(dim, cand_cap):
    """dynamic LDS of range_tail_kernel and grouped_tail_kernel: the query row, one 64-score stretch per wave, the candidate list"""
    return ((dim * 2 + 15) & ~15) + (TAIL_NT // 64) * GROUP * 4 + cand_cap * 4


RANGE_RAISE, GROUPED_RAISE = 32 * 1024, 48 * 1024                 # the hosts ask for more dynamic LDS above these (range.hip, grouped.hip)
RANGE_LIST_BYTES = RANGE_CAP * 8 + 16                             # static: struct RangeList
TAIL_STAGE_BYTES = (TAIL_NT // 64) * 4 + 8                        # static: struct TailStage
LARGE_DIMS = (1536, 4096, 8192)
LARGE_N = 64 * 5 + 9
LARGE_RANGE_MS = (10, 1024)
LARGE_GROUPED = ((3, 2), (32, 8))

# ---- the grouped layouts: run lengths (cycled), the value of run j is 3 j + 5 ----------------------------------------------------------------
LAYOUTS = {
    "runs-1-7": dict(first=None, cycle=(1, 2, 3, 4, 5, 6, 7)),
    "runs-64-off32": dict(first=32, cycle=(64,)),
    "runs-200-straddle": dict(first=76, cycle=(200,)),          # a run is rows 2^20 - 100 ... 2^20 + 99
}
# (shard, layout, P, m, max_run_rows or None): K = P S
GROUPED_CASES = [
    ("B", "runs-1-7", 1, 1, None), ("B", "runs-1-7", 10, 3, None), ("B", "runs-1-7", 32, 8, None),
    ("B", "runs-64-off32", 10, 3, None), ("B", "runs-64-off32", 32, 8, None),
    ("B", "runs-200-straddle", 10, 3, None), ("B", "runs-200-straddle", 32, 1, None), ("B", "runs-200-straddle", 32, 8, None),
    ("B", "runs-200-straddle", 32, 2, 1000),
    ("A", "runs-200-straddle", 10, 3, None), ("A", "runs-1-7", 32, 8, None),
]
GROUPED_MASKS = ("none", "beyond", "best-hidden")
GROUPED_K = {("runs-1-7", 1): 2, ("runs-1-7", 10): 20, ("runs-1-7", 32): 64, ("runs-64-off32", 10): 20, ("runs-64-off32", 32): 64,
             ("runs-200-straddle", 10): 50, ("runs-200-straddle", 32): 160}


def _layout(name, n):
    """-> (group_of int32 [n], run starts int64 [runs + 1])"""
    L = LAYOUTS[name]
    reps = n // sum(L["cycle"]) + 2
    lens = np.concatenate([[L["first"]] if L["first"] else [], np.tile(L["cycle"], reps)]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])
    starts = np.concatenate([starts[starts < n], [n]])
    runs = starts.shape[0] - 1
    return np.repeat(3 * np.arange(runs, dtype=np.int64) + 5, np.diff(starts)).astype(np.int32), starts


def _select_count(P, R):
    from arxiv_rag_amd.grouping import select_count
    return select_count(P, R)


# ---- 0. CPU only: the constants and the arithmetic the GPU cases rely on --------------------------------------------------------------------
def test_the_cases_cross_the_lines_by_the_constants_of_the_sources():
    assert (TAIL_NT, REG_GROUPS, GROUP, CAP_DEFAULT, CAP_MAX, PARTS_MAX) == (1024, 16, 64, 1024, 8192, 128)
    assert (RANGE_CAP, RANGE_PART_KEYS, RANGE_MAX, KSEL_MAX, KMAX, QBATCH) == (2048, 4096, 1024, 512, 32, 1024)
    assert LINE_G == 16384 and LINE == 1 << 20 and (N_A, N_B) == (1048773, 1118464)
    # which groups spill, and the iterations of the spill loops per wave (they start at group LINE_G + 64 w and advance by TAIL_NT)
    assert _groups(N_A) - LINE_G == 4 and N_A % GROUP == 5 and _groups(N_B) - LINE_G == 1092 and N_B % GROUP == 0
    iters = lambda n, w: len(range(LINE_G + 64 * w, _groups(n), TAIL_NT))
    assert [iters(N_A, w) for w in range(16)] == [1] + [0] * 15 and [iters(N_B, w) for w in range(16)] == [2, 2] + [1] * 14
    # ksel of the range tail, its default candidate list, the exhaustive path's parts and the groups of a part (many cut-back sorts)
    assert [M + 1 for M in MS] == [2, 33, 34, 1025] and max(MS) == RANGE_MAX
    assert [_range_cand_cap(M) for M in MS] == [1028, 1090, 1092, 3074] and _range_cand_cap(max(MS)) <= CAP_MAX
    assert [_range_parts(N_B, M) for M in MS] == [128, 128, 124, 4] and [_range_parts(N_A, M) for M in MS] == [128, 128, 124, 4]
    per = [-(-_groups(N_B) // _range_parts(N_B, M)) for M in MS]
    assert per == [137, 137, 141, 4369] and all(p * GROUP > 4 * RANGE_CAP for p in per)          # a part overflows its slots over and over
    assert _range_parts(N_B, 1024) * 1024 <= RANGE_PART_KEYS and RANGE_CAP == 2 * TAIL_NT == 1024 + 16 * GROUP
    # the bitmap "fewer than M + 1 non-empty groups, all spilled" exists on B for every M (and for M = 1 024 on A)
    assert all(min(M, 1000) < M + 1 and min(M, 1000) <= _groups(N_B) - LINE_G for M in MS)
    # K = P S of every grouped case: S = floor((R + 62) / 64) + 1 from the longest run R; one case above GRP_KSEL_MAX (whole call exhaustive)
    for name, R, S in (("runs-1-7", 7, 2), ("runs-64-off32", 64, 2), ("runs-200-straddle", 200, 5)):
        for n in (N_A, N_B):
            g, starts = _layout(name, n)
            assert g.shape == (n,) and int(np.diff(starts).max()) == R and _select_count(1, R) == S and (np.diff(g) >= 0).all()
            assert g[0] == 5 and g[-1] == 3 * (starts.shape[0] - 2) + 5 > starts.shape[0]            # not dense
    for sh, name, P, m, R in GROUPED_CASES:
        if R is None:
            assert _select_count(P, int(np.diff(_layout(name, NS[sh])[1]).max())) == GROUPED_K[(name, P)] <= KSEL_MAX
    assert ("B", "runs-200-straddle", 32, 1, None) in GROUPED_CASES and GROUPED_K[("runs-200-straddle", 32)] == 160
    assert _select_count(32, 1000) == 544 > KSEL_MAX and ("B", "runs-200-straddle", 32, 2, 1000) in GROUPED_CASES
    for n in (N_A, N_B):
        starts = _layout("runs-200-straddle", n)[1]
        assert LINE - 100 in starts and LINE + 100 in starts
    assert N_A - _layout("runs-200-straddle", N_A)[1][-2] == 97 and _layout("runs-200-straddle", N_A)[1][-2] < (N_A // GROUP) * GROUP   # A's last paper ends in the ragged group
    off32 = _layout("runs-64-off32", N_B)[1]
    assert (off32[1:-1] % GROUP == 32).all()
    # dynamic LDS: which (dim, cand_cap) cells cross each kernel's raise-the-limit line
    cross = lambda line, caps: {(d, c) for d in LARGE_DIMS for c in caps if _tail_dyn(d, c) > line}
    caps_r = {_range_cand_cap(M) for M in LARGE_RANGE_MS} | {CAP_MAX}
    assert caps_r == {1046, 3074, 8192}
    assert cross(RANGE_RAISE, caps_r) == {(8192, 3074), (1536, 8192), (4096, 8192), (8192, 8192)}
    assert _tail_dyn(8192, 3074) == 32776 and _tail_dyn(8192, 1046) == 24664 and _tail_dyn(4096, 3074) == 24584
    assert cross(GROUPED_RAISE, {CAP_DEFAULT, CAP_MAX}) == {(8192, 8192)} and _tail_dyn(8192, CAP_MAX) == 53248 and _tail_dyn(4096, CAP_MAX) == 45056
    # the range tail's whole LDS at dim 8192 with the largest list: above the 64 KiB of earlier parts, inside gfx950's 160 KiB
    whole = _tail_dyn(8192, CAP_MAX) + RANGE_LIST_BYTES + TAIL_STAGE_BYTES
    assert whole == 69720 and 64 * 1024 < whole < 160 * 1024
    # the exhaustive and the chunk kernels (query row + a stretch per wave) stay below both lines at every dim the library takes
    assert _tail_dyn(8192, 0) == 20480 < RANGE_RAISE and ((8192 * 2 + 15) & ~15) + 4 * GROUP * 4 == 17408 < GROUPED_RAISE


def _strip(text):
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"\bksel\b", "k", text)
    return re.sub(r"\s+", "", text)


def _cut(text, after, first, end):
    a = text.index(after)
    b = text.index(first, a)
    return text[b:text.index(end, b)]


def test_the_two_texts_of_the_select_are_the_same():
    """masked_tail_kernel carries tail_kth_key's text inline ("Keep the two texts the same"): from the fill of kv to the end of the bit
    loop, without comments and whitespace and with ksel called k, the function's body and the inline copy are one text."""
    src = (CSRC / "masked_topk.h").read_text()
    fn = _strip(_cut(src, "uint32_t tail_kth_key(TailStage& st", "#pragma unroll", "return T;"))
    inline = _strip(_cut(src, "void masked_tail_kernel(const float*", "uint32_t kv[FILT_REG_GROUPS];", "const float thr ="))
    inline = inline[len(_strip("uint32_t kv[FILT_REG_GROUPS];")):]
    assert fn.startswith("#pragmaunrollfor(intj=0;j<FILT_REG_GROUPS;++j)") and fn.endswith("T=tot>=k?cand:T;}")
    assert len(fn) > 600 and "for(intbit=31;bit>=0;--bit)" in fn and fn.count("__ballot") == 2 and fn.count("__syncthreads()") == 3
    assert fn == inline
    # ... and the two tails that call the function do call it
    for name, ksel in (("range.hip", "M + 1"), ("grouped.hip", "ksel")):
        assert f"tail_kth_key(st, kv, col, ldg, n_groups, qs, D, {ksel})" in (CSRC / name).read_text(), name


# ---- 1. the two shards, drawn by numpy: the same rows on the CPU and on the GPU --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shard_np(name):
    """-> (C fp16 [n, 64], Q fp16 [1025, 64], planted rows int64 [32, 64]), all numpy"""
    n = NS[name]
    rng = np.random.default_rng(SEEDS[name])
    C_ = rng.standard_normal((n, DIM), dtype=np.float32)
    C_ /= np.linalg.norm(C_, axis=1, keepdims=True)
    Q_ = rng.standard_normal((NQ_ALL, DIM), dtype=np.float32)
    Q_ = (Q_ / np.linalg.norm(Q_, axis=1, keepdims=True)).astype(np.float16)
    rows, a = _planted_layout(n, n)
    qh = Q_[:N_PLANTED].astype(np.float32)
    qh /= np.linalg.norm(qh, axis=1, keepdims=True)
    noise = rng.standard_normal((N_PLANTED, PLANTED_ROWS, DIM), dtype=np.float32)
    noise -= (noise * qh[:, None, :]).sum(2, keepdims=True) * qh[:, None, :]
    noise /= np.linalg.norm(noise, axis=2, keepdims=True)
    C_ = C_.astype(np.float16)
    at = a.astype(np.float32)[:, :, None]
    C_[rows.ravel()] = (at * qh[:, None, :] + np.sqrt(1 - at * at) * noise).astype(np.float16).reshape(-1, DIM)
    return C_, Q_, rows


_REFS = {}


def _ref(name, device):
    """The shard as tensors on `device` with the float64 reference of the planted queries: e64 [32, n], its 8 192 best rows per query
    (`top_v`, `top_r`), the budget's norms.  Built once per (shard, device) and left unchanged."""
    if (name, device) not in _REFS:
        C_, Q_, rows = _shard_np(name)
        C = torch.from_numpy(C_).to(device)
        Q = torch.from_numpy(Q_).to(device)
        e = scores_fp64(Q[:N_PLANTED], C)
        top_v, top_r = e.topk(8192, dim=1)
        qn = Q[:N_PLANTED].double().norm(dim=1)
        cmax = float(torch.cat([C[a:a + (1 << 18)].double().norm(dim=1).max()[None] for a in range(0, C.shape[0], 1 << 18)]).max())
        planted = torch.zeros(C.shape[0], dtype=torch.bool, device=device)
        planted[torch.from_numpy(rows).to(device).flatten()] = True
        _REFS[(name, device)] = SimpleNamespace(name=name, n=C.shape[0], C=C, Q=Q, rows=rows, e64=e, top_v=top_v, top_r=top_r, planted=planted,
                                                tol=(2 * pass_b_budget(DIM) * (1 + 1e-3) * qn * cmax).cpu().numpy(), device=device)
    return _REFS[(name, device)]


def _mask(sh, kind, M=0):
    """bool [n] on the shard's device (None: `allow=None`)"""
    n = sh.n
    if kind == "none":
        return None
    m = torch.zeros(n, dtype=torch.bool, device=sh.device)
    if kind == "ones":
        m[:] = True
    elif kind == "beyond":                                       # only rows >= 2^20
        m[LINE:] = True
    elif kind == "spilled+16383":                                # only the spilled groups plus group 16383
        m[LINE - GROUP:] = True
    elif kind == "t-inf":                                        # fewer than M + 1 non-empty groups, all of them spilled: t = -inf
        m[LINE:LINE + min(M, 1000) * GROUP] = True
    elif kind == "rand50":
        # a random half; a planted row of rank i follows the coin of its pair (i // 2: one spilled, one head rank), the first four pairs stay
        rs = np.random.RandomState(5000 + n % 1000)
        on = rs.rand(n) < 0.5
        coin = rs.rand(N_PLANTED, PLANTED_ROWS // 2) < 0.5
        coin[:, :4] = True
        on[sh.rows.ravel()] = np.repeat(coin, 2, axis=1).ravel()
        m = torch.from_numpy(on).to(sh.device)
    elif kind == "best-hidden":                                  # every row but the best chunk of each planted query
        m[:] = True
        m[torch.from_numpy(sh.rows[:, 0].copy()).to(sh.device)] = False
    else:
        raise AssertionError(kind)
    return m


def _sorted_visible(sh, vis, kk):
    """The kk best visible rows of every planted query by float64 -> (scores f64 [32, kk], rows int64 [32, kk]), numpy, (-inf, -1) where
    the mask leaves fewer."""
    if vis is None or int(vis.sum()) > 200000:
        keep = torch.ones_like(sh.top_r, dtype=torch.bool) if vis is None else vis[sh.top_r]
        assert (keep.sum(1) >= kk).all(), "the fixture's 8 192 best rows per query do not hold kk visible ones"
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :kk]
        return sh.top_v.gather(1, order).cpu().numpy(), sh.top_r.gather(1, order).cpu().numpy()
    idx = torch.nonzero(vis).flatten()
    k2 = min(kk, idx.numel())
    v, ix = sh.e64[:, idx].topk(k2, dim=1)
    sv = np.full((N_PLANTED, kk), -INF); sr = np.full((N_PLANTED, kk), -1, np.int64)
    sv[:, :k2] = v.cpu().numpy(); sr[:, :k2] = idx[ix].cpu().numpy()
    return sv, sr


SPARE = 32                                                        # rows of a sorted list behind its M + 2: a "more" threshold may lie among them
KINDS = ("spilled", "+inf", "more", "nan", "exact", "more", "-inf", "exact")          # of query j: KINDS[j % 8]


def _threshold(kind, v, r, M):
    """One query's threshold from its sorted visible float64 scores v (rows r), an f32 half way between two of them -> (value, made):
      more     more than M rows qualify (ranks 0 ... M and up to 32 more: the widest gap there): the count must be M + 1
      exact    exactly M rows qualify
      spilled  only rows at or beyond 2^20 qualify: the leading spilled rows of the list (the best row alone when every row is spilled)
    made = False (and -inf) where the mask leaves too few rows for the kind."""
    nv = int((v > -INF).sum())
    mid = lambda p: np.float32((v[p] + v[p + 1]) / 2)
    if kind == "+inf":
        return np.float32(INF), True
    if kind == "nan":
        return np.float32(np.nan), True
    if kind == "more" and nv >= M + 2:
        return mid(M + int(np.argmax(v[M:nv - 1] - v[M + 1:nv]))), True
    if kind == "exact" and nv >= M + 1:
        return mid(M - 1), True
    if kind == "spilled":
        lead = int(np.argmax(r[:nv] < LINE)) if (r[:nv] < LINE).any() else nv
        if 1 <= lead < nv:
            return mid(lead - 1), True
        if lead == nv >= 2:
            return mid(0), True
    return np.float32(-INF), kind == "-inf"


def _thresholds(sv, sr, M):
    out = [_threshold(KINDS[j % len(KINDS)], sv[j], sr[j], M) for j in range(sv.shape[0])]
    return np.array([t for t, _ in out], np.float32), np.array([ok for _, ok in out])


def _expected_range(sh, sv, sr, ms, M, what):
    """The float64 definition over the sorted visible rows (sv, sr: M + 2 + SPARE per query): threshold compared as the f32 value it is, order
    (score desc, row asc), cut at M -> ids [32, M] (local rows, -1 padding), counts [32] (M + 1 = more than M) and `decided` [32, M]:
    the positions float64 decides (module docstring).  Fixture errors: a listed row within the budget of its threshold, or a planted
    row at a position float64 does not decide."""
    assert sv.shape == (N_PLANTED, M + 2 + SPARE)
    tol = sh.tol[:, None]
    with np.errstate(invalid="ignore"):
        qual = (sv >= ms.astype(np.float64)[:, None]) & (sr >= 0)                      # (NaN: none)
        assert (qual[:, 1:] <= qual[:, :-1]).all()
        finite = np.isfinite(ms)[:, None] & (sv > -INF)
        assert not (finite & (np.abs(sv - ms.astype(np.float64)[:, None]) <= tol / 2)).any(), (what, "fixture: a row within the budget of the threshold")
        counts = np.minimum(qual.sum(1), M + 1)
        ids = np.where(qual[:, :M], sr[:, :M], -1)
        vq = np.where(qual, sv, -INF)[:, :M + 1]
        gap_ok = (vq[:, :-1] - vq[:, 1:] > tol) | (vq[:, 1:] == -INF)                   # [32, M]
    decided = np.concatenate([np.ones((N_PLANTED, 1), bool), gap_ok[:, :-1]], axis=1) & gap_ok
    planted = np.stack([np.isin(ids[j], sh.rows[j]) for j in range(N_PLANTED)])
    assert decided[planted].all(), (what, "fixture: float64 does not decide the place of a planted row")
    return SimpleNamespace(ids=ids, counts=counts, decided=decided, planted=planted)


def _interleaves(ids, k):
    """per query: (rows at or beyond 2^20, rows below) among the first k listed ones"""
    head = ids[:, :k]
    return ((head >= LINE).sum(1), ((head >= 0) & (head < LINE)).sum(1))


RANGE_MASKS = {"A": ("none", "spilled+16383", "t-inf", "rand50"), "B": ("none", "ones", "beyond", "spilled+16383", "t-inf", "rand50")}
RANGE_PARAMS = [(s, M) for s in ("A", "B") for M in MS]


def _range_case(sh, mask, M):
    """-> (vis, sorted visible rows, the two threshold vectors (all -inf; every kind across the batch), which thresholds could be made)"""
    vis = _mask(sh, mask, M)
    sv, sr = _sorted_visible(sh, vis, M + 2 + SPARE)
    mix, made = _thresholds(sv, sr, M)
    return vis, sv, sr, (np.full(N_PLANTED, -INF, np.float32), mix), made


@pytest.mark.parametrize("shard,M", RANGE_PARAMS, ids=[f"{s}-M{M}" for s, M in RANGE_PARAMS])
def test_range_fixtures_by_fp64_alone(shard, M):
    """CPU only, the reference alone.  For every mask: each expected list is decided by float64 where it holds planted rows and at its
    threshold (`_expected_range` raises otherwise); the lists of the masks that show both regions interleave them; every kind of
    threshold can be made where the mask leaves M + 2 rows; and the cases bite: a reference that ignores the groups from 16 384 on gives
    another list for EVERY planted query (M = 1: for the queries whose best row is spilled, the even ones), and the (M + 1)-th largest
    group maximum over the first 16 384 groups alone differs from the true one."""
    sh = _ref(shard, "cpu")
    for mask in RANGE_MASKS[shard]:
        what = (shard, M, mask)
        vis, sv, sr, (neg, mix), made = _range_case(sh, mask, M)
        exps = [_expected_range(sh, sv, sr, ms, M, what) for ms in (neg, mix)]
        n_vis = sh.n if vis is None else int(vis.sum())
        if n_vis >= M + 2:
            assert made.all(), (what, "a threshold kind could not be made", made.tolist())
            more = [j for j in range(N_PLANTED) if KINDS[j % 8] == "more"]
            exact = [j for j in range(N_PLANTED) if KINDS[j % 8] == "exact"]
            sp = [j for j in range(N_PLANTED) if KINDS[j % 8] == "spilled"]
            assert (exps[1].counts[more] == M + 1).all() and (exps[1].counts[exact] == M).all()
            ids_sp = exps[1].ids[sp]
            assert (exps[1].counts[sp] >= 1).all() and ((ids_sp >= LINE) | (ids_sp < 0)).all(), (what, "only spilled rows qualify")
            assert (exps[1].counts[[j for j in range(N_PLANTED) if KINDS[j % 8] in ("+inf", "nan")]] == 0).all()
        if mask in ("none", "ones", "rand50") and (shard == "B" or M == 1):
            beyond, below = _interleaves(exps[0].ids, min(M, 32))
            if M >= 8:
                assert (beyond >= 3).all() and (below >= 3).all(), (what, "the expected lists do not interleave the regions", beyond.tolist())
            else:
                assert (beyond[0::2] == 1).all() and (below[1::2] == 1).all(), what
        if mask in ("none", "rand50"):
            # the same definition over a reference that ignores the spilled groups
            head = torch.zeros(sh.n, dtype=torch.bool); head[:LINE] = True
            hv, hr = _sorted_visible(sh, head if vis is None else vis & head, M + 2 + SPARE)
            differ = (np.where(np.isfinite(hv[:, :M]), hr[:, :M], -1) != exps[0].ids).any(axis=1)
            assert differ[0::2].all() and (differ.all() or M == 1), (what, "a reference without the spilled groups gives the same list", differ.tolist())
    # the (M + 1)-th largest float64 group maximum, every row visible: over all groups and over the first 16 384
    G = _groups(sh.n)
    E = torch.nn.functional.pad(sh.e64, (0, G * GROUP - sh.n), value=-INF).view(N_PLANTED, G, GROUP).amax(dim=2)
    true_t = E.topk(M + 1, dim=1).values[:, -1]
    head_t = E[:, :LINE_G].topk(M + 1, dim=1).values[:, -1]
    if M <= 33:
        assert (head_t < true_t - 1e-3).all(), (shard, M, "the spilled groups do not move the (M + 1)-th largest group maximum")
    else:
        assert (head_t < true_t).all(), (shard, M)                       # (the planted spilled groups are among the M + 1 largest)


# ---- the grouped reference ---------------------------------------------------------------------------------------------------------------------
def _expected_grouped(sh, e_np, group_of, starts, vis, P, m, what, need_planted=True):
    """`_fold` of tests/test_gpu_grouped_search.py fed float64, one planted query at a time over the rows that can matter (its 256 best
    visible rows and the whole runs of the first P + 1 papers among them), at (P + 1, m + 1) so that the gaps behind the last paper and
    the last chunk are known -> papers G [32, P], local rows I [32, P, m] (-1 padding) and what float64 decides: `paper_ok` [32, P],
    `chunk_ok` [32, P, m] (a chunk only inside a decided paper).  Fixture error: an undecided paper whose best chunk is a planted row."""
    nq = e_np.shape[0]
    top = 256 if sh.n > 4096 else sh.n
    if sh.n > 4096:
        _, sr = _sorted_visible(sh, vis, top)
    else:
        sr = np.tile(np.arange(sh.n), (nq, 1))
    vis_np = np.ones(sh.n, bool) if vis is None else vis.cpu().numpy()
    G = np.full((nq, P + 1), -1, np.int64); I = np.full((nq, P + 1, m + 1), -1, np.int64); V = np.full((nq, P + 1, m + 1), -INF)
    for q in range(nq):
        rows = sr[q][sr[q] >= 0]
        runs = np.searchsorted(starts, rows, side="right") - 1
        _, first = np.unique(runs, return_index=True)
        papers = runs[np.sort(first)][:P + 1]
        assert papers.size == P + 1 or sh.n <= 4096 or (sr[q] < 0).any(), (what, "fixture: fewer than P + 1 papers among the best rows", papers.size)
        sub = np.zeros(sh.n, bool)
        sub[rows] = True
        for r in papers:
            sub[starts[r]:starts[r + 1]] = True
        _, i1, g1 = _fold(e_np[q:q + 1], group_of, sub & vis_np, P + 1, m + 1, 0)
        G[q], I[q] = g1[0], i1[0]
        V[q] = np.where(i1[0] >= 0, e_np[q][np.maximum(i1[0], 0)], -INF)
    tol = sh.tol[:nq, None]
    with np.errstate(invalid="ignore"):
        pv = V[:, :, 0]
        pgap = (pv[:, :-1] - pv[:, 1:] > tol) | (pv[:, 1:] == -INF)                      # [nq, P]
        cgap = (V[:, :, :-1] - V[:, :, 1:] > tol[:, :, None]) | (V[:, :, 1:] == -INF)   # [nq, P + 1, m]
    paper_ok = np.concatenate([np.ones((nq, 1), bool), pgap[:, :-1]], axis=1) & pgap
    chunk_ok = (np.concatenate([np.ones((nq, P + 1, 1), bool), cgap[:, :, :-1]], axis=2) & cgap)[:, :P] & paper_ok[:, :, None]
    if need_planted:
        best_planted = np.stack([np.isin(I[j, :P, 0], sh.rows[j]) for j in range(nq)])
        assert paper_ok[best_planted].all(), (what, "fixture: float64 does not decide the place of a planted paper")
    return SimpleNamespace(G=G[:, :P], I=I[:, :P, :m], V=V[:, :P, :m], paper_ok=paper_ok, chunk_ok=chunk_ok)


@functools.lru_cache(maxsize=None)
def _e_numpy(name, device):
    return _ref(name, device).e64.cpu().numpy()


@pytest.mark.parametrize("shard", ["A", "B"])
def test_grouped_fixtures_by_fp64_alone(shard):
    """CPU only, the reference alone.  For every grouped case of the shard and every mask: float64 decides every paper whose best chunk
    is planted (`_expected_grouped` raises otherwise) and at least nine in ten of all listed chunks; the selected papers lie on both
    sides of 2^20; in the straddling layout the best paper of every planted query is the run 2^20 - 100 ... 2^20 + 99, and with its
    best chunk hidden the same paper is decided by its chunk on the OTHER side of 2^20.  The cases bite: without the groups from
    16 384 on the fold names other papers for every planted query (P >= 10), and the K-th largest group maximum over the first 16 384
    groups alone differs from the true one."""
    sh = _ref(shard, "cpu")
    e_np = _e_numpy(shard, "cpu")
    G_ = _groups(sh.n)
    E = torch.nn.functional.pad(sh.e64, (0, G_ * GROUP - sh.n), value=-INF).view(N_PLANTED, G_, GROUP).amax(dim=2)
    head = torch.zeros(sh.n, dtype=torch.bool); head[:LINE] = True
    for s_, name, P, m, R in GROUPED_CASES:
        if s_ != shard:
            continue
        group_of, starts = _layout(name, sh.n)
        straddle = int(np.searchsorted(starts, LINE, side="right") - 1)
        plain = None
        for mask in GROUPED_MASKS:
            what = (shard, name, P, m, mask)
            vis = _mask(sh, mask)
            x = _expected_grouped(sh, e_np, group_of, starts, vis, P, m, what)
            assert x.chunk_ok[x.I >= 0].mean() >= 0.9, (what, "float64 decides too few chunks", float(x.chunk_ok.mean()))
            beyond = (x.I[:, :, 0] >= LINE).sum(1)
            if mask == "none" and P >= 10 and shard == "B":
                assert (beyond >= 3).all() and (P - beyond >= 3).all(), (what, "the papers do not interleave the regions", beyond.tolist())
            if mask == "beyond":
                assert (x.I[x.I >= 0] >= LINE).all()
            if name == "runs-200-straddle":
                if mask == "none":
                    plain = x
                    assert (x.G[:, 0] == 3 * straddle + 5).all(), (what, "the straddling run is not every planted query's best paper")
                if mask == "best-hidden":
                    assert (x.G[:, 0] == plain.G[:, 0]).all() and ((x.I[:, 0, 0] >= LINE) != (plain.I[:, 0, 0] >= LINE)).all(), what
                    assert (x.I[:, 0, 0] == sh.rows[:, 1]).all()
            if mask == "none" and P >= 10:
                y = _expected_grouped(sh, e_np, group_of, starts, head, P, m, what, need_planted=False)
                assert (y.G != x.G).any(axis=1).all(), (what, "a reference without the spilled groups names the same papers")
        if R is None and P >= 10 and shard == "B":
            K = GROUPED_K[(name, P)]
            true_t = E.topk(K, dim=1).values[:, -1]
            head_t = E[:, :LINE_G].topk(K, dim=1).values[:, -1]
            assert (head_t < true_t).all(), (shard, name, P, "the spilled groups do not move the K-th largest group maximum")


# ---- the GPU side -------------------------------------------------------------------------------------------------------------------------------
def _pack(vis):
    """bool [n] (device) -> int64 words (device); the last word's bits beyond n are SET"""
    from tests.test_gpu_filtered_search import _pack as pack
    return pack(vis, garbage=True)


def _rows_bitmap(rows, n):
    """the bitmap of a few rows (numpy int64) -> int64 words on the device"""
    w = np.zeros(_groups(n), np.uint64)
    np.bitwise_or.at(w, rows >> 6, np.uint64(1) << (rows & 63).astype(np.uint64))
    return torch.from_numpy(w.view(np.int64)).cuda()


def _assert_search_gives_the_same_bits(idx, q1, loc, bits, n, base, what):
    """`loc` (local rows, numpy) with the f32 score bits `bits`, in the order of an answer of ONE query q1: `search(q1, 32, allow=bitmap of
    the rows)`, 32 rows at a time, returns the same rows with the same bits in the same order."""
    for a in range(0, loc.shape[0], 32):
        r = loc[a:a + 32]
        s, i = idx.search(q1, 32, allow=_rows_bitmap(r, n), n_allowed=int(r.shape[0]))
        s, i = s[0].cpu().numpy(), i[0].cpu().numpy()
        assert np.array_equal(i[:r.shape[0]], r + base) and (i[r.shape[0]:] == -1).all(), (what, "rows", a)
        assert np.array_equal(s[:r.shape[0]].view(np.int32), bits[a:a + 32]), (what, "score bits differ from search()", a)


def _same3(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def _worst_over_budget(sh, s, loc, nq):
    """max |s - float64| / (B |q| |c|) over the returned (query, row) pairs (loc: local rows, < 0 = none; device tensors)"""
    valid = loc >= 0
    if not valid.any():
        return 0.0
    flat = loc.clamp(min=0).reshape(nq, -1)
    ej = sh.e64[:nq].gather(1, flat).reshape(loc.shape)
    qn = sh.Q[:nq].double().norm(dim=1).reshape((nq,) + (1,) * (loc.dim() - 1))
    cn = sh.C[flat.flatten()].double().norm(dim=1).reshape(loc.shape)
    return float(((s.double() - ej).abs() / (pass_b_budget(DIM) * qn * cn))[valid].max())


@pytest.fixture(scope="module")
def shards():
    """name -> the shard on the device with its indexes (built on first use, left unchanged, freed with the module)"""
    from arxiv_rag_amd.index import ShardIndex
    built = {}

    def get(name):
        if name not in built:
            sh = _ref(name, "cuda")
            sh.idx = ShardIndex(sh.C, idx_base=RANGE_BASE[name])
            sh.grouped = {}
            built[name] = sh
        return built[name]
    torch.cuda.reset_peak_memory_stats()
    yield get
    print(f"\nlarge shards: peak device memory of the tests that used them {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    for key in [k for k in _REFS if k[1] == "cuda"]:
        del _REFS[key]
    built.clear()
    torch.cuda.empty_cache()


# ---- 2. search_range over the line -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shard,M", RANGE_PARAMS, ids=[f"{s}-M{M}" for s, M in RANGE_PARAMS])
def test_range_search_beyond_2_20_rows_is_the_fp64_definition_on_every_path(hip, shards, shard, M):
    """Per mask and per threshold vector (all -inf; spilled-only / +inf / more than M / NaN / exactly M / -inf across the batch), over the
    32 planted queries: counts and padding are the float64 definition's, ids equal it wherever float64 decides (every planted row), the
    whole answer passes check_range_fp64; the scan, the exhaustive path and the scan with a one-entry candidate list return the bits of
    the library's choice; sampled queries' scores are the bits `search` gives the returned rows.  ksel = M + 1 in tail_kth_key."""
    sh = shards(shard)
    idx, n, base = sh.idx, sh.n, RANGE_BASE[shard]
    Q_ = sh.Q[:N_PLANTED].contiguous()
    col = np.arange(M)[None, :]
    for mask in RANGE_MASKS[shard]:
        vis, sv, sr, vectors, made = _range_case(sh, mask, M)
        allow = None if vis is None else _pack(vis)
        words = None if vis is None else allow.cpu().numpy().view(np.uint64)
        n_vis = n if vis is None else int(vis.sum())
        groups_seen = _groups(n) if vis is None else int(torch.nn.functional.pad(vis, (0, _groups(n) * GROUP - n)).view(-1, GROUP).any(1).sum())
        for name, ms in zip(("-inf", "mix"), vectors):
            what = (shard, M, mask, name)
            x = _expected_range(sh, sv, sr, ms, M, what)
            got = idx.search_range(Q_, ms, M, allow=allow)
            over, _ = idx.range_stats()
            s, i, cnt = (t.cpu().numpy() for t in got)
            assert np.array_equal(cnt, x.counts), (what, "counts", cnt.tolist(), x.counts.tolist())
            held = col < np.minimum(cnt, M)[:, None]
            assert np.array_equal(i >= 0, held) and (i[~held] == -1).all() and np.isneginf(s[~held]).all(), (what, "padding")
            loc = np.where(held, i - base, -1)
            assert np.array_equal(loc[x.decided], x.ids[x.decided]), (what, "ids differ from the float64 definition", np.argwhere((loc != x.ids) & x.decided)[:4].tolist())
            check_range_fp64(sh.C, Q_, sh.e64, words, ms, M, got[0], got[1], got[2], base, what)
            worst = _worst_over_budget(sh, got[0], torch.from_numpy(loc).cuda(), N_PLANTED)
            stats = {}
            for pname, kw in (("scan", dict(path=1)), ("exhaustive", dict(path=2)), ("cap1", dict(path=1, cand_cap=1))):
                other = idx.search_range(Q_, torch.from_numpy(ms).cuda(), M, allow=allow, **kw)
                stats[pname] = idx.range_stats()
                assert _same3(other, got), (what, pname, "not the bits of the library's choice")
            live = int((ms < INF).sum())
            spread = sum(len(set((x.ids[j][x.ids[j] >= 0] >> 6).tolist())) >= 2 for j in range(N_PLANTED))
            assert over == 0 and stats["scan"][0] == 0 and stats["exhaustive"] == (0, 0), (what, stats)
            assert spread <= stats["cap1"][0] <= (live if groups_seen >= 2 else 0), (what, "fallback counter", stats, spread, live)
            if name == "-inf" and groups_seen >= 2:
                assert stats["cap1"][0] == N_PLANTED and stats["scan"][1] >= N_PLANTED * min(M + 1, groups_seen), (what, stats)
            for j in ((0, 1, 5, 18) if M <= 33 else (0, 5)):
                r = loc[j][loc[j] >= 0]
                _assert_search_gives_the_same_bits(idx, Q_[j:j + 1], r, s[j, :r.shape[0]].view(np.int32), n, base, (what, j))
            print(f"range {shard}-M{M}-{mask}-{name}: allowed {n_vis} of {n} rows in {groups_seen} groups; overflowed queries {over}; candidate "
                  f"groups per query {stats['scan'][1] / max(live, 1):.2f}; one-entry list: overflowed {stats['cap1'][0]} of {live}; positions "
                  f"float64 decides {int(x.decided[held].sum())} of {int(held.sum())}; worst error / budget {worst:.3f}")


@gpu
@pytest.mark.parametrize("shard,M", [("B", 33), ("A", 1024)])
def test_range_query_gets_the_same_bits_alone_and_in_a_batch_of_two_slices(hip, shards, shard, M):
    """1 025 queries (two internal slices of the call; idx_base = 1 << 33 on B) under a random half of the rows and every kind of
    threshold: queries 0, 5, 31 and the one of the second slice have the bits of a batch of 1."""
    sh = shards(shard)
    vis, sv, sr, (_, mix), _ = _range_case(sh, "rand50", M)
    allow = _pack(vis)
    ms = np.resize(mix, NQ_ALL).astype(np.float32)
    ms[NQ_ALL - 1] = 0.25
    whole = sh.idx.search_range(sh.Q, ms, M, allow=allow)
    assert sh.idx.range_stats()[0] == 0
    for j in (0, 5, 31, NQ_ALL - 1):
        alone = sh.idx.search_range(sh.Q[j:j + 1].contiguous(), float(ms[j]), M, allow=allow)
        assert _same3(alone, tuple(t[j:j + 1] for t in whole)), (shard, M, j)
    x = _expected_range(sh, sv, sr, mix, M, (shard, M, "batch"))
    loc = np.where(whole[1][:N_PLANTED].cpu().numpy() >= 0, whole[1][:N_PLANTED].cpu().numpy() - RANGE_BASE[shard], -1)
    assert np.array_equal(whole[2][:N_PLANTED].cpu().numpy(), x.counts) and np.array_equal(loc[x.decided], x.ids[x.decided])
    assert 0 < int(whole[2][NQ_ALL - 1]) <= M + 1


# ---- 3. search_grouped over the line --------------------------------------------------------------------------------------------------------------------
def _grouped_index(sh, layout):
    from arxiv_rag_amd.index import ShardIndex
    if layout not in sh.grouped:
        group_of, starts = _layout(layout, sh.n)
        sh.grouped[layout] = (ShardIndex(sh.C, idx_base=BASE).set_groups(group_of), group_of, starts)
    return sh.grouped[layout]


def _assert_grouped_is_fp64(got, x, what):
    """papers, chunk ids and padding of `got` against the float64 fold `x`, wherever float64 decides"""
    s, i, g = (t.cpu().numpy() for t in got)
    assert np.array_equal(g[x.paper_ok], (x.G[x.paper_ok]).astype(np.int32)), (what, "papers differ from the float64 fold")
    loc = np.where(i >= 0, i - BASE, -1)
    assert np.array_equal(loc[x.chunk_ok], x.I[x.chunk_ok]), (what, "chunks differ from the float64 fold", np.argwhere((loc != x.I) & x.chunk_ok)[:4].tolist())
    assert np.array_equal((i >= 0)[x.paper_ok], (x.I >= 0)[x.paper_ok]) and np.isneginf(s[i < 0]).all() and np.array_equal(g >= 0, x.G >= 0), (what, "padding")
    return s, loc


@gpu
@pytest.mark.parametrize("case", GROUPED_CASES, ids=[f"{c[0]}-{c[1]}-P{c[2]}-m{c[3]}" + (f"-R{c[4]}" if c[4] else "") for c in GROUPED_CASES])
def test_grouped_search_beyond_2_20_rows_is_the_fp64_fold_on_every_path(hip, shards, case):
    """Per mask (none; only rows >= 2^20; the best chunk of every planted query hidden), over the 32 planted queries: papers, chunk ids
    and padding equal `_fold` fed float64 wherever float64 decides (every planted paper), every score lies within the pass-B budget, the
    scan, the exhaustive path and the scan with a one-entry candidate list return the bits of the library's choice, and sampled queries'
    scores are the bits `search` gives the returned rows.  ksel = K = P S in tail_kth_key; max_run_rows = 1 000 makes K = 544 and the
    whole call exhaustive.  `arx_group_runs_info` (through set_groups) equals numpy on the layout."""
    shard, layout, P, m, R = case
    sh = shards(shard)
    idx, group_of, starts = _grouped_index(sh, layout)
    assert (idx.n_runs, idx.max_run_rows) == (starts.shape[0] - 1, int(np.diff(starts).max())), (case, "arx_group_runs_info")
    K = _select_count(P, R or idx.max_run_rows)
    scan = K <= KSEL_MAX
    assert scan == (R is None) and (R is not None or K == GROUPED_K[(layout, P)])
    Q_ = sh.Q[:N_PLANTED].contiguous()
    e_np = _e_numpy(shard, "cuda")
    kw0 = {} if R is None else dict(max_run_rows=R)
    for mask in GROUPED_MASKS:
        what = case + (mask,)
        vis = _mask(sh, mask)
        allow = None if vis is None else _pack(vis)
        groups_seen = _groups(sh.n) if vis is None else int(torch.nn.functional.pad(vis, (0, _groups(sh.n) * GROUP - sh.n)).view(-1, GROUP).any(1).sum())
        x = _expected_grouped(sh, e_np, group_of, starts, vis, P, m, what)
        got = idx.search_grouped(Q_, P, m, allow=allow, **kw0)
        over, cands = idx.grouped_stats()
        s, loc = _assert_grouped_is_fp64(got, x, what)
        _grouped_check_fp64(sh.C, Q_, got, what)
        worst = _worst_over_budget(sh, got[0], torch.from_numpy(loc).cuda(), N_PLANTED)
        stats = {}
        for pname, kw in (("scan", dict(path=1)), ("exhaustive", dict(path=2)), ("cap1", dict(path=1, cand_cap=1))):
            other = idx.search_grouped(Q_, P, m, allow=allow, **kw, **kw0)
            stats[pname] = idx.grouped_stats()
            assert _same3(other, got), (what, pname, "not the bits of the library's choice")
        assert over == 0 and (cands > 0) == scan and stats["exhaustive"] == (0, 0), (what, over, cands, stats)
        if scan:
            assert stats["scan"] == (over, cands) and cands >= N_PLANTED * min(K, groups_seen), (what, stats)
            assert stats["cap1"][0] == N_PLANTED, (what, "every query has min(K, non-empty groups) >= 2 candidate groups", stats)
        else:
            assert stats["scan"] == (0, 0) and stats["cap1"] == (0, 0), (what, "K > GRP_KSEL_MAX: no candidate group is listed", stats)
        for j in (0, 5, 18):
            r = loc[j].reshape(-1)
            keep = r >= 0
            order = np.lexsort((r[keep], -s[j].reshape(-1)[keep].astype(np.float64)))      # search's order: score desc, row asc
            _assert_search_gives_the_same_bits(idx, Q_[j:j + 1], r[keep][order], s[j].reshape(-1)[keep][order].view(np.int32), sh.n, BASE, (what, j))
        print(f"grouped {shard}-{layout}-P{P}-m{m}{'-R' + str(R) if R else ''}-{mask}: K {K}; allowed {sh.n if vis is None else int(vis.sum())} of "
              f"{sh.n} rows in {groups_seen} groups; overflowed queries {over}; candidate groups per query {cands / N_PLANTED:.2f}; one-entry list: "
              f"overflowed {stats['cap1'][0]} of {N_PLANTED}; float64 decides {int(x.paper_ok.sum())} of {x.paper_ok.size} papers, "
              f"{int(x.chunk_ok[x.I >= 0].sum())} of {int((x.I >= 0).sum())} chunks; worst error / budget {worst:.3f}")


# ---- 4. large dims, small shards --------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", LARGE_DIMS)
def test_range_and_grouped_search_at_large_dims_with_the_default_and_the_largest_candidate_list(hip, d):
    """329 rows of mixed norms at dims 1536 / 4096 / 8192, 8 queries of every family, every row and a random half: both searches with the default
    cand_cap and with FILT_CAND_CAP_MAX, so that every raise-the-limit cell of the CPU test runs (range tail: above 32 KiB at dim 8192
    with M = 1 024 by default, at every dim with the largest list - 69 720 B of LDS in all at dim 8192; grouped tail: above 48 KiB at
    dim 8192 with the largest list).  Range (M = 10, 1 024; -inf and mixed thresholds): check_range_fp64, every path the same bits,
    and `search(Q, 10, allow)` bit for bit at M = 10 and -inf.  Grouped ((3, 2), (32, 8); runs of 1 ... 7): `_fold` fed float64 where
    float64 decides, the pass-B budget, every path the same bits."""
    from arxiv_rag_amd.index import ShardIndex
    from tests.test_gpu_search_fp64 import _case_data
    C_, Q_ = _case_data(dict(id=f"range-grouped-large-{d}", d=d, n=LARGE_N, nq=58, rows="mixed"))
    Q_ = Q_[[0, 1, 2, 41, 42, 51, 52, 53]].contiguous()              # the zero query, two rounding-adversarial, two tiny, three unit (one of norm 8)
    n, nq = LARGE_N, 8
    group_of, starts = _layout("runs-1-7", n)
    idx = ShardIndex(C_, idx_base=BASE).set_groups(group_of)
    e = scores_fp64(Q_, C_)
    e_np = e.cpu().numpy()
    tol = (2 * pass_b_budget(d) * (1 + 1e-3) * Q_.double().norm(dim=1) * C_.double().norm(dim=1).max()).cpu().numpy()
    small = SimpleNamespace(n=n, tol=tol, rows=np.zeros((nq, 0), np.int64))
    rs = np.random.RandomState(d)
    for mask in ("none", "rand50"):
        vis = None if mask == "none" else torch.from_numpy(rs.rand(n) < 0.5).cuda()
        allow = None if vis is None else _pack(vis)
        words = None if vis is None else allow.cpu().numpy().view(np.uint64)
        n_vis = n if vis is None else int(vis.sum())
        for M in LARGE_RANGE_MS:
            top = e.masked_fill(~vis[None, :], -INF).topk(5, dim=1).values[:, -1] if vis is not None else e.topk(5, dim=1).values[:, -1]
            mixed = np.array([(-INF, float(top[j]), INF, np.nan, 0.0, -INF, float(top[j]), 0.03125)[j] for j in range(nq)], np.float32)
            for tname, ms in (("-inf", np.full(nq, -INF, np.float32)), ("mix", mixed)):
                what = (d, mask, M, tname)
                got = idx.search_range(Q_, ms, M, allow=allow)
                check_range_fp64(C_, Q_, e, words, ms, M, got[0], got[1], got[2], BASE, what)
                stats = {}
                for pname, kw in (("scan", dict(path=1)), ("cap-max", dict(path=1, cand_cap=CAP_MAX)), ("exhaustive", dict(path=2)),
                                  ("cap1", dict(path=1, cand_cap=1))):
                    assert _same3(idx.search_range(Q_, ms, M, allow=allow, **kw), got), (what, pname)
                    stats[pname] = idx.range_stats()
                assert stats["scan"][0] == 0 and stats["cap-max"] == stats["scan"] and stats["exhaustive"] == (0, 0), (what, stats)
                if tname == "-inf":
                    assert (got[2] == min(M + 1, n_vis)).all() and stats["cap1"][0] == nq, (what, stats)
                    if M <= KMAX:
                        ts, ti = idx.search(Q_, M, allow=allow if allow is not None else _pack(torch.ones(n, dtype=torch.bool, device="cuda")))
                        assert torch.equal(ti, got[1]) and torch.equal(ts.view(torch.int32), got[0].view(torch.int32)), (what, "not search(Q, M, allow)")
                print(f"range dim {d}-{mask}-M{M}-{tname}: allowed {n_vis} of {n}; dynamic LDS of the tail {_tail_dyn(d, _range_cand_cap(M))} B by default, "
                      f"{_tail_dyn(d, CAP_MAX)} B with the largest list; (overflowed queries, candidate groups) = {stats}")
        for P, m in LARGE_GROUPED:
            what = (d, mask, P, m)
            x = _expected_grouped(small, e_np, group_of, starts, vis, P, m, what, need_planted=False)
            got = idx.search_grouped(Q_, P, m, allow=allow)
            _assert_grouped_is_fp64(got, x, what)
            _grouped_check_fp64(C_, Q_, got, what)
            stats = {}
            for pname, kw in (("scan", dict(path=1)), ("cap-max", dict(path=1, cand_cap=CAP_MAX)), ("exhaustive", dict(path=2)),
                              ("cap1", dict(path=1, cand_cap=1))):
                assert _same3(idx.search_grouped(Q_, P, m, allow=allow, **kw), got), (what, pname)
                stats[pname] = idx.grouped_stats()
            assert stats["scan"][0] == 0 and stats["cap-max"] == stats["scan"] and stats["exhaustive"] == (0, 0) and stats["cap1"][0] == nq, (what, stats)
            assert x.paper_ok[5:].any(axis=1).all(), (what, "float64 decides no paper of a unit query: the comparison means nothing")
            print(f"grouped dim {d}-{mask}-P{P}-m{m}: dynamic LDS of the tail {_tail_dyn(d, CAP_DEFAULT)} B by default, {_tail_dyn(d, CAP_MAX)} B with the "
                  f"largest list; float64 decides {int(x.paper_ok.sum())} of {x.paper_ok.size} papers; (overflowed queries, candidate groups) = {stats}")
