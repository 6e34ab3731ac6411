"""The masked exact top-k searches (csrc/masked_topk.h: `ShardIndex.search(allow=...)`, `search_prefix`, `nearest_earlier`) where the other
masked suites stop: shards of more than FILT_REG_GROUPS * FILT_TAIL_NT = 16 384 groups (2^20 rows), whose further group maxima the tail
kernel re-reads from memory in two loops of their own (the bit-by-bit search for the k-th largest group maximum, and the candidate pass),
and dims 1536 / 4096 / 8192, up to the dynamic-LDS size at which the host raises the tail kernel's limit.

Every reference is float64 (tests/helpers.py: check_topk_fp64 with the certificate's own budgets) or an independent path of the library
(the unfiltered search of the compacted rows, the filtered search of a prefix bitmap); the masked scan is never compared with itself alone.

Two shards of dim 64, built once per module from seeded unit rows:
  A  N_A = 64 * 16384 + 64 * 3 + 5 rows: four spilled groups (16384 ... 16387), the last ragged; only lanes 0 ... 3 of wave 0 work in the
     spill loops
  B  N_B = 256 * 4369 rows: 17 476 groups, 1 092 spilled; every wave takes one spill iteration, waves 0 and 1 a second (68 groups, wave
     1's partial); a multiple of 256, so a roll by 2^20 rows keeps every row's place inside its 256-row tile
By chance about 7 % of a unit query's top-10 lie beyond row 2^20, so rows are PLANTED: for each of the first 32 queries q, 64 rows
a q + sqrt(1 - a^2) noise (noise unit and orthogonal to q) with a from 0.95 down to 0.70, in 64 distinct groups, the ranks alternating
between the spilled groups and the first 16 384 (B: 32 and 32, with groups 16383, 16384 and the shard's last among them; A has only four
spilled groups, of which the last holds five rows: three spilled rows per query, a fourth for queries 0 ... 4).  Chance rows stay below
0.125 * sqrt(2 ln N) = 0.66, so a planted query's exact top-k interleaves both regions; the tests assert that from the float64 scores
before they trust a result.

Figures printed (profiles/masked_search_large_fp64.md): allowed rows, overflowed queries and candidate groups per query of every case."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import U24, allow_below, check_against_filtered_and_fp64, check_prefix_answer, pass_a_budget, scores_fp64
from tests.test_gpu_filtered_search import BASE, _bits_equal, _check_fp64, _pack, hip  # noqa: F401  (`hip`: the module's fixture)
from tests.test_gpu_search_fp64 import _case_data, _gen, _unit

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

# ---- the constants the shapes below are derived from, read from the sources: if one changes, test_the_fixtures_cross_the_lines fails
CSRC = Path(__file__).resolve().parents[1] / "arxiv_rag_amd" / "csrc"


def _define(header, name):
    m = re.search(rf"^#define\s+{name}\s+(\d+)\b", (CSRC / header).read_text(), re.M)
    assert m, f"{header} no longer defines {name}"
    return int(m.group(1))


TAIL_NT = _define("masked_topk.h", "FILT_TAIL_NT")                # threads of a tail block
REG_GROUPS = _define("masked_topk.h", "FILT_REG_GROUPS")          # group maxima a tail thread keeps in registers
CAP_DEFAULT = _define("masked_topk.h", "FILT_CAND_CAP_DEFAULT")
CAP_MAX = _define("masked_topk.h", "FILT_CAND_CAP_MAX")
GROUP = _define("search_consts.h", "GROUP_ROWS")
LINE_G = REG_GROUPS * TAIL_NT                                     # groups held in registers: the first spilled group
LINE = LINE_G * GROUP                                             # = 2^20: the first row of a spilled group
N_A = GROUP * LINE_G + GROUP * 3 + 5
N_B = 256 * 4369
DIM = 64
N_PLANTED, PLANTED_ROWS, NQ_ALL = 32, 64, 300
# limits of the prefix batch: the spill loops' bounds at 0 groups (2^20 - 65 ... 2^20), 1 (2^20 + 1 ... + 64), 2 (+ 65), 1 024 and 1 025
# (every wave one whole iteration / wave 0 a second), the shard's end and beyond; and, not in that list, 63 / 64 / 65 spilled groups (a
# wave's last lane, the next wave's first)
LISTED_LIMITS = [0, 1, 64, LINE - 65, LINE - 1, LINE, LINE + 1, LINE + 63, LINE + 64, LINE + 65, LINE + TAIL_NT * GROUP,
                 LINE + TAIL_NT * GROUP + 1, N_B - 1, N_B, N_B + 5, 1 << 40]
EXTRA_LIMITS = [LINE + 62 * GROUP + 1, LINE + 64 * GROUP, LINE + 64 * GROUP + 1]
# exact copies planted in B for the self-join: row -> the row it copies (rows 5 and 2^20 + 7 are ordinary unit rows)
COPIES = {LINE + 2 * GROUP + 50: 5, LINE + 2 * GROUP + 55: LINE + 7, N_B - 2 * GROUP + 50: LINE + 7, N_B - GROUP + 50: 5}


def _tail_lds_bytes(dim, cand_cap):
    """dynamic LDS of masked_tail_kernel (masked_search_impl): the query row, one 64-score stretch per wave, the candidate list"""
    return ((dim * 2 + 15) & ~15) + (TAIL_NT // 64) * GROUP * 4 + cand_cap * 4


def test_the_fixtures_cross_the_lines():
    """CPU only: the arithmetic the GPU tests of this file rely on, from the constants of the sources."""
    assert (TAIL_NT, REG_GROUPS, GROUP, CAP_DEFAULT, CAP_MAX) == (1024, 16, 64, 1024, 8192)
    assert LINE_G == 16384 and LINE == 1 << 20
    assert N_A == 1048773 and N_B == 1118464 and N_B % 256 == 0 and N_B > LINE and (N_B - LINE) % 256 == 0
    groups = lambda n: (n + GROUP - 1) // GROUP
    assert groups(N_A) - LINE_G == 4 and N_A % GROUP == 5                      # four spilled groups, the last ragged
    assert groups(N_B) == 17476 and groups(N_B) - LINE_G == 1092
    # the spill loops of wave w start at group LINE_G + 64 w and advance by TAIL_NT groups
    iters = lambda n, w: len(range(LINE_G + 64 * w, groups(n), TAIL_NT))
    assert [iters(N_A, w) for w in range(TAIL_NT // 64)] == [1] + [0] * 15
    assert [iters(N_B, w) for w in range(TAIL_NT // 64)] == [2, 2] + [1] * 14
    second = groups(N_B) - LINE_G - TAIL_NT
    assert second == 68 and second - 64 == 4                                   # wave 0 whole, wave 1 four lanes
    # the prefix batch: spilled groups per listed limit (a limit is clamped to the shard)
    spilled = lambda lim: max(0, groups(min(max(lim, 0), N_B)) - LINE_G)
    assert [spilled(v) for v in LISTED_LIMITS] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 1024, 1025, 1092, 1092, 1092, 1092]
    assert [spilled(v) for v in EXTRA_LIMITS] == [63, 64, 65]
    assert len(LISTED_LIMITS) + len(EXTRA_LIMITS) <= 24
    # planted rows sit at offset 16 + query of their group (A's ragged last group: at offset query, queries 0 ... 4); the copies elsewhere
    for row, src in COPIES.items():
        assert row > LINE + 100 and src < row < N_B and row % GROUP >= 16 + N_PLANTED and src % GROUP < 16
    assert LINE - 3 < LINE + 7 < min(COPIES) and max(r for r in COPIES if r < LINE + 200) < LINE + 200
    assert sorted(r for r in COPIES if r >= N_B - 130) == [N_B - 2 * GROUP + 50, N_B - GROUP + 50]
    # dynamic LDS of the tail: above 48 KB (the host then raises the kernel's limit) from dim 6208 on with the largest candidate list
    assert _tail_lds_bytes(8192, CAP_MAX) == 16384 + 4096 + 32768 == 53248 > 48 * 1024
    assert min(d for d in range(64, 8193, 64) if _tail_lds_bytes(d, CAP_MAX) > 48 * 1024) == 6208
    assert _tail_lds_bytes(8192, CAP_DEFAULT) < 48 * 1024 and _tail_lds_bytes(64, CAP_MAX) < 48 * 1024


# ---- 6. large dims (first in the file: the two large shards below are built after these cases have freed their tensors) -----------------------------------------------------------------------------------------------------------------------------
# d x nq x k an orthogonal array; `ties` (n = 64 * 130 + 37) and `mixed` (n = 256 * 5 + 1) meet every d, nq and k
N_TIES, N_MIXED = 64 * 130 + 37, 256 * 5 + 1
LARGE_DIM_CASES = [
    dict(id="masked-1536-ties-7q-k1", d=1536, n=N_TIES, nq=7, k=1, rows="ties"),
    dict(id="masked-1536-mixed-70q-k10", d=1536, n=N_MIXED, nq=70, k=10, rows="mixed"),
    dict(id="masked-1536-ties-257q-k32", d=1536, n=N_TIES, nq=257, k=32, rows="ties"),
    dict(id="masked-4096-mixed-7q-k10", d=4096, n=N_MIXED, nq=7, k=10, rows="mixed"),
    dict(id="masked-4096-ties-70q-k32", d=4096, n=N_TIES, nq=70, k=32, rows="ties"),
    dict(id="masked-4096-mixed-257q-k1", d=4096, n=N_MIXED, nq=257, k=1, rows="mixed"),
    dict(id="masked-8192-mixed-7q-k32", d=8192, n=N_MIXED, nq=7, k=32, rows="mixed"),
    dict(id="masked-8192-ties-70q-k1", d=8192, n=N_TIES, nq=70, k=1, rows="ties"),
    dict(id="masked-8192-ties-257q-k10", d=8192, n=N_TIES, nq=257, k=10, rows="ties"),
]


@gpu
@pytest.mark.parametrize("case", LARGE_DIM_CASES, ids=[c["id"] for c in LARGE_DIM_CASES])
def test_masked_searches_at_large_dims_every_path_and_fp64(hip, case):
    """Both policies at dims 1536 / 4096 / 8192 on near-tied and mixed-norm rows: bitmap masks `rand50` and `garbage` (every row, the last
    word's spare bits set), prefix limits `random` and `self` (300 rows of the shard, the first and the last, each against its earlier
    rows).  The four paths return the same bits, held to float64 and to the independent path as in the other masked suites.  At dim
    8192 also with the largest candidate list, cand_cap = 8192: 53 248 B of dynamic LDS, above the 48 KB a kernel gets without asking."""
    from arxiv_rag_amd.index import ShardIndex
    c = case
    C_, Q_ = _case_data(c)
    n, d, k, nq = C_.shape[0], c["d"], c["k"], c["nq"]
    assert (n, Q_.shape[0]) == (c["n"], nq)
    idx = ShardIndex(C_, idx_base=BASE)
    big_list = (("cap-max", dict(path=1, cand_cap=CAP_MAX)),) if d == 8192 else ()
    if big_list:
        assert _tail_lds_bytes(d, CAP_MAX) > 48 * 1024
    g = _gen(c["d"] + 7 * nq + k)
    for mask in ("rand50", "garbage"):
        what = (c["id"], mask)
        m = torch.rand(n, generator=g, device="cuda") < 0.5 if mask == "rand50" else torch.ones(n, dtype=torch.bool, device="cuda")
        rows = torch.nonzero(m).flatten()
        allow = _pack(m, garbage=mask == "garbage")
        ref = idx.search(Q_, k, allow=allow, n_allowed=int(rows.shape[0]))
        _check_fp64(C_, Q_, ref[0], ref[1], rows, k, what)
        stats = _four_paths(lambda **kw: idx.search(Q_, k, allow=allow, **kw), idx.filtered_stats, ref, what, extra=big_list)
        print(f"{c['id']} {mask}: allowed {rows.shape[0]} of {n}; (overflowed queries, candidate groups) = {stats}")
        if big_list:
            assert stats["cap-max"][0] == 0 and stats["cap-max"] == stats["scan"], (what, stats)
        s2, i2 = ShardIndex(C_[rows].contiguous()).search(Q_, k)
        i2 = torch.where(i2 >= 0, rows[i2.clamp_min(0)] + BASE, i2)
        assert _bits_equal((s2, i2), ref), (what, "differs from the unfiltered search of the compacted rows")
        if mask == "garbage":
            assert _bits_equal(idx.search(Q_, k), ref), (what, "all-rows mask differs from the unfiltered search")
    rs = np.random.RandomState(d + nq)
    for kind in ("random", "self"):
        what = (c["id"], kind)
        if kind == "random":
            Qp, lim = Q_, rs.randint(0, n + 1, size=nq).astype(np.int64)
        else:
            lim = np.concatenate([np.arange(0, 130), np.arange(n - 170, n)]).astype(np.int64)
            Qp = C_[torch.from_numpy(lim).cuda()].contiguous()
        lim_d = torch.from_numpy(lim).cuda()
        ref = idx.search_prefix(Qp, lim_d, k)
        stats = _four_paths(lambda **kw: idx.search_prefix(Qp, lim_d, k, **kw), idx.prefix_stats, ref, what, extra=big_list)
        print(f"{c['id']} {kind}: (overflowed queries, candidate groups) = {stats}")
        if big_list:
            assert stats["cap-max"][0] == 0 and stats["cap-max"] == stats["scan"], (what, stats)
        if k >= 2:
            assert stats["cap1"][0] == int((lim > GROUP).sum()), (what, stats)
        check_prefix_answer(ref[0], ref[1], lim, k, BASE, what)
        pick = rs.choice(lim.shape[0], size=min(lim.shape[0], 8), replace=False).tolist()
        sample = list(dict.fromkeys(([0, 1, 64, 65, 129, 130, lim.shape[0] - 1] if kind == "self" else []) + pick))[:12]
        check_against_filtered_and_fp64(idx, C_, Qp, lim, ref[0], ref[1], k, sample, what)


# ---- the two shards ------------------------------------------------------------------------------------------------------------------------
def _planted_layout(n, seed):
    """rows [32, 64] and target scores [32, 64] of the planted rows: rank i of query j scores 0.95 - 0.25 i / 63 and lies in a spilled
    group when i + j is even (while the query has spilled groups left), else in one of the first LINE_G."""
    rs = np.random.RandomState(seed)
    n_groups = (n + GROUP - 1) // GROUP
    last = n_groups - 1
    rows = np.zeros((N_PLANTED, PLANTED_ROWS), np.int64)
    for j in range(N_PLANTED):
        if n_groups - LINE_G > PLANTED_ROWS // 2:
            sp = [LINE_G, last] + rs.choice(np.arange(LINE_G + 1, last), size=PLANTED_ROWS // 2 - 2, replace=False).tolist()
        else:
            sp = list(range(LINE_G, last)) + ([last] if j < n - last * GROUP else [])
        head = [LINE_G - 1] + rs.choice(np.arange(1, LINE_G - 1), size=PLANTED_ROWS - len(sp) - 1, replace=False).tolist()
        assert len(set(sp + head)) == PLANTED_ROWS
        for i in range(PLANTED_ROWS):
            g = sp.pop(0) if (sp and ((i + j) % 2 == 0 or not head)) else head.pop(0)
            r = g * GROUP + 16 + j
            rows[j, i] = r if r < n else g * GROUP + j
    assert rows.max() < n and np.unique(rows).shape[0] == rows.size
    a = np.broadcast_to(0.95 - 0.25 * np.arange(PLANTED_ROWS) / (PLANTED_ROWS - 1), rows.shape)
    return rows, a


def _build_shard(name):
    from arxiv_rag_amd.index import ShardIndex
    n = {"A": N_A, "B": N_B}[name]
    g = _gen({"A": 1101, "B": 1102}[name])
    C_ = _unit(n, DIM, g).half()
    Q_ = _unit(NQ_ALL, DIM, g).half().contiguous()
    rows, a = _planted_layout(n, n)
    qh = torch.nn.functional.normalize(Q_[:N_PLANTED].float(), dim=1)                       # [32, 64]
    noise = torch.randn((N_PLANTED, PLANTED_ROWS, DIM), generator=g, device="cuda")
    noise = noise - (noise * qh[:, None, :]).sum(2, keepdim=True) * qh[:, None, :]
    noise = torch.nn.functional.normalize(noise, dim=2)
    at = torch.from_numpy(np.ascontiguousarray(a)).cuda().float()[:, :, None]
    C_[torch.from_numpy(rows).cuda().flatten()] = (at * qh[:, None, :] + (1 - at * at).sqrt() * noise).half().view(-1, DIM)
    if name == "B":
        for row, src in COPIES.items():
            C_[row] = C_[src]
    C_ = C_.contiguous()
    planted = torch.zeros(n, dtype=torch.bool, device="cuda")
    planted[torch.from_numpy(rows).cuda().flatten()] = True
    return SimpleNamespace(name=name, n=n, C=C_, Q=Q_, idx=ShardIndex(C_, idx_base=BASE), e64=scores_fp64(Q_[:64], C_),
                           planted_rows=torch.from_numpy(rows).cuda(), planted=planted)


@pytest.fixture(scope="module")
def shards():
    """name -> the shard (built on first use, left unchanged, freed with the module): corpus, 300 queries (the first 32 planted), index,
    the float64 scores of the first 64 queries."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = _build_shard(name)
        return built[name]
    torch.cuda.reset_peak_memory_stats()
    yield get
    print(f"\nlarge shards: peak device memory of the tests that used them {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    built.clear()
    torch.cuda.empty_cache()


def _mask(kind, sh, seed=0):
    n = sh.n
    m = torch.zeros(n, dtype=torch.bool, device="cuda")
    if kind == "all":
        m[:] = True
    elif kind == "rand50":
        # a random half of the rows; a planted row of rank i follows the coin of its pair (i // 2: one spilled, one head rank), and the
        # first four pairs stay: the visible planted rows still alternate between the regions
        g = _gen(5000 + seed)
        m = torch.rand(n, generator=g, device="cuda") < 0.5
        coin = torch.rand((N_PLANTED, PLANTED_ROWS // 2), generator=g, device="cuda") < 0.5
        coin[:, :4] = True
        m[sh.planted_rows.flatten()] = coin.repeat_interleave(2, dim=1).flatten()
    elif kind == "spilled-only":
        m[LINE:] = True
    elif kind == "head-only":
        m[:LINE] = True
    elif kind == "boundary":
        m[LINE - 70:LINE + 70] = True
    elif kind == "lastgroup":
        m[(n - 1) // GROUP * GROUP:] = True
    else:
        raise AssertionError(kind)
    return m


def _assert_both_regions_decide(sh, m, nq, k, what):
    """The precondition, from float64: the exact top-k (over the rows of `m`) of every planted query among the first nq holds at least
    three rows at or beyond 2^20 and three below (k = 1: the best row lies beyond 2^20 for query 0, below for query 1)."""
    np_ = min(nq, N_PLANTED)
    top = sh.e64[:np_].masked_fill(~m[None, :], float("-inf")).topk(k, dim=1).indices
    beyond = (top >= LINE).sum(1)
    if k >= 6:
        assert (beyond >= 3).all() and (k - beyond >= 3).all(), (what, "the planted rows do not interleave the regions", beyond.tolist())
    else:
        assert int(beyond[0]) == k and (np_ < 2 or int(beyond[1]) == 0), (what, beyond.tolist())


def _check_fp64_in_slices(C_, Q_, s, i, rows, k, what, step=64):
    """_check_fp64 over 64 queries at a time (a float64 score matrix of 64 x 1.1 M is 0.6 GB)"""
    for a in range(0, Q_.shape[0], step):
        _check_fp64(C_, Q_[a:a + step].contiguous(), s[a:a + step], i[a:a + step], rows, k, (what, a))


def _four_paths(search, stats, ref, what, extra=()):
    """`search(**kw)` by the masked scan, the exhaustive path and the masked scan with a one-entry list: the bits of `ref`; -> the counters"""
    out = {}
    for name, kw in (("scan", dict(path=1)), ("exhaustive", dict(path=2)), ("cap1", dict(path=1, cand_cap=1))) + tuple(extra):
        got = search(**kw)
        out[name] = stats()
        assert _bits_equal(got, ref), (what, name, "differs from the library's choice")
    assert out["exhaustive"] == (0, 0), (what, out)
    return out


# ---- 1. the bitmap search beyond 2^20 rows: every path, float64, the compacted rows -------------------------------------------------------------
# (shard, nq, k) pairwise over {A, B} x {1, 64, 257} x {1, 10, 32}; every mask on both shards (lastgroup: A's ragged one, B's full one)
BITMAP_CASES = [
    ("A", 1, 10, ("all", "lastgroup", "boundary")),
    ("A", 64, 32, ("rand50", "spilled-only")),
    ("A", 257, 1, ("all", "head-only", "lastgroup")),
    ("A", 257, 10, ("rand50",)),
    ("B", 1, 32, ("all", "spilled-only")),
    ("B", 64, 10, ("all", "rand50", "boundary", "head-only")),
    ("B", 64, 1, ("rand50", "lastgroup")),
    ("B", 257, 32, ("rand50", "boundary")),
    ("B", 257, 10, ("spilled-only",)),
]
BITMAP_PARAMS = [(s, nq, k, m) for s, nq, k, ms in BITMAP_CASES for m in ms]


@gpu
@pytest.mark.parametrize("shard,nq,k,mask", BITMAP_PARAMS, ids=[f"{s}-{nq}q-k{k}-{m}" for s, nq, k, m in BITMAP_PARAMS])
def test_bitmap_search_beyond_2_20_rows_every_path_fp64_and_the_compacted_rows(hip, shards, shard, nq, k, mask):
    """Per case: the library's choice, the masked scan (with and without the count of allowed rows), the exhaustive path and the masked scan
    with a one-entry candidate list return the same bits; the answer passes the float64 check over the allowed rows and equals, bit for
    bit, the unfiltered search of an index of the allowed rows alone (and of the whole shard when every row is allowed).  The masked scan
    answers every query itself (no overflow) from at least min(k, non-empty groups) candidate groups per query."""
    from arxiv_rag_amd.index import ShardIndex
    sh = shards(shard)
    what = f"{shard}-{nq}q-k{k}-{mask}"
    C_, Q_, idx = sh.C, sh.Q[:nq].contiguous(), sh.idx
    m = _mask(mask, sh)
    if mask in ("all", "rand50"):
        _assert_both_regions_decide(sh, m, nq, k, what)
    rows = torch.nonzero(m).flatten()
    n_allowed = int(rows.shape[0])
    allow = _pack(m, garbage=True)                               # (A: the bits of the last word beyond the shard are set)
    G = (sh.n + GROUP - 1) // GROUP
    nonempty = int(torch.nn.functional.pad(m, (0, G * GROUP - sh.n)).view(G, GROUP).any(dim=1).sum())      # groups with an allowed row
    ref = idx.search(Q_, k, allow=allow, n_allowed=n_allowed)
    _check_fp64_in_slices(C_, Q_, ref[0], ref[1], rows, k, what)
    stats = _four_paths(lambda **kw: idx.search(Q_, k, allow=allow, **{"n_allowed": n_allowed, **kw}), idx.filtered_stats, ref, what,
                        extra=(("unknown-count", dict(n_allowed=None)),))
    over, cand = stats["scan"]
    print(f"{what}: allowed {n_allowed} of {sh.n} rows in {nonempty} groups; overflowed queries {over}, candidate groups per query "
          f"{cand / nq:.2f}; one-entry list: overflowed {stats['cap1'][0]} of {nq}")
    assert stats["unknown-count"] == stats["scan"], (what, "without n_allowed the library takes the masked scan", stats)
    assert over == 0, (what, "a query overflowed the default candidate list: the fallback answered, not the scan", stats)
    assert cand >= nq * min(k, nonempty), (what, "fewer candidate groups than the k-th largest maximum admits", stats)
    if k >= 2 and nonempty >= 2:
        assert stats["cap1"][0] == nq, (what, stats)
    s2, i2 = ShardIndex(C_[rows].contiguous()).search(Q_, k)
    i2 = torch.where(i2 >= 0, rows[i2.clamp_min(0)] + BASE, i2)
    assert _bits_equal((s2, i2), ref), (what, "differs from the unfiltered search of the compacted rows")
    if mask == "all":
        assert _bits_equal(idx.search(Q_, k), ref), (what, "all-rows mask differs from the unfiltered search")


# ---- 2. the fallback cannot hide a broken scan: no overflow, and the candidate count is the one float64 gives ---------------------------------
def _candidate_bounds(sh, m, k, idx):
    """Per query of the first 64: (lo, hi) bounds on the number of candidate groups of the masked scan, from the float64 group maxima E_g
    over the rows of `m`.  Pass A's maximum of a group lies within a = A(D) |q| max|c| of E_g (tests/helpers.py: pass_a_budget), so the
    k-th largest of them, t, within a of E_(k); a group is a candidate iff its pass-A maximum is >= t - 2 tau (masked_tail_kernel; tau =
    (0.3125 D + 4) u |q| max(max|c|, 1 + 2^-9), masked_search_impl).  Hence E_g >= E_(k) - 2 tau + 2 a makes g a candidate and every
    candidate has E_g >= E_(k) - 2 tau - 2 a; 2 u (1 + |E_(k)|) more for the float32 roundings of |q|, tau and the subtraction (the
    threshold, a value below 2, is rounded once: half an ulp, at most u).  With
    fewer than k non-empty groups every non-empty group is a candidate."""
    e = sh.e64.masked_fill(~m[None, :], float("-inf"))
    G = (sh.n + GROUP - 1) // GROUP
    pad = torch.full((e.shape[0], G * GROUP - sh.n), float("-inf"), dtype=torch.float64, device="cuda")
    E = torch.cat([e, pad], dim=1).view(e.shape[0], G, GROUP).amax(dim=2)                    # [64, G]
    kth = E.topk(min(k, G), dim=1).values[:, -1]
    kth = kth if k <= G else torch.full_like(kth, float("-inf"))
    qn = sh.Q[:64].double().norm(dim=1)
    cmax = float(sh.C.double().norm(dim=1).max())
    tau = (0.3125 * DIM + 4) * U24 * qn * max(idx.max_row_norm(), 1 + 2.0 ** -9)
    a = pass_a_budget(DIM) * qn * cmax
    slack = 2 * U24 * (1 + kth.abs().nan_to_num(posinf=0.0))
    finite = torch.isfinite(E)
    lo = ((E >= (kth - 2 * tau + 2 * a + slack)[:, None]) & finite).sum(1)
    hi = ((E >= (kth - 2 * tau - 2 * a - slack)[:, None]) & finite).sum(1)
    return lo, hi


@gpu
@pytest.mark.parametrize("shard", ["A", "B"])
def test_the_scan_never_overflows_on_unit_rows_and_rescores_the_groups_float64_names(hip, shards, shard):
    """path = 1 on unit rows, 64 queries (32 planted), k = 1 / 10 / 32, all rows and a random half: no query overflows the default list
    (float64 itself allows every query far fewer than 1 024 candidates), and the number of candidate groups rescored lies between the two
    float64 counts of _candidate_bounds — an over-count of the groups at or above a trial threshold in the spill loop raises the threshold
    and pushes the count below `lo`, an under-count lowers it and pushes the count above `hi`."""
    sh = shards(shard)
    Q_, idx = sh.Q[:64].contiguous(), sh.idx
    for mask in ("all", "rand50"):
        m = _mask(mask, sh, seed=1)
        allow = _pack(m)
        for k in (1, 10, 32):
            lo, hi = _candidate_bounds(sh, m, k, idx)
            idx.search(Q_, k, allow=allow, path=1)
            over, cand = idx.filtered_stats()
            print(f"{shard}-{mask}-k{k}: overflowed {over}; candidate groups {cand} (per query {cand / 64:.2f}); float64 bounds "
                  f"{int(lo.sum())} ... {int(hi.sum())}, largest per query {int(hi.max())}")
            assert int(hi.max()) <= 3 * PLANTED_ROWS < CAP_DEFAULT and int(lo.min()) >= k, (shard, mask, k, "the test's own inputs")
            assert over == 0, (shard, mask, k, over)
            assert cand >= 64 * k
            assert int(lo.sum()) <= cand <= int(hi.sum()), (shard, mask, k, "candidate groups outside the float64 bounds (tau as csrc/masked_topk.h masked_search_impl computes tau_scale)", cand)


# ---- 3. the candidate count does not depend on where the groups sit -----------------------------------------------------------------------------
def _assert_same_answer_under_a_row_shift(a, b, shift, n, what):
    """b = the answer over the shard rolled by `shift` rows: the score bits of `a`, and its ids moved by the shift (positions of one query
    that report bit-equal scores may come in another order: compared as sets)."""
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (what, "score bits")
    moved = torch.where(a[1] >= 0, (a[1] - BASE + shift) % n + BASE, a[1])
    differ = torch.nonzero((moved != b[1]).any(dim=1)).flatten().tolist()
    for q in differ:
        bits, x, y = a[0][q].view(torch.int32).tolist(), moved[q].tolist(), b[1][q].tolist()
        for v in set(bits):
            pos = [p for p, w in enumerate(bits) if w == v]
            assert sorted(x[p] for p in pos) == sorted(y[p] for p in pos), (what, "query", q, "ids")
    return len(differ)


@gpu
def test_rolling_the_shard_by_2_20_rows_keeps_the_answer_and_the_candidate_count(hip, shards):
    """B rolled by 2^20 rows (a multiple of the 256-row tile: every row keeps its place inside its tile, so pass A gives every group the
    bits it had): the spilled groups of the rolled shard are groups 0 ... 1091 of the original and the other way round.  Scores bit-equal,
    ids moved by the roll, and the same number of candidate groups: the set of candidate groups is defined by the group maxima alone, so a
    count that depends on whether a group's maximum sits in a register or is re-read is a defect (it need not change the answer)."""
    from arxiv_rag_amd.index import ShardIndex
    sh = shards("B")
    n, k, Q_ = sh.n, 10, sh.Q[:64].contiguous()
    m = _mask("rand50", sh, seed=2)
    _assert_both_regions_decide(sh, m, 64, k, "roll")
    a = sh.idx.search(Q_, k, allow=_pack(m), path=1)
    stats_a = sh.idx.filtered_stats()
    C2 = torch.roll(sh.C, LINE, 0).contiguous()
    assert torch.equal(C2[(LINE + 7 + LINE) % n], sh.C[LINE + 7]) and torch.equal(C2[LINE:], sh.C[:n - LINE])
    idx2 = ShardIndex(C2, idx_base=BASE)
    b = idx2.search(Q_, k, allow=_pack(torch.roll(m, LINE)), path=1)
    stats_b = idx2.filtered_stats()
    reordered = _assert_same_answer_under_a_row_shift(a, b, LINE, n, "roll")
    print(f"roll by 2^20: (overflowed, candidate groups) = {stats_a} and rolled {stats_b}; queries with tied scores in another order: {reordered}")
    assert stats_a[0] == 0 and stats_b == stats_a, ("the candidate count depends on where the groups sit", stats_a, stats_b)
    # ... and through the other policy: every row of the rolled shard below the limit n
    lim = torch.full((64,), n, dtype=torch.int64, device="cuda")
    pa = sh.idx.search_prefix(Q_, lim, k, path=1)
    stats_pa = sh.idx.prefix_stats()
    pb = idx2.search_prefix(Q_, lim, k, path=1)
    stats_pb = idx2.prefix_stats()
    _assert_same_answer_under_a_row_shift(pa, pb, LINE, n, "roll, prefix")
    print(f"roll by 2^20, prefix policy, every row: {stats_pa} and rolled {stats_pb}")
    assert stats_pa[0] == 0 and stats_pb == stats_pa, (stats_pa, stats_pb)
    del C2, idx2


# ---- 4. the check can fail ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shard", ["A", "B"])
def test_the_fp64_check_rejects_an_answer_that_ignores_the_spilled_groups(hip, shards, shard):
    """What a tail that skipped the spilled groups would return is the answer for the mask with every row >= 2^20 cleared.  For each
    planted query that answer passes the float64 check over its own mask and raises against the full one."""
    sh = shards(shard)
    k = 10
    Q_ = sh.Q[:N_PLANTED].contiguous()
    full = _mask("all", sh)
    head = _mask("head-only", sh)
    _assert_both_regions_decide(sh, full, N_PLANTED, k, shard)
    s, i = sh.idx.search(Q_, k, allow=_pack(head))
    _check_fp64(sh.C, Q_, s, i, torch.nonzero(head).flatten(), k, (shard, "head-only"))
    rows = torch.nonzero(full).flatten()
    for j in range(N_PLANTED):
        with pytest.raises(AssertionError):
            _check_fp64(sh.C, Q_[j:j + 1], s[j:j + 1], i[j:j + 1], rows, k, (shard, "full mask", j))


# ---- 5. prefix search across the line -------------------------------------------------------------------------------------------------------------
def _prefix_limits():
    """300 limits: the listed ones twice over the planted queries (0 ... 15 and, reversed, 16 ... 31: either parity of the planting),
    the extra ones on queries 32 ... 34, the rest random in [0, N_B]"""
    rs = np.random.RandomState(300)
    lim = rs.randint(0, N_B + 1, size=NQ_ALL).astype(np.int64)
    lim[:16] = LISTED_LIMITS
    lim[16:32] = LISTED_LIMITS[::-1]
    lim[32:35] = EXTRA_LIMITS
    return lim


@gpu
@pytest.mark.parametrize("k", [10, 32])
def test_prefix_search_with_limits_on_both_sides_of_2_20(hip, shards, k):
    """One batch of 300 queries over B whose blocks read 0, 1, 2, 63, 64, 65, 1 024, 1 025 and 1 092 spilled groups side by side: every
    path the same bits; ids below the limit, padding exact; a sample holding every listed limit bit-equal to the filtered search of the
    bitmap of rows below the limit and an exact top-k of C[:limit] by float64."""
    sh = shards("B")
    C_, Q_, idx, n = sh.C, sh.Q, sh.idx, sh.n
    lim = _prefix_limits()
    lim_d, lim_c = torch.from_numpy(lim).cuda(), np.clip(lim, 0, n)
    what = f"prefix-k{k}"
    ref = idx.search_prefix(Q_, lim_d, k)
    over0, cand0 = idx.prefix_stats()
    stats = _four_paths(lambda **kw: idx.search_prefix(Q_, lim_d, k, **kw), idx.prefix_stats, ref, what)
    spilled_blocks = int((lim_c > LINE).sum())
    print(f"{what}: {spilled_blocks} of {NQ_ALL} blocks read spilled groups; overflowed queries {stats['scan'][0]}, candidate groups per query "
          f"{stats['scan'][1] / NQ_ALL:.2f}; one-entry list: overflowed {stats['cap1'][0]}")
    assert 32 <= spilled_blocks <= NQ_ALL - 32                   # (a uniform limit lies beyond 2^20 with probability 1 / 16)
    assert (over0, cand0) == stats["scan"] and stats["scan"][0] == 0, (what, stats)
    assert stats["cap1"][0] == int((lim_c > GROUP).sum()), (what, "fallback count with a one-entry list", stats)
    check_prefix_answer(ref[0], ref[1], lim_c, k, BASE, what)
    # the planted queries whose limit covers the shard see both regions
    whole = [j for j in range(N_PLANTED) if lim_c[j] == n]
    assert len(whole) >= 6
    beyond = ((ref[1][whole] - BASE) >= LINE).sum(1)
    assert (beyond >= 3).all() and (k - beyond >= 3).all(), (what, beyond.tolist())
    sample = list(range(16)) + [32, 33, 34] + [40, 77, 130, 211, 299]
    assert len(sample) <= 24 and set(LISTED_LIMITS) <= set(lim[sample].tolist())
    check_against_filtered_and_fp64(idx, C_, Q_, lim_c, ref[0], ref[1], k, sample, what)


def _below_words(limit, n):
    """the bitmap of rows < limit, built on the device (the self-join check below makes hundreds of them)"""
    g = torch.arange((n + GROUP - 1) // GROUP, device="cuda")
    full, rem = divmod(int(limit), GROUP)
    w = torch.where(g < full, torch.full_like(g, -1), torch.zeros_like(g))
    if rem:
        w[full] = (1 << rem) - 1
    return w


@gpu
@pytest.mark.parametrize("k", [1, 10])
def test_self_join_across_2_20_and_at_the_end_of_the_shard(hip, shards, k):
    """nearest_earlier over rows 2^20 - 3 ... 2^20 + 199 (blocks without and with spilled groups in one batch) and over the last 130 rows:
    every row's answer bit-equal to the filtered search of the bitmap of its earlier rows; the planted exact copies of rows 5 and 2^20 + 7
    report their first original."""
    sh = shards("B")
    C_, idx, n = sh.C, sh.idx, sh.n
    for lim in (1, GROUP, LINE + 7, n - 1):
        assert torch.equal(_below_words(lim, n), allow_below(lim, n))
    for a, b in ((LINE - 3, LINE + 200), (n - 130, n)):
        s, i = idx.nearest_earlier(a, b, k)
        over, cand = idx.prefix_stats()
        print(f"self-join k{k} rows {a} ... {b - 1}: overflowed queries {over}, candidate groups per query {cand / (b - a):.2f}")
        assert over == 0
        check_prefix_answer(s, i, np.arange(a, b, dtype=np.int64), k, BASE, (a, b))
        copies = [r for r in COPIES if a <= r < b]
        assert len(copies) == 2
        for r in copies:
            first = COPIES[r]
            assert torch.equal(C_[r], C_[first]) and int(i[r - a, 0]) == first + BASE, (r, "a copy does not report its first original", int(i[r - a, 0]) - BASE)
            assert float(s[r - a, 0]) > 0.99
        fs = torch.empty_like(s); fi = torch.empty_like(i)
        for r in range(a, b):
            idx.search(C_[r:r + 1], k, allow=_below_words(r, n), n_allowed=r, out=(fs[r - a:r - a + 1], fi[r - a:r - a + 1]))
        differ = torch.nonzero((fi != i).any(1) | (fs.view(torch.int32) != s.view(torch.int32)).any(1)).flatten()
        assert differ.numel() == 0, ("rows whose self-join answer differs from the filtered search", (differ + a).tolist()[:8])
        s2, i2 = idx.nearest_earlier(a, b, k, path=2)
        assert _bits_equal((s2, i2), (s, i)), (a, b, "exhaustive path")
