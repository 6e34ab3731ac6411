"""Boosted search (csrc/boosted.hip: `ShardIndex.search_boosted`, `prior_info`) where tests/test_gpu_boosted_search.py stops: shards of
more than FILT_REG_GROUPS * FILT_TAIL_NT = 16 384 groups (2^20 rows), whose further group maxima the tail re-reads in the spill loops of
tail_kth_key and tail_candidates and whose candidate rows read prior[row] and eff[group] beyond 2^20; calls of more than QBATCH_MAX
queries (the slice's `weight + q0`, the slice-local wq[q]); dims 1536 / 4096 / 8192 up to the dynamic LDS at which the host raises the
tail kernel's limit.

The shards.  Two of dim 64 with the sizes and the planted layout of tests/test_gpu_masked_search_large.py (`N_A`: 4 spilled groups, the
last ragged; `N_B`: 1 092 spilled groups; `_planted_layout`: per query 64 rows a q + sqrt(1 - a^2) noise, a from 0.95 down to 0.70,
alternating between the spilled groups and the first 16 384), but drawn with numpy, because the reference runs on the host.  8 planted
queries; the prior is a seeded f32 in [0, 1) per row; weights cycle through (0, 0.02, 0.2, 5, -0.2).

The reference.  The GPU's scores, base scores and ids are compared bit for bit with `boost.boosted_host` (base = `exact_scores_host`,
computed once per shard).  So that this is not the project compared with itself, a CPU test holds that restatement to float64 on these
very inputs: S64 = X64 . q64 + float64(w) float64(prior) (the product of two f32 values is exact in float64).  The restatement's score is
fl32(b + fl32(w p)) with |b - q . c| <= B(D) |q| |c| (tests/helpers.py: pass_b_budget), one rounding of the product, at most
2^-24 |w p|, and one of the sum, at most 2^-24 |b + w p|:
    |s - S64| <= E := pass_b_budget(D) |q| max|c| + 2^-24 (|w p| + |b + w p|)
A position of the float64 order is DECIDED when its gaps to both neighbours exceed 2 E (E the largest over the rows at hand): no
assignment of errors within E can move another row there, and the restatement must name the float64 row.  Every position that holds a
planted row must be decided (a fixture error otherwise, never a skip); of the others at most 2 % may be undecided.  The seeds below meet
that on the reference alone; the cap is not to be raised.

Figures printed (profiles/boosted_large_fp64.md): overflowed queries and candidate groups per case, the undecided share per case."""
import re

import numpy as np
import pytest

from arxiv_rag_amd import boost as BO
from arxiv_rag_amd.topics import exact_scores_host
from arxiv_rag_amd.where import pack_bitmap
from tests.helpers import pass_b_budget
from tests.test_gpu_masked_search_large import CAP_DEFAULT, CAP_MAX, CSRC, GROUP, LINE, LINE_G, N_A, N_B, TAIL_NT, _define, _planted_layout

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
DEV = "cuda:0"
DIM, NQ = 64, 8
WEIGHTS = np.array([0.0, 0.02, 0.2, 5.0, -0.2], np.float32)
QBATCH_MAX = _define("search_consts.h", "QBATCH_MAX")
MASKS = ("none", "beyond", "best-hidden", "non-finite")
UNDECIDED_CAP = 0.02
U24 = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same(got, want):
    gs, gb, gi = (t.cpu().numpy() for t in got)
    return np.array_equal(bits(gs), bits(want[0])) and np.array_equal(bits(gb), bits(want[1])) and np.array_equal(gi, want[2])


def first_k(want, k):
    """the answer at k from the answer at 32: the k best are a prefix of the 32 best, pads included"""
    return tuple(a[:, :k] for a in want)


def _unit_rows(rs, n, dim):
    out = np.empty((n, dim), np.float32)
    for a in range(0, n, 1 << 16):
        v = rs.randn(min(1 << 16, n - a), dim)
        out[a:a + v.shape[0]] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return out


# ---- the two shards, on the host ---------------------------------------------------------------------------------------------------------
_SHARDS = {}


def shard(name):
    """The shard's rows, queries, prior, weights, masks, `exact_scores_host` and float64 base scores, and `boosted_host` at k = 32 per
    mask: host data, built once per process, left unchanged."""
    if name in _SHARDS:
        return _SHARDS[name]
    n = {"A": N_A, "B": N_B}[name]
    rs = np.random.RandomState({"A": 4101, "B": 4102}[name])
    Xf = _unit_rows(rs, n, DIM)
    Q = _unit_rows(rs, NQ, DIM).astype(np.float16)
    rows, a = _planted_layout(n, n)
    rows, a = rows[:NQ], np.asarray(a[:NQ], np.float64)
    qh = Q.astype(np.float64)
    qh /= np.linalg.norm(qh, axis=1, keepdims=True)
    noise = rs.randn(NQ, rows.shape[1], DIM)
    noise -= (noise * qh[:, None, :]).sum(2, keepdims=True) * qh[:, None, :]
    noise /= np.linalg.norm(noise, axis=2, keepdims=True)
    Xf[rows.reshape(-1)] = (a[:, :, None] * qh[:, None, :] + np.sqrt(1 - a * a)[:, :, None] * noise).reshape(-1, DIM)
    X = Xf.astype(np.float16)
    del Xf
    prior = rs.rand(n).astype(np.float32)
    weight = WEIGHTS[np.arange(NQ) % len(WEIGHTS)].copy()
    base64 = np.concatenate([X[s:s + (1 << 18)].astype(np.float64) @ Q.astype(np.float64).T for s in range(0, n, 1 << 18)])      # [n, 8]
    beyond = np.zeros(n, bool); beyond[LINE:] = True
    hidden = np.ones(n, bool); hidden[rows[:, 0]] = False; hidden[int(prior.argmax())] = False
    bad = prior.copy()
    bad[rows[:, 0]] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(NQ) % 3]
    bad[(LINE_G + 2) * GROUP:(LINE_G + 3) * GROUP] = np.nan      # a whole spilled group
    masks = {"none": (None, prior), "beyond": (beyond, prior), "best-hidden": (hidden, prior), "non-finite": (None, bad)}
    w = dict(name=name, n=n, X=X, Q=Q, prior=prior, weight=weight, planted=rows, masks=masks, B=exact_scores_host(X, Q), base64=base64,
             qn=np.linalg.norm(Q.astype(np.float64), axis=1), cmax=float(np.linalg.norm(X.astype(np.float32), axis=1).max()))
    w["want"] = {m: BO.boosted_host(X, Q, p, weight, 32, allow, base=w["B"]) for m, (allow, p) in masks.items()}
    _SHARDS[name] = w
    return w


def fp64_order(w, mask, q, weight, k):
    """The float64 order of query q under `mask` and `weight`: -> (rows of the k + 1 best, their S64, the error bound E over them)"""
    allow, prior = w["masks"][mask]
    vis = np.isfinite(prior) if allow is None else allow & np.isfinite(prior)
    wp = np.float64(weight) * np.where(vis, prior, 0).astype(np.float64)
    S = np.where(vis, w["base64"][:, q] + wp, -np.inf)
    top = np.argpartition(-S, k + 1)[:k + 1]
    top = top[np.lexsort((top, -S[top]))]
    top = top[np.isfinite(S[top])]
    e0 = pass_b_budget(DIM) * w["qn"][q] * w["cmax"]
    E = float((e0 + U24 * (np.abs(wp[top]) + np.abs(S[top]) + e0)).max())
    return top, S[top], E


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_restatement_holds_to_float64_on_these_shards(name):
    """CPU only: `boosted_host` against float64 at every decided position of every mask, k = 32 (the header says what decided means);
    the planted positions all decided, at most 2 % of the others undecided; and the inputs let neither term decide alone: at weights
    0.02 and 0.2 the float64 top-10 and top-32 hold rows on both sides of row 2^20 and differ from the weight-0 ones."""
    w = shard(name)
    planted = set(w["planted"].reshape(-1).tolist())
    for mask in MASKS:
        ids = w["want"][mask][2]
        undecided = others = 0
        for q in range(NQ):
            top, S, E = fp64_order(w, mask, q, w["weight"][q], 32)
            m = min(32, top.shape[0])
            assert (ids[q, m:] == -1).all() and (ids[q, :m] >= 0).all(), (name, mask, q)
            for p in range(m):
                gaps = [S[p - 1] - S[p]] if p else []
                gaps += [S[p] - S[p + 1]] if p + 1 < top.shape[0] else []
                decided = all(g > 2 * E for g in gaps)
                if int(top[p]) in planted:
                    assert decided, (name, mask, q, p, "a planted position is not decided: the fixture is wrong", gaps, E)
                else:
                    others += 1
                    undecided += not decided
                if decided:
                    assert ids[q, p] == top[p], (name, mask, q, p, "boosted_host names another row than float64", int(ids[q, p]), int(top[p]))
        print(f"{name} {mask}: undecided {undecided} of {others} positions without a planted row ({100.0 * undecided / max(others, 1):.2f} %)")
        assert undecided <= UNDECIDED_CAP * others, (name, mask, undecided, others)
    for q in range(NQ):
        if w["weight"][q] not in (np.float32(0.02), np.float32(0.2)):
            continue
        for k in (10, 32):
            top = fp64_order(w, "none", q, w["weight"][q], k)[0][:k]
            plain = fp64_order(w, "none", q, 0.0, k)[0][:k]
            assert (top >= LINE).any() and (top < LINE).any(), (name, q, k, "the top-k lies on one side of 2^20")
            assert top.tolist() != plain.tolist(), (name, q, k, "the prior does not move the top-k")
            assert set(top.tolist()) & set(plain.tolist()), (name, q, k, "the cosine does not matter")
    assert sum(set(fp64_order(w, "none", q, w["weight"][q], 10)[0][:10].tolist()) != set(fp64_order(w, "none", q, 0.0, 10)[0][:10].tolist())
               for q in range(NQ) if w["weight"][q] != 0) >= 3


def _tail_lds_bytes(dim, cand_cap):
    """dynamic LDS of boosted_tail_kernel (BoostedSearch::launch_tail): the query row, one 64-score stretch per wave, the candidate list"""
    return ((dim * 2 + 15) & ~15) + (TAIL_NT // 64) * GROUP * 4 + cand_cap * 4


def test_the_shapes_cross_the_lines():
    """CPU only: the largest candidate list at dim 8192 is above the dynamic LDS a kernel gets without asking, the default list at dim
    4096 is not; the two shards have spilled groups; QBATCH_MAX + 70 queries are two slices."""
    src = (CSRC / "boosted.hip").read_text()
    m = re.search(r"kSmemRaise\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", src)
    assert m, "boosted.hip no longer defines kSmemRaise"
    raise_at = int(m.group(1)) * int(m.group(2))
    assert raise_at == 48 * 1024 and (CAP_DEFAULT, CAP_MAX) == (1024, 8192)
    assert _tail_lds_bytes(8192, CAP_MAX) == 16384 + 4096 + 32768 > raise_at >= _tail_lds_bytes(4096, CAP_DEFAULT) == 8192 + 4096 + 4096
    assert _tail_lds_bytes(8192, CAP_DEFAULT) <= raise_at
    assert LINE == 1 << 20 and (N_A + GROUP - 1) // GROUP - LINE_G == 4 and N_A % GROUP == 5 and (N_B + GROUP - 1) // GROUP - LINE_G == 1092
    assert QBATCH_MAX == 1024 and N_B % 256 == 0 and LINE % 256 == 0


# ---- a. the shards on the device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def on_device():
    """name -> the shard's index and device tensors (built on first use, freed with the module)"""
    from arxiv_rag_amd.index import ShardIndex
    built = {}

    def get(name):
        if name not in built:
            w = shard(name)
            d = dict(idx=ShardIndex(dev(w["X"], np.float16), prefilter=None), Q=dev(w["Q"], np.float16), prior={}, allow={})
            for m, (allow, p) in w["masks"].items():
                d["prior"][m] = dev(p, np.float32)
                d["allow"][m] = None if allow is None else dev(pack_bitmap(allow).view(np.int64), np.int64)
            built[name] = d
        return built[name]
    yield get
    built.clear()
    torch.cuda.empty_cache()


PATHS = (("default", {}), ("scan", dict(path=1)), ("cap8", dict(path=1, cand_cap=8)), ("exhaustive", dict(path=2)))


@gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_boosted_search_beyond_2_20_rows_every_path(on_device, name, mask):
    w, d = shard(name), on_device(name)
    idx = d["idx"]
    visible_groups = 4 if (name, mask) == ("A", "beyond") else 1000
    for k in (1, 10, 32):
        want = first_k(w["want"][mask], k)
        stats = {}
        for label, kw in PATHS:
            got = idx.search_boosted(d["Q"], k, d["prior"][mask], w["weight"], allow=d["allow"][mask], **kw)
            stats[label] = idx.boosted_stats()
            assert same(got, want), (name, mask, k, label)
        print(f"{name} {mask} k{k}: (overflowed queries, candidate groups) = {stats}")
        assert stats["scan"][0] == 0 and stats["exhaustive"] == (0, 0), (name, mask, k, stats)
        if k >= 10 and visible_groups > 8:
            assert stats["cap8"][0] == NQ, (name, mask, k, "a list of 8 groups did not overflow", stats)
    i = w["want"][mask][2]
    if mask == "none":
        assert all((i[q, :10] >= LINE).any() and (i[q, :10] < LINE).any() for q in (1, 2, 6, 7))
    if mask == "beyond":
        assert (i[i >= 0] >= LINE).all() and (i[:, :10] >= 0).all()
    if mask in ("best-hidden", "non-finite"):
        assert not set(i.reshape(-1).tolist()) & set(w["planted"][:, 0].tolist())
    if mask == "non-finite":
        assert not ((i >= (LINE_G + 2) * GROUP) & (i < (LINE_G + 3) * GROUP)).any()
        assert np.isfinite(w["want"][mask][0]).all()


# ---- b. a roll by 2^20 rows --------------------------------------------------------------------------------------------------------------
@gpu
def test_rolling_shard_b_by_2_20_rows_keeps_the_answer(on_device):
    """B rolled by 2^20 rows, with its prior and bitmap (a multiple of the 256-row tile: every row keeps its place inside its tile): the
    spilled groups of the rolled shard are the first 1 092 of the original.  Score and base bits equal, ids moved by the roll (positions
    of one query with bit-equal scores compared as sets), and the same number of candidate groups."""
    from arxiv_rag_amd.index import ShardIndex
    w, d = shard("B"), on_device("B")
    n, k = w["n"], 10
    rs = np.random.RandomState(12)
    mask = rs.rand(n) < 0.5
    mask[w["planted"].reshape(-1)] = True
    for allow in (None, mask):
        a = d["idx"].search_boosted(d["Q"], k, d["prior"]["none"], w["weight"], path=1,
                                    allow=None if allow is None else dev(pack_bitmap(allow).view(np.int64), np.int64))
        stats_a = d["idx"].boosted_stats()
        a = tuple(t.cpu().numpy() for t in a)
        idx2 = ShardIndex(torch.roll(d["idx"].corpus, LINE, 0).contiguous(), prefilter=None)
        b = idx2.search_boosted(d["Q"], k, torch.roll(d["prior"]["none"], LINE).contiguous(), w["weight"], path=1,
                                allow=None if allow is None else dev(pack_bitmap(np.roll(allow, LINE)).view(np.int64), np.int64))
        stats_b = idx2.boosted_stats()
        b = tuple(t.cpu().numpy() for t in b)
        del idx2
        print(f"roll by 2^20, bitmap {allow is not None}: (overflowed, candidate groups) = {stats_a} and rolled {stats_b}")
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
        moved = np.where(a[2] >= 0, (a[2] + LINE) % n, a[2])
        for q in range(NQ):
            for v in set(bits(a[0][q]).tolist()):
                pos = bits(a[0][q]) == v
                assert sorted(moved[q][pos].tolist()) == sorted(b[2][q][pos].tolist()), (q, "ids")
        assert (a[2][[1, 2, 6, 7]] >= LINE).any(axis=1).all() and (a[2][[1, 2, 6, 7]] < LINE).any(axis=1).all()
        assert stats_a[0] == 0 and stats_a == stats_b, (stats_a, stats_b)


# ---- c. more queries than one slice ------------------------------------------------------------------------------------------------------
N_SMALL, NQ_TWO = 1000, QBATCH_MAX + 70


@pytest.fixture(scope="module")
def two_slices():
    """dim -> 1000 rows and QBATCH_MAX + 70 queries whose last 70 repeat queries 0 ... 69 with the weights rotated by one, so a slice
    that read the first slice's weights would return other rows; the host answers with and without a bitmap"""
    built = {}

    def get(dim):
        if dim not in built:
            rs = np.random.RandomState(3000 + dim)
            X = (rs.randn(N_SMALL, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
            Q = (rs.randn(QBATCH_MAX, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
            Q = np.concatenate([Q, Q[:70]])
            prior = rs.rand(N_SMALL).astype(np.float32)
            weight = WEIGHTS[np.concatenate([np.arange(QBATCH_MAX), np.arange(70) + 1]) % len(WEIGHTS)].copy()
            B = exact_scores_host(X, Q[:QBATCH_MAX])
            B = np.concatenate([B, B[:, :70]], axis=1)
            half = rs.rand(N_SMALL) < 0.5
            built[dim] = dict(X=X, Q=Q, prior=prior, weight=weight, half=half,
                              want={"all": BO.boosted_host(X, Q, prior, weight, 10, None, base=B),
                                    "half": BO.boosted_host(X, Q, prior, weight, 10, half, base=B)})
        return built[dim]
    yield get
    built.clear()


@gpu
@pytest.mark.parametrize("dim", [64, 768])
def test_more_queries_than_one_slice(two_slices, dim):
    from arxiv_rag_amd.index import ShardIndex
    w = two_slices(dim)
    idx = ShardIndex(dev(w["X"], np.float16), prefilter=None)
    dQ, dp = dev(w["Q"], np.float16), dev(w["prior"], np.float32)
    for name, allow in (("all", None), ("half", dev(pack_bitmap(w["half"]).view(np.int64), np.int64))):
        want = w["want"][name]
        for label, kw in (("default", {}), ("cap1", dict(path=1, cand_cap=1)), ("exhaustive", dict(path=2))):
            got = idx.search_boosted(dQ, 10, dp, w["weight"], allow=allow, **kw)
            over = idx.boosted_stats()[0]
            assert same(got, want), (dim, name, label)
            if label == "cap1":                                  # ten rows lie in more than one group: every query of both slices is redone
                assert over == NQ_TWO, (dim, name, over)
        # what a second slice with the first slice's weights would return differs in ids, not only in score bits
        again, first = want[2][QBATCH_MAX:], want[2][:70]
        assert sum(again[j].tolist() != first[j].tolist() for j in range(70)) >= 50, (dim, name)
        same_w = [j for j in range(70) if w["weight"][QBATCH_MAX + j] == w["weight"][j]]
        assert same_w == []


@gpu
def test_one_query_more_than_a_slice_on_shard_a(on_device):
    """QBATCH_MAX + 1 queries on shard A: the 8 planted queries over and over with their weights, and one query of a second slice,
    planted query 0 with weight 0.02 where the first slice gave it weight 0: the answer of the last query differs from query 0's."""
    w, d = shard("A"), on_device("A")
    k, nq = 10, QBATCH_MAX + 1
    pick = np.arange(nq) % NQ
    weight = w["weight"][pick].copy()
    weight[-1] = WEIGHTS[1]
    want8 = first_k(w["want"]["none"], k)
    last = BO.boosted_host(w["X"], w["Q"][:1], w["prior"], WEIGHTS[1:2], k, None, base=w["B"][:, :1])
    want = tuple(np.concatenate([a[pick[:-1]], b]) for a, b in zip(want8, last))
    assert want[2][-1].tolist() != want[2][0].tolist()
    dQ = d["Q"][torch.from_numpy(pick).to(DEV)].contiguous()
    for label, kw in PATHS:
        got = d["idx"].search_boosted(dQ, k, d["prior"]["none"], weight, **kw)
        assert same(got, want), label


# ---- d. large dims -----------------------------------------------------------------------------------------------------------------------
N_WIDE = 64 * 5 + 9


@gpu
@pytest.mark.parametrize("dim", [1536, 4096, 8192])
def test_large_dims_every_path_and_the_largest_candidate_list(dim):
    from arxiv_rag_amd.index import ShardIndex
    rs = np.random.RandomState(dim)
    X = (rs.randn(N_WIDE, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
    X[300] = X[10]
    Q = (rs.randn(NQ, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
    Q[0] = X[10]
    prior = rs.rand(N_WIDE).astype(np.float32)
    prior[[20, 328]] = np.nan, np.inf
    weight = WEIGHTS[np.arange(NQ) % len(WEIGHTS)].copy()
    half = rs.rand(N_WIDE) < 0.5
    B = exact_scores_host(X, Q)
    idx = ShardIndex(dev(X, np.float16), prefilter=None)
    dQ, dp = dev(Q, np.float16), dev(prior, np.float32)
    for name, allow in (("all", None), ("half", half)):
        want32 = BO.boosted_host(X, Q, prior, weight, 32, allow, base=B)
        da = None if allow is None else dev(pack_bitmap(allow).view(np.int64), np.int64)
        vis = np.isfinite(prior) & (True if allow is None else allow)
        nonempty = sum(bool(vis[g:g + GROUP].any()) for g in range(0, N_WIDE, GROUP))      # groups with a visible row: each a candidate at k = 32
        assert nonempty >= 5
        for k in (1, 32):
            for label, kw in PATHS + (("cap-max", dict(path=1, cand_cap=CAP_MAX)), ("cap1", dict(path=1, cand_cap=1))):
                got = idx.search_boosted(dQ, k, dp, weight, allow=da, **kw)
                stats = idx.boosted_stats()
                assert same(got, first_k(want32, k)), (dim, name, k, label)
                if label in ("scan", "cap-max"):
                    assert stats[0] == 0 and stats[1] >= NQ * min(k, nonempty), (dim, name, k, label, stats)
    assert not set(want32[2].reshape(-1).tolist()) & {20, 328}


# ---- e. arx_prior_info beyond 2^20 -------------------------------------------------------------------------------------------------------
@gpu
def test_prior_info_on_shard_b(on_device):
    w, d = shard("B"), on_device("B")
    p = w["prior"].copy()
    p[N_B - 1] = -3.25
    p[[LINE + 1, LINE + 60000, N_B - 2]] = np.nan, np.inf, -np.inf
    assert d["idx"].prior_info(dev(p, np.float32)) == (3.25, 3)
    assert d["idx"].prior_info(d["prior"]["none"]) == (float(w["prior"].max()), 0)
