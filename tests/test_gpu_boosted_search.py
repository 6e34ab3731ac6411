"""Boosted search on the GPU (`arx_topk_search_boosted`, `arx_prior_info`; INTEGRATION.md "Boosted search"): every comparison is exact,
float bits through a uint32 view and ids equal, against `boost.boosted_host`."""

import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib
from arxiv_rag_amd import boost as BO
from arxiv_rag_amd.index import ShardIndex
from arxiv_rag_amd.topics import exact_scores_host
from arxiv_rag_amd.where import pack_bitmap

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, NQ = 1000, 70                                                # 70 queries: the 64-query tile is full and a second one is ragged
N_ROWS = (1, 63, 64, 65, 257, 1000)
WEIGHTS = np.array([0.0, 0.02, 0.2, 5.0, -0.2], np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same(got, want):
    gs, gb, gi = (t.cpu().numpy() for t in got)
    return np.array_equal(bits(gs), bits(want[0])) and np.array_equal(bits(gb), bits(want[1])) and np.array_equal(gi, want[2])


_BASE = {}


def base(dim):
    """The shard of one dim, its queries, prior and weights, the host's base scores: computed once, shared and left unchanged."""
    if dim not in _BASE:
        rs = np.random.RandomState(1000 + dim)
        X = (rs.randn(N, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        X[500] = X[10]                                           # two identical rows ...
        Q = (rs.randn(NQ, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        Q[0] = X[10]                                             # ... and a query equal to them
        prior = rs.rand(N).astype(np.float32)
        weight = WEIGHTS[np.arange(NQ) % len(WEIGHTS)].copy()    # mixed within the batch; query 0 has weight 0
        w = dict(X=X, Q=Q, prior=prior, weight=weight, B=exact_scores_host(X, Q), dX=dev(X, np.float16), dQ=dev(Q, np.float16),
                 dprior=dev(prior, np.float32), idx={})
        _BASE[dim] = w
    return _BASE[dim]


def index(w, n=N):
    if n not in w["idx"]:
        w["idx"][n] = ShardIndex(w["dX"][:n].contiguous(), prefilter=None)
    return w["idx"][n]


def weights(w, weight, qs):
    """The batch's weights (or `weight`: a number, or one per query of the whole batch) of the queries `qs`."""
    weight = w["weight"] if weight is None else weight
    return weight if np.ndim(weight) == 0 else np.asarray(weight)[qs]


def host(w, k, n=N, prior=None, weight=None, allow=None, queries=None):
    qs = slice(None) if queries is None else queries
    return BO.boosted_host(w["X"][:n], w["Q"][qs], w["prior"][:n] if prior is None else prior, weights(w, weight, qs), k, allow,
                           base=w["B"][:n, qs])


def run(w, k, n=N, prior=None, weight=None, allow=None, queries=None, **kw):
    qs = slice(None) if queries is None else queries
    p = w["dprior"][:n].contiguous() if prior is None else dev(prior, np.float32)
    return index(w, n).search_boosted(w["dQ"][qs].contiguous(), k, p, weights(w, weight, qs),
                                      allow=None if allow is None else dev(allow, np.int64), **kw)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 10, 32))
@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("dim", [64, 768])
def test_boosted_search_equals_the_definition(dim, n, k):
    w = base(dim)
    got, want = run(w, k, n), host(w, k, n)
    assert same(got, want)
    assert (want[2][:, :min(k, n)] >= 0).all() and (want[2][:, min(k, n):] == -1).all()


@pytest.mark.parametrize("dim", [64, 768])
def test_the_data_lets_neither_term_decide_alone(dim):
    """At weight 0.02 the boosted top-10 of more than half of the queries holds a row outside the plain top-10 and a row inside it: on
    these inputs the prior is neither a no-op nor the only thing that matters.  Host data only (the device equals it: the test above)."""
    w = base(dim)
    plain = host(w, 10, weight=0.0)[2]
    boosted = host(w, 10, weight=0.02)[2]
    both = sum(1 for q in range(NQ) if set(boosted[q]) - set(plain[q]) and set(boosted[q]) & set(plain[q]))
    assert both * 2 > NQ, both
    got = run(w, 10, weight=0.02)
    assert np.array_equal(got[2].cpu().numpy(), boosted)


@pytest.mark.parametrize("dim", [64, 768])
def test_zero_weight_is_the_filtered_search(dim):
    w = base(dim)
    rs = np.random.RandomState(3)
    for mask in (np.ones(N, bool), rs.rand(N) < 0.5):
        words = pack_bitmap(mask).view(np.int64)
        s, b, i = run(w, 10, weight=0.0, allow=words)
        fs, fi = index(w).search(w["dQ"], 10, allow=dev(words, np.int64))
        assert torch.equal(i, fi) and np.array_equal(bits(b.cpu().numpy()), bits(fs.cpu().numpy()))
        assert np.array_equal(bits(s.cpu().numpy()), bits(fs.cpu().numpy()))      # base + 0 * prior = base (no score here is -0.0)


@pytest.mark.parametrize("dim", [64, 768])
def test_base_holds_the_filtered_searchs_bits_of_the_same_rows(dim):
    w = base(dim)
    s, b, i = (t.cpu().numpy() for t in run(w, 10))
    for q in range(NQ):
        mask = np.zeros(N, bool); mask[i[q]] = True
        fs, fi = index(w).search(w["dQ"][q:q + 1].contiguous(), 32, allow=dev(pack_bitmap(mask).view(np.int64), np.int64))
        of = dict(zip(fi[0].cpu().numpy().tolist(), bits(fs[0].cpu().numpy()).tolist()))
        assert [of[r] for r in i[q].tolist()] == bits(b[q]).tolist(), q


@pytest.mark.parametrize("dim", [64, 768])
def test_ties_go_to_the_lower_row_and_a_larger_prior_wins(dim):
    w = base(dim)
    q0 = slice(0, 1)
    equal = w["prior"].copy(); equal[500] = equal[10] = 1.0        # above every other prior: the twins lead
    got = run(w, 10, prior=equal, weight=5.0, queries=q0)
    assert same(got, host(w, 10, prior=equal, weight=5.0, queries=q0))
    s, b, i = (t.cpu().numpy() for t in got)
    assert i[0, 0] == 10 and i[0, 1] == 500 and bits(s[0, :1]) == bits(s[0, 1:2]) and bits(b[0, :1]) == bits(b[0, 1:2])
    larger = equal.copy(); larger[500] = 1.5
    got = run(w, 10, prior=larger, weight=5.0, queries=q0)
    assert same(got, host(w, 10, prior=larger, weight=5.0, queries=q0))
    i = got[2].cpu().numpy()
    assert i[0, 0] == 500 and 10 in i[0, 1:]


@pytest.mark.parametrize("dim", [64, 768])
def test_rows_with_a_non_finite_prior_are_hidden(dim):
    w = base(dim)
    p = w["prior"].copy()
    p[10], p[11], p[12] = np.nan, np.inf, -np.inf
    p[64:128] = np.nan                                           # a whole group
    got = run(w, 32, prior=p)
    assert same(got, host(w, 32, prior=p))
    s, b, i = (t.cpu().numpy() for t in got)
    assert not np.isnan(s).any() and not np.isnan(b).any()
    assert not (set(i.ravel().tolist()) & ({10, 11, 12} | set(range(64, 128))))
    assert i[0, 0] == 500                                        # the twin of the hidden row 10 answers query 0
    for bad in (np.nan, np.inf, -np.inf):
        s, b, i = (t.cpu().numpy() for t in run(w, 10, prior=np.full(N, bad, np.float32)))
        assert np.isneginf(s).all() and np.isneginf(b).all() and (i == -1).all()
    for path in (1, 2):
        assert same(run(w, 32, prior=p, path=path), host(w, 32, prior=p))


@pytest.mark.parametrize("dim", [64, 768])
def test_allow_bitmaps(dim):
    w = base(dim)
    rs = np.random.RandomState(7)
    half = rs.rand(N) < 0.5
    single = np.zeros(N, bool); single[777] = True
    holes = np.ones(N, bool); holes[64:256] = False; holes[320:384] = False; holes[960:] = False       # whole 64-row words of zeros
    garbage = pack_bitmap(np.ones(N, bool)).copy()
    garbage[-1] |= np.uint64(0xffffff) << np.uint64(40)         # bits at rows 1000..1023 set: they name no row
    for name, words, mask in (("half", pack_bitmap(half), half), ("single", pack_bitmap(single), single),
                              ("empty", pack_bitmap(np.zeros(N, bool)), np.zeros(N, bool)), ("garbage", garbage, np.ones(N, bool)),
                              ("holes", pack_bitmap(holes), holes)):
        want = host(w, 10, allow=mask)
        for kw in ({}, {"path": 1}, {"path": 2}, {"n_allowed": int(mask.sum())}):
            got = run(w, 10, allow=words.view(np.int64), **kw)
            assert same(got, want), (name, kw)
        i = want[2]
        assert mask[i[i >= 0]].all() and ((i >= 0).sum(axis=1) == min(10, int(mask.sum()))).all()


@pytest.mark.parametrize("k", (1, 10, 32))
@pytest.mark.parametrize("dim", [64, 768])
def test_the_path_the_list_size_and_the_batch_do_not_matter(dim, k):
    w = base(dim)
    want = host(w, k)
    idx = index(w)
    assert same(run(w, k, path=1), want) and idx.boosted_stats()[0] == 0
    assert same(run(w, k, path=2), want)
    assert same(run(w, k, path=1, cand_cap=1), want)            # every query with more than one candidate group overflows
    assert idx.boosted_stats()[0] > 0
    for q in (0, 1, 33, 69):
        alone = run(w, k, queries=slice(q, q + 1))
        assert same(alone, tuple(a[q:q + 1] for a in want)), q
    rev = np.arange(NQ)[::-1].copy()
    got = index(w).search_boosted(w["dQ"][torch.from_numpy(rev).to(DEV)].contiguous(), k, w["dprior"], w["weight"][rev])
    assert same(got, tuple(a[rev] for a in want))


@pytest.mark.parametrize("dim", [64, 768])
def test_near_ties_across_groups(dim):
    """prior = -base(q0, .): with weight 1 every boosted score of query 0 is 0 or a few ulps from it, with weight 0.5 half of the cosine
    is cancelled.  Every group is then within the tolerance of the k-th group maximum: query 0 is rescored widely or overflows."""
    w = base(dim)
    p = -w["B"][:, 0].astype(np.float32)
    idx = index(w)
    for wt in (1.0, 0.5):
        weight = np.full(NQ, wt, np.float32)
        want = host(w, 10, prior=p, weight=weight)
        assert same(run(w, 10, prior=p, weight=weight), want), wt
        got = run(w, 10, prior=p, weight=weight, queries=slice(0, 1), path=1)
        assert same(got, tuple(a[0:1] for a in want)), wt
        over, cands = idx.boosted_stats()
        print(f"dim={dim} weight={wt}: query 0 overflowed={over} candidate groups={cands}")
        assert over + cands > 0
        if wt == 1.0:                                            # every boosted score of query 0 within a few ulps of 0: rescored widely
            run(w, 10, queries=slice(0, 1), path=1)
            usual = idx.boosted_stats()[1]                       # the same query under the uniform prior
            assert over > 0 or (cands > 10 and cands > usual), (over, cands, usual)
        assert same(run(w, 10, prior=p, weight=weight, path=1, cand_cap=2), want), wt


def test_many_groups():
    n, dim, k, nq = 2 ** 18 + 300, 64, 10, 8
    rs = np.random.RandomState(5)
    X = (rs.randn(n, dim).astype(np.float32) / np.sqrt(dim) + 0.05).astype(np.float16)
    Q = (rs.randn(nq, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
    prior = rs.rand(n).astype(np.float32)
    weight = WEIGHTS[np.arange(nq) % len(WEIGHTS)]
    want = BO.boosted_host(X, Q, prior, weight, k)
    idx = ShardIndex(dev(X, np.float16), prefilter=None)
    dQ, dp = dev(Q, np.float16), dev(prior, np.float32)
    assert same(idx.search_boosted(dQ, k, dp, weight), want)
    assert same(idx.search_boosted(dQ, k, dp, weight, path=1, cand_cap=8), want)
    assert same(idx.search_boosted(dQ, k, dp, weight, path=2), want)


def test_idx_base_shifts_the_ids_and_empty_inputs_pad():
    w = base(64)
    idx = ShardIndex(w["dX"], idx_base=5000, prefilter=None)
    s, b, i = idx.search_boosted(w["dQ"], 10, w["dprior"], w["weight"])
    want = host(w, 10)
    assert same((s, b, i - 5000), want)
    s, b, i = idx.search_boosted(w["dQ"][:0].contiguous(), 10, w["dprior"], 0.5)
    assert s.shape == (0, 10) and b.shape == (0, 10) and i.shape == (0, 10)
    with pytest.raises(TypeError):
        idx.search_boosted(w["dQ"], 10, w["dprior"], 0.5, paht=1)


def test_the_wrapper_refuses_bad_weights_and_priors():
    w = base(64)
    idx = index(w)
    for weight in (np.nan, np.inf, [0.1] * (NQ - 1), "x", 1e39):
        with pytest.raises(ValueError, match="weight"):
            idx.search_boosted(w["dQ"], 10, w["dprior"], weight)
    big = np.full(N, 3e38, np.float32)
    with pytest.raises(ValueError, match="not finite"):
        idx.search_boosted(w["dQ"], 10, dev(big, np.float32), 2.0)
    with pytest.raises(ValueError, match="prior"):
        idx.search_boosted(w["dQ"], 10, w["dprior"][:-1].contiguous(), 0.5)
    with pytest.raises(ValueError, match="k="):
        idx.search_boosted(w["dQ"], 33, w["dprior"], 0.5)


def test_the_library_refuses_bad_arguments_before_any_launch():
    w = base(64)
    lib = _lib.load()
    X, Q, prior = w["dX"], w["dQ"], w["dprior"]
    weight = dev(w["weight"], np.float32)
    s = torch.empty((NQ, 32), dtype=torch.float32, device=DEV)
    b = torch.empty((NQ, 32), dtype=torch.float32, device=DEV)
    i = torch.empty((NQ, 32), dtype=torch.int64, device=DEV)
    allow = dev(pack_bitmap(np.ones(N, bool)).view(np.int64), np.int64)
    ws = torch.empty(lib.arx_topk_search_boosted_workspace_bytes(N, NQ, 64, 32), dtype=torch.uint8, device=DEV)

    def call(x_p=X.data_ptr(), n_rows=N, prior_p=prior.data_ptr(), mx=1.0, w_p=weight.data_ptr(), allow_p=allow.data_ptr(), n_allowed=-1,
             q_p=Q.data_ptr(), nq=NQ, dim=64, k=10, s_p=s.data_ptr(), b_p=b.data_ptr(), i_p=i.data_ptr(), ws_p=ws.data_ptr(),
             ws_bytes=ws.numel(), path=0, cand_cap=0):
        rc = lib.arx_topk_search_boosted(x_p, n_rows, prior_p, mx, w_p, allow_p, n_allowed, q_p, nq, dim, k, s_p, b_p, i_p, 0, 0.0, ws_p,
                                         ws_bytes, path, cand_cap, None)
        return rc, lib.arx_last_error().decode()
    assert call()[0] == 0 and call(allow_p=None)[0] == 0
    for kw, part in ((dict(x_p=None), "null"), (dict(prior_p=None), "null"), (dict(w_p=None), "null"), (dict(q_p=None), "null"),
                     (dict(s_p=None), "null"), (dict(b_p=None), "null"), (dict(i_p=None), "null"), (dict(ws_p=None), "null"),
                     (dict(x_p=X.data_ptr() + 2), "aligned"), (dict(q_p=Q.data_ptr() + 8), "aligned"), (dict(prior_p=prior.data_ptr() + 4), "aligned"),
                     (dict(w_p=weight.data_ptr() + 2), "aligned"), (dict(s_p=s.data_ptr() + 2), "aligned"), (dict(b_p=b.data_ptr() + 1), "aligned"),
                     (dict(i_p=i.data_ptr() + 4), "aligned"), (dict(allow_p=allow.data_ptr() + 4), "aligned"), (dict(ws_p=ws.data_ptr() + 8), "aligned"),
                     (dict(k=0), "k="), (dict(k=33), "k="), (dict(dim=96), "dim"), (dict(dim=8256), "dim"), (dict(dim=0), "dim"),
                     (dict(n_rows=-1), "negative"), (dict(nq=-1), "negative"), (dict(n_rows=0), "empty"), (dict(nq=0), "empty"),
                     (dict(n_allowed=N + 1), "n_allowed"), (dict(mx=-1.0), "max_abs_prior"), (dict(mx=float("inf")), "max_abs_prior"),
                     (dict(mx=float("nan")), "max_abs_prior"), (dict(path=3), "path"), (dict(cand_cap=-1), "cand_cap"),
                     (dict(ws_bytes=64, k=32), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and part in msg, (kw, msg)
    f = lib.arx_topk_search_boosted_workspace_bytes
    assert f(1000, 64, 768, 10) > 0 and f(1000, 5000, 64, 32) == f(1000, 1024, 64, 32)
    assert [f(1000, 64, 768, 33), f(1000, 64, 768, 0), f(1000, 64, 100, 10), f(1000, 64, 8256, 10), f(0, 1, 64, 1), f(-1, 1, 64, 1), f(10, 0, 64, 1)] == [-1] * 7
    torch.cuda.synchronize()


def test_prior_info():
    lib = _lib.load()
    idx = index(base(64))
    p = np.linspace(-3.0, 2.0, 100003).astype(np.float32)
    p[[5, 77777]] = np.nan; p[[6, 99]] = np.inf; p[100002] = -np.inf
    p[4242] = -7.25
    assert idx.prior_info(dev(p, np.float32)) == (7.25, 5)
    assert idx.prior_info(dev(np.zeros(10, np.float32), np.float32)) == (0.0, 0)
    assert idx.prior_info(dev(np.full(3, np.nan, np.float32), np.float32)) == (0.0, 3)
    out = torch.full((2,), 9, dtype=torch.int64, device=DEV)
    d = dev(p, np.float32)
    assert lib.arx_prior_info(d.data_ptr(), 0, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
    for args, part in (((None, 10, out.data_ptr()), "null"), ((d.data_ptr(), 10, None), "null"), ((d.data_ptr(), -1, out.data_ptr()), "negative"),
                       ((d.data_ptr() + 2, 10, out.data_ptr()), "aligned"), ((d.data_ptr(), 10, out.data_ptr() + 4), "aligned")):
        assert lib.arx_prior_info(*args, None) != 0 and part in lib.arx_last_error().decode(), args
