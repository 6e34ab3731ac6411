"""The numpy restatement of the product-quantised search (`pq.encode_host`, `lut_host`, `candidates_host`), every Python-side refusal
and the exports of `arx_pq_encode` / `arx_pq_lut` / `arx_pq_candidates` (no GPU; INTEGRATION.md "Product-quantised search").  The C
entry points' argument refusals need the HIP runtime loaded and are checked in tests/test_gpu_pq.py."""
import argparse
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import pq as P
from arxiv_rag_amd.where import pack_bitmap

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_pq_encode": 8, "arx_pq_lut": 7, "arx_pq_workspace_bytes": 5, "arx_pq_candidates": 14, "arx_pq_candidates_tuned": 15}


# ---- exports ------------------------------------------------------------------------------------------------------------------------
def test_the_new_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        proto = re.search(rf"^int(?:32|64)_t {name}\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(_lib.EXPORTS[name][1]), name
        assert hasattr(lib, name), name
    bound = _lib.load()
    ws = bound.arx_pq_workspace_bytes
    for legal in ((0, 1, 64, 8, 1), (1000, 70, 768, 8, 256), (10_000_000, 64, 768, 8, 256), (5000, 9, 2048, 8, 40), (100, 1, 8192, 64, 10),
                  (100, 1, 64, 64, 10), (100, 1, 1024, 4, 10)):
        assert ws(*legal) > 0, legal
    assert ws(10_000_000, 1024, 768, 8, 256) <= 64 << 20
    for bad in ((100, 1, 64, 3, 10), (100, 1, 8192, 128, 10), (100, 1, 2112, 8, 10), (100, 1, 96, 8, 10), (100, 1, 64, 8, 0),
                (100, 1, 64, 8, 257), (-1, 1, 64, 8, 10), (100, 0, 64, 8, 10), (1 << 31, 1, 64, 8, 10), (100, 1, 2048, 4, 10)):
        assert ws(*bad) == -1, bad
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert " pq " in build and "$BLD/pq.o" in build and "$f = pq" in build       # built, linked, and without FMA contraction


# ---- encode -------------------------------------------------------------------------------------------------------------------------
def _codebooks(M, dsub, seed):
    return np.random.RandomState(seed).randn(M, 256, dsub).astype(np.float32)


def _encode_loop(X, cb, centre):
    """the definition, one scalar operation at a time"""
    M, _, dsub = cb.shape
    out = np.zeros((X.shape[0], M), np.uint8)
    with np.errstate(all="ignore"):
        for r in range(X.shape[0]):
            for m in range(M):
                best, code = None, 0
                for j in range(256):
                    acc = np.float32(0)
                    for t in range(dsub):
                        v = np.float32(X[r, m * dsub + t])
                        if centre is not None:
                            v = np.float32(v - centre[m * dsub + t])
                        e = np.float32(v - cb[m, j, t])
                        acc = np.float32(acc + np.float32(e * e))
                    if j == 0:
                        best = acc
                    elif acc < best:
                        best, code = acc, j
                out[r, m] = code
    return out


def test_encode_host_on_hand_made_cases():
    dim, dsub = 64, 8
    M = dim // dsub
    cb = _codebooks(M, dsub, 1)
    cb[:, 200] = cb[:, 17]                                       # two identical centroids in every subspace
    X = np.zeros((4, dim), np.float16)
    X[0] = cb[:, 17].reshape(-1).astype(np.float16)              # nearest to centroid 17 = centroid 200: the lower one wins
    X[1] = np.nan                                                # every distance NaN: code 0
    X[2] = cb[:, 3].reshape(-1).astype(np.float16)
    X[3, :8] = np.inf                                            # inf - finite = inf for every centroid: nothing is below d_0
    codes = P.encode_host(X, cb)
    assert codes.dtype == np.uint8 and codes.shape == (4, M)
    assert (codes[0] == 17).all() and (codes[1] == 0).all() and (codes[2] == 3).all() and codes[3, 0] == 0
    assert np.array_equal(codes, _encode_loop(X, cb, None))
    centre = (cb[:, 3] - cb[:, 90]).reshape(-1).astype(np.float16).astype(np.float32)           # x - centre lands near centroid 90
    shifted = P.encode_host(X, cb, centre)
    assert (shifted[2] == 90).all() and not np.array_equal(shifted, codes)
    assert np.array_equal(shifted, _encode_loop(X, cb, centre))
    rs = np.random.RandomState(2)
    Y = rs.randn(3, dim).astype(np.float16)
    assert np.array_equal(P.encode_host(Y, cb, centre), _encode_loop(Y, cb, centre))
    nan_first = cb.copy()
    nan_first[0, 0] = np.nan                                     # (not a legal codebook: the restatement still follows the definition)
    assert (P.encode_host(Y, nan_first)[:, 0] == 0).all()
    assert P.encode_host(X[:0], cb).shape == (0, M)
    with pytest.raises(ValueError):
        P.encode_host(X.astype(np.float32), cb)


# ---- lut ----------------------------------------------------------------------------------------------------------------------------
def test_lut_host_on_hand_made_cases():
    dim, dsub = 64, 8
    M = dim // dsub
    cb = _codebooks(M, dsub, 3)
    Q = np.random.RandomState(4).randn(3, dim).astype(np.float16)
    Q[1] = 0                                                     # a zero query: every inner product 0, a constant table
    lut = P.lut_host(Q, cb)
    assert lut.dtype == np.uint8 and lut.shape == (3, M, 256)
    assert not lut[1].any()
    f = P.lut_float_host(Q, cb)
    spans = f[0].max(axis=1) - f[0].min(axis=1)
    widest = int(np.argmax(spans))
    assert lut[0, widest].min() == 0 and lut[0, widest].max() == 255 and (lut[0].min(axis=1) == 0).all()
    assert lut[0, widest, int(np.argmin(f[0, widest]))] == 0 and lut[0, widest, int(np.argmax(f[0, widest]))] == 255
    for m in range(M):                                           # against the scalar definition
        for j in (0, 5, 255):
            acc = np.float32(0)
            for t in range(dsub):
                acc = np.float32(acc + np.float32(np.float32(Q[0, m * dsub + t]) * cb[m, j, t]))
            assert acc == f[0, m, j]
            inv = np.float32(np.float32(255) / np.float32(spans.max()))
            assert lut[0, m, j] == min(255, int(np.rint(np.float32(np.float32(acc - f[0, m].min()) * inv))))
    const = np.full((2, M, 256), 1.5, np.float32)
    assert not P.quantise_host(const).any()
    one_inf = f.copy()
    one_inf[2, 3, 7] = np.inf
    got = P.quantise_host(one_inf)
    assert not got[2].any() and np.array_equal(got[:2], lut[:2])
    one_nan = f.copy()
    one_nan[0, 0, 0] = np.nan
    assert not P.quantise_host(one_nan)[0].any()
    Qi = Q.copy()
    Qi[2, 5] = np.inf                                            # a query with an inf: its whole table is 0
    assert not P.lut_host(Qi, cb)[2].any()


# ---- candidates ---------------------------------------------------------------------------------------------------------------------
def test_candidates_host_against_a_brute_force_loop():
    n, M, nq = 200, 8, 5
    rs = np.random.RandomState(5)
    codes = rs.randint(0, 256, (n, M)).astype(np.uint8)
    lut = rs.randint(0, 4, (nq, M, 256)).astype(np.uint8)        # small bytes: many equal sums
    codes[77] = codes[12]
    mask = rs.rand(n) < 0.5
    garbage = pack_bitmap(np.ones(n, bool)).copy()
    garbage[-1] |= np.uint64(0xffff) << np.uint64(48)            # bits beyond n_rows
    s_all = P.sums_host(codes, lut)
    for allow, m in ((None, np.ones(n, bool)), (mask, mask), (pack_bitmap(mask), mask), (pack_bitmap(mask).view(np.int64), mask),
                     (np.zeros(n, bool), np.zeros(n, bool)), (garbage, np.ones(n, bool))):
        for R in (1, 7, 256):
            cand, sums, count = P.candidates_host(codes, lut, R, allow)
            assert cand.dtype == np.int32 and sums.dtype == np.int32 and count.dtype == np.int64
            for q in range(nq):
                tuples = sorted((-sum(int(lut[q, mm, codes[r, mm]]) for mm in range(M)), r) for r in range(n) if m[r])[:R]
                assert count[q] == len(tuples)
                assert [(-int(s), int(r)) for s, r in zip(sums[q, :count[q]], cand[q, :count[q]])] == tuples
                assert (cand[q, count[q]:] == -1).all() and (sums[q, count[q]:] == -1).all()
                assert all(s_all[q, r] == s for r, s in zip(cand[q, :count[q]], sums[q, :count[q]]))
    zero = P.candidates_host(codes, np.zeros_like(lut), 9)
    assert (zero[0] == np.arange(9)).all() and (zero[1] == 0).all()


# ---- quantisation does not cost recall ----------------------------------------------------------------------------------------------
def _lloyd(V, dsub, iters=8, seed=0):
    n, dim = V.shape
    M = dim // dsub
    rs = np.random.RandomState(seed)
    cb = np.zeros((M, 256, dsub), np.float32)
    for m in range(M):
        sub = V[:, m * dsub:(m + 1) * dsub]
        c = sub[rs.permutation(n)[:256]].copy()
        for _ in range(iters):
            d = (sub * sub).sum(1)[:, None] - 2 * sub @ c.T + (c * c).sum(1)[None, :]
            a = d.argmin(1)
            for j in range(256):
                if (a == j).any():
                    c[j] = sub[a == j].mean(0)
        cb[m] = c
    return cb


def test_the_byte_tables_do_not_cost_recall_against_float_adc():
    n, dim, dsub, nq, R, k = 4096, 64, 8, 32, 64, 10
    rs = np.random.RandomState(11)
    centres = rs.randn(32, dim)
    X = centres[rs.randint(0, 32, n)] + 0.6 * rs.randn(n, dim)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    Q = centres[rs.randint(0, 32, nq)] + 0.6 * rs.randn(nq, dim)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float16)
    mean = X.astype(np.float32).mean(0)
    cb = _lloyd(X.astype(np.float32) - mean, dsub)
    codes = P.encode_host(X, cb, mean)
    exact = np.argsort(-(Q.astype(np.float32) @ X.astype(np.float32).T), axis=1, kind="stable")[:, :k]
    f = P.lut_float_host(Q, cb)
    adc = np.zeros((nq, n), np.float32)
    for m in range(dim // dsub):
        adc += f[:, m, :][:, codes[:, m]]
    float_list = np.argsort(-adc, axis=1, kind="stable")[:, :R]
    byte_list = P.candidates_host(codes, P.lut_host(Q, cb), R)[0]

    def recall(lists):
        return np.mean([len(set(exact[q]) & set(lists[q])) / k for q in range(nq)])
    r_float, r_byte = recall(float_list), recall(byte_list)
    print(f"recall@10 float ADC {r_float:.3f}, byte tables {r_byte:.3f}")
    assert r_byte >= r_float - 0.05, (r_byte, r_float)
    assert r_float > 0.5                                         # the set-up is one where PQ works at all


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_check_args_dsub_and_codebooks():
    P.check_args(10, 10, 768, 8)
    P.check_args(None, 256)
    for k, R in ((10, 9), (0, 5), (33, 40), (1, 0), (1, 257), (1, 2.5), (True, 5)):
        with pytest.raises(ValueError):
            P.check_args(k, R)
    assert P.check_dsub(768, 8) == 96 and P.check_dsub(2048, 8) == 256 and P.check_dsub(64, 64) == 1 and P.check_dsub(8192, 32) == 256
    for dim, dsub in ((768, 3), (768, 128), (768, 2), (2112, 8), (96, 8), (8256, 64), (768, 8.0), (4096, 4)):
        with pytest.raises(ValueError):
            P.check_dsub(dim, dsub)
    cb = _codebooks(8, 8, 0)
    assert P.check_codebooks(cb.astype(np.float64), 64, 8).dtype == np.float32
    bad = cb.copy()
    bad[1, 2, 3] = np.inf
    for c, dim, dsub in ((bad, 64, 8), (cb, 128, 8), (cb[:, :255], 64, 8), (cb.astype(np.int32), 64, 8), (cb, 64, 4)):
        with pytest.raises(ValueError):
            P.check_codebooks(c, dim, dsub)
    with pytest.raises(ValueError, match="finite"):
        P.check_codebooks(bad, 64, 8)


def test_every_refusal_of_check_query_with_pq():
    ok = dict(has_index=True, n_width=10)
    P.check_query_with_pq(40, **ok)
    P.check_query_with_pq(10, **ok)
    P.check_query_with_pq(256, **ok)
    for kw, part in ((dict(nprobe=4), "nprobe"), (dict(binary_candidates=40), "binary_candidates"), (dict(hybrid_alpha=0.5), "hybrid_alpha"),
                     (dict(group_by="paper"), "group_by"), (dict(min_score=0.2), "min_score"), (dict(boost_weight=0.1), "boost_weight"),
                     (dict(per_query_filters=True), "per-query filter lists"), (dict(world=2), "world"), (dict(has_index=False), "build_pq")):
        with pytest.raises(ValueError, match=part):
            P.check_query_with_pq(40, **{**ok, **kw})
    for R in (9, 257, 0, 12.0):
        with pytest.raises(ValueError, match="n_candidates"):
            P.check_query_with_pq(R, **ok)
    from arxiv_rag_amd.binary import check_query_with_binary
    from arxiv_rag_amd.boost import check_query_with_boost
    with pytest.raises(ValueError, match="pq_candidates"):
        check_query_with_binary(40, has_index=True, n_width=10, pq_candidates=40)
    check_query_with_binary(40, has_index=True, n_width=10, pq_candidates=None)
    with pytest.raises(ValueError, match="pq_candidates"):
        check_query_with_boost(0.5, has_prior=True, pq_candidates=40)


def _cli_args(**kw):
    base = dict(pq_candidates=40, pq_dsub=8, pq_centre="mean", queries="q.txt", nprobe=None, ivf_lists=None, binary_candidates=None,
                hybrid_alpha=None, group_by_paper=False, min_score=None, where_filters=None, boost_key=None, top_k=10, rerank_model=None,
                rerank_top_k=32, mmr_lambda=None, mmr_fetch_k=32)
    base.update(kw)
    return argparse.Namespace(**base)


def test_every_refusal_of_check_pq_args(monkeypatch):
    from arxiv_rag_amd.generate_embeddings_parallel import check_pq_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert check_pq_args(_cli_args()) is None
    assert check_pq_args(_cli_args(pq_candidates=None)) is None
    assert check_pq_args(argparse.Namespace()) is None
    for kw, part in ((dict(pq_candidates=0), "[1, 256]"), (dict(pq_candidates=257), "[1, 256]"), (dict(pq_dsub=3), "--pq-dsub"),
                     (dict(pq_dsub=128), "--pq-dsub"), (dict(queries=None), "--queries"), (dict(nprobe=4), "--nprobe"),
                     (dict(ivf_lists=64), "--nprobe"), (dict(binary_candidates=40), "--binary-candidates"), (dict(hybrid_alpha=0.5), "--hybrid-alpha"),
                     (dict(group_by_paper=True), "--group-by-paper"), (dict(min_score=0.1), "--min-score"), (dict(where_filters=[{"year": 2020}]), "--where-file"),
                     (dict(boost_key="year"), "--boost-key"), (dict(pq_candidates=5), "below the 10 rows"),
                     (dict(pq_candidates=20, mmr_lambda=0.5), "below the 32 rows"), (dict(pq_candidates=20, rerank_model="m"), "below the 32 rows")):
        msg = check_pq_args(_cli_args(**kw))
        assert msg and part in msg, (kw, msg)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in check_pq_args(_cli_args())
