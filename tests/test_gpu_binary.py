"""arx_binary_pack / arx_binary_candidates (csrc/binary.hip) and `binary.BinaryIndex` on the device (-m gpu).  Every comparison is
exact: codes word for word, candidate rows, distances and counts against the numpy restatement (`binary.pack_host`,
`candidates_host`), score bits and ids against `search_host` and against the existing filtered search over the candidates' bitmap."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib
from arxiv_rag_amd import binary as B
from arxiv_rag_amd.index import ShardIndex
from arxiv_rag_amd.where import pack_bitmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NQ = 1000, 70                                                # 70 queries: nine tiles of 8, the last one ragged; 1000 rows: four rounds of 256
RS = (1, 10, 32, 256)
N_ROWS = (1, 63, 64, 65, 1000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host_of(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(host_of(got), want))


_BASE = {}


def base(dim):
    """The shard of one dim, its queries, centre, codes and the host answers, computed once and shared."""
    if dim not in _BASE:
        rs = np.random.RandomState(dim)
        X = (rs.randn(N, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        X[500] = X[10]                                           # two identical rows ...
        Q = (rs.randn(NQ, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        Q[0] = X[10]                                             # ... and a query equal to them
        centre = X.astype(np.float32).mean(axis=0)
        codes, qcodes = B.pack_host(X, centre), B.pack_host(Q, centre)
        w = dict(X=X, Q=Q, centre=centre, codes=codes, qcodes=qcodes, host={}, dX=dev(X, np.float16), dQ=dev(Q, np.float16),
                 dcodes=dev(codes.view(np.int64), np.int64), dqcodes=dev(qcodes.view(np.int64), np.int64))
        w["index"] = ShardIndex(w["dX"], prefilter=None)
        w["binary"] = B.BinaryIndex(w["index"], w["dcodes"], dev(centre, np.float32))
        _BASE[dim] = w
    return _BASE[dim]


def host(w, R, n=N):
    if (R, n) not in w["host"]:
        w["host"][(R, n)] = B.candidates_host(w["codes"][:n], w["qcodes"], R)
    return w["host"][(R, n)]


def run(w, R, n=N, allow=None, qcodes=None, **kw):
    return B.candidates_device(w["dcodes"][:n].contiguous(), w["dqcodes"] if qcodes is None else qcodes, R,
                               allow=None if allow is None else dev(allow, np.int64), **kw)


# ---- pack -----------------------------------------------------------------------------------------------------------------------------
def _special(X):
    X = X.copy()
    X[0, :6] = (np.nan, np.inf, -np.inf, 0.0, -0.0, 65504.0)
    X[1, -3:] = (np.nan, -0.0, np.inf)
    return X


@pytest.mark.parametrize("dim", [64, 768])
def test_pack_equals_the_definition(dim):
    w = base(dim)
    X, Q = _special(w["X"]), _special(w["Q"])
    centre = w["centre"].copy()
    centre[5] = np.inf
    X[2] = centre.astype(np.float16)
    X[3] = w["centre"].astype(np.float16)                        # equal to the centre wherever the centre is an fp16 value
    for c in (None, np.zeros(dim, np.float32), w["centre"], centre):
        dc = None if c is None else dev(c, np.float32)
        for A in (X, Q, X[:1], X[:65], X[:0]):
            got = B.pack_device(dev(A, np.float16).reshape(-1, dim), dc).cpu().numpy().view(np.uint64)
            assert np.array_equal(got, B.pack_host(A, c)), (dim, A.shape)
    assert np.array_equal(B.BinaryIndex.build(w["index"], centre=w["centre"]).codes.cpu().numpy().view(np.uint64), w["codes"])
    built = B.BinaryIndex.build(w["index"], centre="mean")       # the stored mean is what the codes were packed with
    assert np.array_equal(built.codes.cpu().numpy().view(np.uint64), B.pack_host(w["X"], built.centre.cpu().numpy()))
    assert np.allclose(built.centre.cpu().numpy(), w["centre"], atol=1e-4)
    assert B.BinaryIndex.build(w["index"], centre=None).centre is None


def test_pack_at_dim_8192():
    rs = np.random.RandomState(1)
    X = _special((rs.randn(70, 8192) * 0.1).astype(np.float16))
    centre = (rs.randn(8192) * 0.05).astype(np.float32)
    for c in (None, centre):
        got = B.pack_device(dev(X, np.float16), None if c is None else dev(c, np.float32)).cpu().numpy().view(np.uint64)
        assert got.shape == (70, 128) and np.array_equal(got, B.pack_host(X, c))


# ---- candidates -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("dim", [64, 768])
def test_candidates_equal_the_definition(dim, n):
    w = base(dim)
    for R in RS:
        got, want = run(w, R, n), host(w, R, n)
        assert same(got, want), (dim, n, R)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int64
        assert (want[2] == min(R, n)).all()


def test_cuts_fall_inside_runs_of_ties_and_ties_go_to_the_lower_row():
    w = base(64)                                                 # distances in 0..64 over 1000 rows: long runs of equal distances
    cand, dist, _ = host(w, 256)
    d_all = B.distances_host(w["codes"], w["qcodes"])
    for R in (1, 10, 32, 256):
        inside = sum(int((d_all[q] == dist[q, R - 1]).sum()) > int((dist[q, :R] == dist[q, R - 1]).sum()) for q in range(NQ))
        assert inside >= 1 if R == 1 else inside > NQ // 2, (R, inside)      # the cut drops rows at the distance of the last one kept
    assert cand[0, :2].tolist() == [10, 500] and dist[0, :2].tolist() == [0, 0]
    got = host_of(run(w, 256))
    assert np.array_equal(got[0], cand) and np.array_equal(got[1], dist)
    for q in range(NQ):
        for a in range(255):
            assert (dist[q, a], cand[q, a]) < (dist[q, a + 1], cand[q, a + 1])


@pytest.mark.parametrize("dim", [64, 768])
def test_shorter_lists_are_prefixes_and_the_launch_shape_does_not_matter(dim):
    w = base(dim)
    full = host_of(run(w, 256))
    for R in (1, 10, 32):
        c, d, n = host_of(run(w, R))
        assert np.array_equal(c, full[0][:, :R]) and np.array_equal(d, full[1][:, :R]) and (n == R).all()
    for R in (10, 256):
        for rpb in (64, 128, 1024):
            assert same(run(w, R, rows_per_block=rpb), host(w, R)), (R, rpb)
    no_dist = run(w, 10, want_dist=False)
    assert no_dist[1] is None and np.array_equal(no_dist[0].cpu().numpy(), host(w, 10)[0])


@pytest.mark.parametrize("dim", [64, 768])
def test_a_query_alone_and_the_batch_reversed_give_the_same_rows(dim):
    w = base(dim)
    want = host(w, 32)
    rev = host_of(run(w, 32, qcodes=w["dqcodes"].flip(0).contiguous()))
    assert all(np.array_equal(r[::-1], x) for r, x in zip(rev, want))
    for q in range(NQ):
        one = host_of(run(w, 32, qcodes=w["dqcodes"][q:q + 1].contiguous()))
        assert all(np.array_equal(o[0], x[q]) for o, x in zip(one, want)), q


def test_more_candidates_than_rows_returns_every_visible_row():
    w = base(64)
    c, d, n = host_of(run(w, 256, 200))
    assert (n == 200).all() and (c[:, 200:] == -1).all() and (d[:, 200:] == -1).all()
    assert all(sorted(c[q, :200].tolist()) == list(range(200)) for q in range(NQ))
    assert same((torch.from_numpy(c), torch.from_numpy(d), torch.from_numpy(n)), host(w, 256, 200))
    e = host_of(run(w, 5, 0))                                    # an empty shard is legal
    assert (e[0] == -1).all() and (e[1] == -1).all() and (e[2] == 0).all()


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
        for R in (10, 256):
            got = run(w, R, allow=words.view(np.int64))
            want = B.candidates_host(w["codes"], w["qcodes"], R, mask)
            assert same(got, want), (name, R)
            assert (want[2] == min(R, int(mask.sum()))).all()
            c = got[0].cpu().numpy()
            assert mask[c[c >= 0]].all()
    assert same(run(w, 10, rows_per_block=64, allow=pack_bitmap(holes).view(np.int64)), B.candidates_host(w["codes"], w["qcodes"], 10, holes))


def test_the_library_refuses_bad_arguments_before_any_launch():
    w = base(64)
    lib = _lib.load()
    codes, qc = w["dcodes"], w["dqcodes"]
    cand = torch.empty((NQ, 256), dtype=torch.int32, device=DEV)
    count = torch.empty(NQ, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.arx_binary_workspace_bytes(N, NQ, 64, 256), dtype=torch.uint8, device=DEV)

    def call(n_rows=N, dim=64, nq=NQ, R=10, codes_p=codes.data_ptr(), qc_p=qc.data_ptr(), allow_p=None, cand_p=cand.data_ptr(),
             count_p=count.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=ws.numel(), rpb=0):
        rc = lib.arx_binary_candidates_tuned(codes_p, n_rows, dim, qc_p, nq, allow_p, R, cand_p, None, count_p, ws_p, ws_bytes, rpb, None)
        return rc, lib.arx_last_error().decode()
    assert call()[0] == 0
    for kw, part in ((dict(R=0), "n_candidates"), (dict(R=257), "n_candidates"), (dict(dim=96), "dim"), (dict(dim=8256), "dim"), (dict(dim=0), "dim"),
                     (dict(n_rows=-1), "n_rows"), (dict(n_rows=1 << 31), "n_rows"), (dict(nq=0), "n_queries"), (dict(rpb=100), "rows_per_block"),
                     (dict(codes_p=None), "null"), (dict(qc_p=None), "null"), (dict(cand_p=None), "null"), (dict(count_p=None), "null"),
                     (dict(ws_p=None), "null"), (dict(codes_p=codes.data_ptr() + 8), "aligned"), (dict(qc_p=qc.data_ptr() + 4), "aligned"),
                     (dict(cand_p=cand.data_ptr() + 2), "aligned"), (dict(ws_bytes=64, R=256), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and part in msg, (kw, msg)
    x = w["dX"]
    out = torch.empty((N, 1), dtype=torch.int64, device=DEV)
    for args, part in (((x.data_ptr(), N, 96, None, out.data_ptr()), "dim"), ((x.data_ptr(), -1, 64, None, out.data_ptr()), "n_rows"),
                       ((None, N, 64, None, out.data_ptr()), "null"), ((x.data_ptr(), N, 64, None, None), "null"),
                       ((x.data_ptr(), N, 64, None, out.data_ptr() + 4), "aligned")):
        assert lib.arx_binary_pack(*args, None) != 0 and part in lib.arx_last_error().decode(), args
    assert lib.arx_binary_pack(None, 0, 64, None, None, None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="n_candidates"):
        w["binary"].candidates(w["dQ"], 257)
    with pytest.raises(ValueError, match="below k"):
        w["binary"].search(w["dQ"], 10, 5)


# ---- search ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 10, 32))
@pytest.mark.parametrize("dim", [64, 768])
def test_search_equals_the_definition_and_the_filtered_search_over_the_candidates(dim, k):
    w = base(dim)
    R = 40
    s, i, n = host_of(w["binary"].search(w["dQ"], k, R))
    ws, wi, wn = B.search_host(w["X"], w["codes"], w["qcodes"], w["Q"], k, R)
    assert np.array_equal(bits(s), bits(ws)) and np.array_equal(i, wi) and np.array_equal(n, wn)
    cand = host(w, R)[0]
    for q in range(NQ):                                          # query by query: the exact search under the bitmap of C(q)
        mask = np.zeros(N, bool); mask[cand[q]] = True
        fs, fi = w["index"].search(w["dQ"][q:q + 1].contiguous(), k, allow=dev(pack_bitmap(mask).view(np.int64), np.int64))
        assert np.array_equal(bits(fs.cpu().numpy()), bits(s[q:q + 1])) and np.array_equal(fi.cpu().numpy(), i[q:q + 1]), (q, k)
    assert i[0, 0] == 10 and (k == 1 or i[0, 1] == 500)


@pytest.mark.parametrize("dim", [64, 768])
def test_every_row_a_candidate_is_the_exact_search_and_idx_base_shifts_the_ids(dim):
    w = base(dim)
    small = ShardIndex(w["dX"][:200].contiguous(), prefilter=None)
    bi = B.BinaryIndex.build(small, centre="mean")
    q = w["dQ"]
    s, i, n = bi.search(q, 10, 256)
    es, ei = small.search(q, 10)
    assert torch.equal(s.view(torch.int32), es.view(torch.int32)) and torch.equal(i, ei) and (n == 200).all()
    mask = np.random.RandomState(3).rand(200) < 0.3
    allow = dev(pack_bitmap(mask).view(np.int64), np.int64)
    s, i, n = bi.search(q, 10, 256, allow=allow)
    es, ei = small.search(q, 10, allow=allow)
    assert torch.equal(s.view(torch.int32), es.view(torch.int32)) and torch.equal(i, ei) and (n == int(mask.sum())).all()
    shifted = B.BinaryIndex(ShardIndex(w["dX"][:200].contiguous(), idx_base=5000, prefilter=None), bi.codes, bi.centre)
    s2, i2, n2 = shifted.search(q, 10, 40)
    s1, i1, n1 = bi.search(q, 10, 40)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(i1 + 5000, i2) and torch.equal(n1, n2)
    c1, c2 = bi.candidates(q, 40)[0], shifted.candidates(q, 40)[0]
    assert torch.equal(c1, c2)                                   # the candidate rows are local
