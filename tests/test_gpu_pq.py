"""arx_pq_encode / arx_pq_lut / arx_pq_candidates (csrc/pq.hip) and `pq.PqIndex` on the device (-m gpu).  Every comparison is exact:
code bytes, table bytes, candidate rows, sums and counts against the numpy restatement (`pq.encode_host`, `lut_host`,
`candidates_host`), score bits and ids against `search_host` and against the existing filtered search over the candidates' bitmap."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib
from arxiv_rag_amd import pq as P
from arxiv_rag_amd.index import ShardIndex
from arxiv_rag_amd.where import pack_bitmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((64, 4), (64, 8), (64, 64), (768, 8), (2048, 8))      # (dim, dsub): M = 16, 8, 1, 96, 256
N_ENC = (0, 1, 63, 64, 65, 1000)
MS = (1, 8, 96, 256)                                            # scan tiles of 8, 4, 2 and 1 queries; code loads of 1, 4 and 16 bytes
N_CAND = (0, 1, 64, 65, 1000, 5000)                             # 5000 rows: blocks of 2048 rows, whose lists are cut in mid-scan
NQ = 70


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host_of(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


# ---- encode and lut ---------------------------------------------------------------------------------------------------------------------
_ENC = {}


def enc_base(dim, dsub):
    """Rows, queries, a centre and codebooks of one shape, with the host codes of the 1000 rows, computed once and shared (a row's
    code does not depend on the other rows, so a prefix's codes are a prefix of them)."""
    if (dim, dsub) not in _ENC:
        M = dim // dsub
        rs = np.random.RandomState(dim + dsub)
        X = (rs.randn(1000, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        centre = X.astype(np.float32).mean(axis=0)               # (of the finite rows: taken before the special values go in)
        X[3, :5] = (np.nan, np.inf, -np.inf, -0.0, 65504.0)
        X[7] = np.nan
        X[64, -1] = np.inf
        X[999, 0] = -np.inf
        cb = np.ascontiguousarray((X[100:356].astype(np.float32) - centre).reshape(256, M, dsub).transpose(1, 0, 2))
        cb[:, 200] = cb[:, 17]                                   # duplicated centroids: the lower one wins
        cb[:, 255] = cb[:, 0]
        X[5] = (cb[:, 17].reshape(-1) + centre).astype(np.float16)
        Q = (rs.randn(9, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        Q[2] = 0                                                 # a zero query
        Q[4, dim // 2] = np.inf                                  # a query with an inf
        Q[5, 1] = np.nan
        _ENC[(dim, dsub)] = dict(X=X, Q=Q, centre=centre, cb=cb, dcb=dev(cb, np.float32), dcentre=dev(centre, np.float32),
                                 codes=P.encode_host(X, cb, centre), codes0=P.encode_host(X, cb, None), lut=P.lut_host(Q, cb))
    return _ENC[(dim, dsub)]


@pytest.mark.parametrize("dim,dsub", SHAPES)
def test_encode_equals_the_definition(dim, dsub):
    w = enc_base(dim, dsub)
    for n in N_ENC:
        x = dev(w["X"][:n], np.float16).reshape(n, dim)
        got = P.encode_device(x, dsub, w["dcentre"], w["dcb"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, dim // dsub)
        assert np.array_equal(got.cpu().numpy(), w["codes"][:n]), (dim, dsub, n, "centre")
        assert np.array_equal(P.encode_device(x, dsub, None, w["dcb"]).cpu().numpy(), w["codes0"][:n]), (dim, dsub, n, "no centre")
    assert (w["codes"][7] == 0).all()                            # a row of NaN
    assert (w["codes"][5] == 17).all() or dsub < 8               # (fp16 rounding of the row can move a 4-dimensional nearest)
    assert not (w["codes"] == 200).any() and not (w["codes"] == 255).any()
    assert not np.array_equal(w["codes"], w["codes0"])


@pytest.mark.parametrize("dim,dsub", SHAPES)
def test_lut_equals_the_definition(dim, dsub):
    w = enc_base(dim, dsub)
    for nq in (1, 9):
        got = P.lut_device(dev(w["Q"][:nq], np.float16), dsub, w["dcb"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (nq, dim // dsub, 256)
        assert np.array_equal(got.cpu().numpy(), w["lut"][:nq]), (dim, dsub, nq)
    assert not w["lut"][2].any() and not w["lut"][4].any() and not w["lut"][5].any()
    assert w["lut"][0].max() == 255 and w["lut"][0].min() == 0
    assert tuple(P.lut_device(dev(w["Q"][:0], np.float16).reshape(0, dim), dsub, w["dcb"]).shape) == (0, dim // dsub, 256)


# ---- candidates: random code bytes and random table bytes, the integer path on its own -------------------------------------------------------
_CAND = {}


def cand_base(M):
    if M not in _CAND:
        rs = np.random.RandomState(M)
        codes = rs.randint(0, 256, (5000, M)).astype(np.uint8)
        lut = rs.randint(0, 256, (NQ, M, 256)).astype(np.uint8)
        lut[1] = 0                                               # a table of zeros: rows 0 .. R - 1
        lut[2] = 255                                             # the largest sum there is, for every row
        lut[3] = 0
        lut[3, 0, :128] = 1                                      # sums 0 or 1: half of the rows tie at the top, every cut falls inside that run
        lut[4] = rs.randint(0, 2, (M, 256))                      # sums in 0 .. M: long runs of equal sums
        codes[4000] = codes[10]                                  # two identical rows
        _CAND[M] = dict(codes=codes, lut=lut, dcodes=dev(codes, np.uint8), dlut=dev(lut, np.uint8), host={})
    return _CAND[M]


def host(w, n, allow_key=None, allow=None):
    """`candidates_host` at R = 256 for the first n rows, once; a shorter list is a prefix by definition"""
    if (n, allow_key) not in w["host"]:
        w["host"][(n, allow_key)] = P.candidates_host(w["codes"][:n], w["lut"], 256, allow)
    return w["host"][(n, allow_key)]


def cut(full, R, qs=slice(None)):
    cand, sums, count = full
    return cand[qs, :R], sums[qs, :R], np.minimum(count[qs], R)


def run(w, R, n=5000, allow=None, lut=None, **kw):
    M = w["codes"].shape[1]
    dsub = 64 if M <= 128 else 8                                 # any legal dsub: the scan reads M alone
    return P.candidates_device(w["dcodes"][:n].contiguous(), w["dlut"] if lut is None else lut, dsub, R,
                               allow=None if allow is None else dev(allow, np.int64), **kw)


def same(got, want):
    return all(np.array_equal(g, x) for g, x in zip(host_of(got), want))


@pytest.mark.parametrize("M", MS)
def test_candidates_equal_the_definition(M):
    w = cand_base(M)
    for n in N_CAND:
        full = host(w, n)
        for R in (1, 40, 256):
            got = run(w, R, n)
            assert same(got, cut(full, R)), (M, n, R)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int64
        assert (full[2] == min(256, n)).all()
    full = host(w, 1000)
    for nq in (1, 8, 9):
        assert same(run(w, 40, 1000, lut=w["dlut"][:nq].contiguous()), cut(full, 40, slice(0, nq))), (M, nq)
    c, s, n = host_of(run(w, 256, 200))                           # R above the rows: every row, padded with -1
    assert (n == 200).all() and (c[:, 200:] == -1).all() and (s[:, 200:] == -1).all()
    assert all(sorted(c[q, :200].tolist()) == list(range(200)) for q in range(NQ))
    no_sum = run(w, 10, want_sum=False)
    assert no_sum[1] is None and np.array_equal(no_sum[0].cpu().numpy(), host(w, 5000)[0][:, :10])
    empty = run(w, 5, lut=w["dlut"][:0].contiguous())
    assert tuple(empty[0].shape) == (0, 5) and tuple(empty[2].shape) == (0,)


@pytest.mark.parametrize("M", MS)
def test_zero_tables_ties_and_prefixes(M):
    w = cand_base(M)
    cand, sums, _ = host(w, 5000)
    assert cand[1].tolist() == list(range(256)) and (sums[1] == 0).all()
    assert cand[2].tolist() == list(range(256)) and (sums[2] == 255 * M).all()
    s_all = P.sums_host(w["codes"], w["lut"])
    for R in (1, 40, 256):                                       # the cut drops rows at the sum of the last one kept
        inside = sum(int((s_all[q] == sums[q, R - 1]).sum()) > int((sums[q, :R] == sums[q, R - 1]).sum()) for q in range(NQ))
        assert inside >= 3, (M, R, inside)
    for q in range(NQ):
        assert all((-sums[q, a], cand[q, a]) < (-sums[q, a + 1], cand[q, a + 1]) for a in range(255))
    got = host_of(run(w, 256))
    assert np.array_equal(got[0], cand) and np.array_equal(got[1], sums)
    for R in (1, 40):
        c, s, n = host_of(run(w, R))
        assert np.array_equal(c, got[0][:, :R]) and np.array_equal(s, got[1][:, :R]) and (n == R).all()


@pytest.mark.parametrize("M", MS)
def test_the_launch_shape_the_batch_and_its_order_do_not_matter(M):
    w = cand_base(M)
    want = cut(host(w, 5000), 40)
    for rpb in (64, 256):
        assert same(run(w, 40, rows_per_block=rpb), want), (M, rpb)
    assert same(run(w, 256, rows_per_block=256), host(w, 5000)), M
    rev = host_of(run(w, 40, lut=w["dlut"].flip(0).contiguous()))
    assert all(np.array_equal(r[::-1], x) for r, x in zip(rev, want))
    for q in (0, 1, 3, 8, 69):
        one = host_of(run(w, 40, lut=w["dlut"][q:q + 1].contiguous()))
        assert all(np.array_equal(o[0], x[q]) for o, x in zip(one, want)), (M, q)
    big = torch.empty(1 << 26, dtype=torch.uint8, device=DEV)    # another workspace, larger than asked for
    assert same(run(w, 40, ws=big), want)


@pytest.mark.parametrize("M", (8, 96))
def test_allow_bitmaps(M):
    w = cand_base(M)
    N = 1000
    rs = np.random.RandomState(7)
    sparse = rs.rand(N) < 0.01
    holes = np.ones(N, bool); holes[64:256] = False; holes[320:384] = False; holes[960:] = False       # whole 64-row words of zeros
    garbage = pack_bitmap(np.ones(N, bool)).copy()
    garbage[-1] |= np.uint64(0xffffff) << np.uint64(40)         # bits at rows 1000..1023 set: they name no row
    for name, words, mask in (("ones", pack_bitmap(np.ones(N, bool)), np.ones(N, bool)), ("sparse", pack_bitmap(sparse), sparse),
                              ("zeros", pack_bitmap(np.zeros(N, bool)), np.zeros(N, bool)), ("garbage", garbage, np.ones(N, bool)),
                              ("holes", pack_bitmap(holes), holes)):
        full = host(w, N, name, mask)
        for R in (10, 256):
            got = run(w, R, N, allow=words.view(np.int64))
            assert same(got, cut(full, R)), (M, name, R)
            c = got[0].cpu().numpy()
            assert mask[c[c >= 0]].all()
        assert (full[2] == min(256, int(mask.sum()))).all()
    assert same(run(w, 10, N, allow=pack_bitmap(np.ones(N, bool)).view(np.int64)), cut(host(w, N), 10))
    assert same(run(w, 10, N, rows_per_block=64, allow=pack_bitmap(holes).view(np.int64)), cut(host(w, N, "holes", holes), 10))


def test_the_library_refuses_bad_arguments_before_any_launch():
    w = cand_base(8)
    lib = _lib.load()
    N, dim, dsub = 1000, 64, 8
    codes, lut = w["dcodes"][:N].contiguous(), w["dlut"]
    cand = torch.empty((NQ, 256), dtype=torch.int32, device=DEV)
    count = torch.empty(NQ, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.arx_pq_workspace_bytes(N, NQ, dim, dsub, 256), dtype=torch.uint8, device=DEV)

    def call(n_rows=N, dim=dim, dsub=dsub, nq=NQ, R=10, codes_p=codes.data_ptr(), lut_p=lut.data_ptr(), allow_p=None, cand_p=cand.data_ptr(),
             count_p=count.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=ws.numel(), rpb=0):
        rc = lib.arx_pq_candidates_tuned(codes_p, n_rows, dim, dsub, lut_p, nq, allow_p, R, cand_p, None, count_p, ws_p, ws_bytes, rpb, None)
        return rc, lib.arx_last_error().decode()
    assert call()[0] == 0
    assert call(nq=0)[0] == 0                                     # no queries: nothing is launched
    for kw, part in ((dict(R=0), "n_candidates"), (dict(R=257), "n_candidates"), (dict(dim=96), "dim"), (dict(dim=8256), "dim"), (dict(dim=0), "dim"),
                     (dict(dsub=3), "dsub"), (dict(dsub=128), "dsub"), (dict(dsub=2), "dsub"), (dict(dim=2112, dsub=8), "M="),
                     (dict(n_rows=-1), "n_rows"), (dict(n_rows=1 << 31), "n_rows"), (dict(nq=-1), "n_queries"), (dict(rpb=100), "rows_per_block"),
                     (dict(codes_p=None), "null"), (dict(lut_p=None), "null"), (dict(cand_p=None), "null"), (dict(count_p=None), "null"),
                     (dict(ws_p=None), "null"), (dict(codes_p=codes.data_ptr() + 8), "aligned"), (dict(lut_p=lut.data_ptr() + 4), "aligned"),
                     (dict(cand_p=cand.data_ptr() + 2), "aligned"), (dict(ws_p=ws.data_ptr() + 8), "ws must be 16-byte aligned"),
                     (dict(ws_bytes=64, R=256), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and part in msg, (kw, msg)
    e = enc_base(64, 8)
    x = dev(e["X"], np.float16)
    out = torch.empty((1000, 8), dtype=torch.uint8, device=DEV)
    cb = e["dcb"]
    for args, part in (((x.data_ptr(), 1000, 96, 8, None, cb.data_ptr(), out.data_ptr()), "dim"),
                       ((x.data_ptr(), 1000, 64, 3, None, cb.data_ptr(), out.data_ptr()), "dsub"),
                       ((x.data_ptr(), 1000, 2112, 8, None, cb.data_ptr(), out.data_ptr()), "M="),
                       ((x.data_ptr(), -1, 64, 8, None, cb.data_ptr(), out.data_ptr()), "n_rows"),
                       ((None, 1000, 64, 8, None, cb.data_ptr(), out.data_ptr()), "null"),
                       ((x.data_ptr(), 1000, 64, 8, None, None, out.data_ptr()), "null"),
                       ((x.data_ptr(), 1000, 64, 8, None, cb.data_ptr(), out.data_ptr() + 4), "aligned")):
        assert lib.arx_pq_encode(*args, None) != 0 and part in lib.arx_last_error().decode(), args
    assert lib.arx_pq_encode(None, 0, 64, 8, None, None, None, None) == 0
    q = dev(e["Q"], np.float16)
    tab = torch.empty((9, 8, 256), dtype=torch.uint8, device=DEV)
    for args, part in (((q.data_ptr(), 9, 96, 8, cb.data_ptr(), tab.data_ptr()), "dim"), ((q.data_ptr(), 9, 64, 5, cb.data_ptr(), tab.data_ptr()), "dsub"),
                       ((q.data_ptr(), -1, 64, 8, cb.data_ptr(), tab.data_ptr()), "n_queries"), ((None, 9, 64, 8, cb.data_ptr(), tab.data_ptr()), "null"),
                       ((q.data_ptr(), 9, 64, 8, cb.data_ptr() + 4, tab.data_ptr()), "aligned")):
        assert lib.arx_pq_lut(*args, None) != 0 and part in lib.arx_last_error().decode(), args
    assert lib.arx_pq_lut(None, 0, 64, 8, None, None, None) == 0
    torch.cuda.synchronize()
    for bad in (lambda: P.encode_device(x, 3, None, cb), lambda: P.encode_device(x, 8, None, cb[:, :255].contiguous()),
                lambda: P.lut_device(q.float(), 8, cb), lambda: P.candidates_device(codes.to(torch.int32), lut, 8, 10),
                lambda: P.candidates_device(codes, lut[:, :7].contiguous(), 8, 10)):
        with pytest.raises(ValueError):
            bad()


# ---- search ---------------------------------------------------------------------------------------------------------------------------
_SEARCH = {}
N = 1000


def search_base(dim):
    if dim not in _SEARCH:
        dsub = 8
        M = dim // dsub
        rs = np.random.RandomState(dim)
        X = (rs.randn(N, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        X[500] = X[10]
        Q = (rs.randn(NQ, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        Q[0] = X[10]
        centre = X.astype(np.float32).mean(axis=0)
        cb = np.ascontiguousarray((X[rs.permutation(N)[:256]].astype(np.float32) - centre).reshape(256, M, dsub).transpose(1, 0, 2))
        codes, lut = P.encode_host(X, cb, centre), P.lut_host(Q, cb)
        w = dict(X=X, Q=Q, cb=cb, centre=centre, codes=codes, lut=lut, dX=dev(X, np.float16), dQ=dev(Q, np.float16))
        w["index"] = ShardIndex(w["dX"], prefilter=None)
        w["pq"] = P.PqIndex.build(w["index"], dsub=dsub, centre=centre, codebooks=cb)
        _SEARCH[dim] = w
    return _SEARCH[dim]


@pytest.mark.parametrize("k", (1, 10, 32))
@pytest.mark.parametrize("dim", [64, 768])
def test_search_equals_the_definition_and_the_filtered_search_over_the_candidates(dim, k):
    w = search_base(dim)
    R = 40
    assert np.array_equal(w["pq"].codes.cpu().numpy(), w["codes"]) and np.array_equal(w["pq"].codebooks.cpu().numpy(), w["cb"])
    s, i, n = host_of(w["pq"].search(w["dQ"], k, R))
    ws, wi, wn = P.search_host(w["X"], w["codes"], w["lut"], w["Q"], k, R)
    assert np.array_equal(bits(s), bits(ws)) and np.array_equal(i, wi) and np.array_equal(n, wn)
    cand = P.candidates_host(w["codes"], w["lut"], R)[0]
    assert np.array_equal(w["pq"].candidates(w["dQ"], R)[0].cpu().numpy(), cand)
    for q in range(0, NQ, 7):                                    # query by query: the exact search under the bitmap of C(q)
        mask = np.zeros(N, bool); mask[cand[q]] = True
        fs, fi = w["index"].search(w["dQ"][q:q + 1].contiguous(), k, allow=dev(pack_bitmap(mask).view(np.int64), np.int64))
        assert np.array_equal(bits(fs.cpu().numpy()), bits(s[q:q + 1])) and np.array_equal(fi.cpu().numpy(), i[q:q + 1]), (q, k)
    assert i[0, 0] == 10 and (k == 1 or i[0, 1] == 500)


@pytest.mark.parametrize("dim", [64, 768])
def test_every_row_a_candidate_is_the_exact_search_and_idx_base_shifts_the_ids(dim):
    w = search_base(dim)
    small = ShardIndex(w["dX"][:200].contiguous(), prefilter=None)
    pi = P.PqIndex.build(small, dsub=8, centre="mean", codebooks=w["cb"])
    q = w["dQ"]
    s, i, n = pi.search(q, 10, 256)
    es, ei = small.search(q, 10)
    assert torch.equal(s.view(torch.int32), es.view(torch.int32)) and torch.equal(i, ei) and (n == 200).all()
    mask = np.random.RandomState(3).rand(200) < 0.3
    allow = dev(pack_bitmap(mask).view(np.int64), np.int64)
    s, i, n = pi.search(q, 10, 256, allow=allow)
    es, ei = small.search(q, 10, allow=allow)
    assert torch.equal(s.view(torch.int32), es.view(torch.int32)) and torch.equal(i, ei) and (n == int(mask.sum())).all()
    shifted = P.PqIndex(ShardIndex(w["dX"][:200].contiguous(), idx_base=5000, prefilter=None), pi.codes, pi.codebooks, pi.centre, 8)
    s2, i2, n2 = shifted.search(q, 10, 40)
    s1, i1, n1 = pi.search(q, 10, 40, rows_per_block=64)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(i1 + 5000, i2) and torch.equal(n1, n2)
    with pytest.raises(ValueError, match="n_candidates"):
        pi.candidates(q, 257)
    with pytest.raises(ValueError, match="below k"):
        pi.search(q, 10, 5)


# ---- training -------------------------------------------------------------------------------------------------------------------------
def test_training_runs_and_its_codebooks_are_kept_as_given():
    rs = np.random.RandomState(5)
    X = dev((rs.randn(2000, 64) / 8 + 0.05).astype(np.float16), np.float16)
    centre = X.float().mean(dim=0).contiguous()
    cb = P.train(X, 8, centre, iters=3, seed=1)
    assert tuple(cb.shape) == (8, 256, 8) and cb.dtype == torch.float32 and bool(torch.isfinite(cb).all())
    few = P.train(X[:100].contiguous(), 8, None, iters=2)        # fewer rows than codes: the remaining centroids repeat
    assert bool(torch.isfinite(few).all()) and int(P.encode_device(X, 8, None, few).max()) < 100
    index = ShardIndex(X, prefilter=None)
    pi = P.PqIndex.build(index, dsub=8, centre=centre, codebooks=cb)
    assert torch.equal(pi.codebooks, cb) and torch.equal(pi.centre, centre)
    assert torch.equal(pi.codes, pi.encode(X)) and torch.equal(pi.codes, P.encode_device(X, 8, centre, cb))
    assert np.array_equal(pi.codes.cpu().numpy(), P.encode_host(X.cpu().numpy(), cb.cpu().numpy(), centre.cpu().numpy()))
    trained = P.PqIndex.build(index, dsub=8, centre="mean", train_rows=500, iters=2, seed=3)
    assert bool(torch.isfinite(trained.codebooks).all()) and tuple(trained.codes.shape) == (2000, 8)
    s, i, n = trained.search(X[:5].contiguous(), 1, 40)
    assert i[:, 0].tolist() == [0, 1, 2, 3, 4] and (n == 40).all()      # a row finds itself among its 40 candidates
    with pytest.raises(ValueError):
        P.PqIndex.build(index, dsub=8, codebooks=cb[:, :, :4])
    with pytest.raises(ValueError):
        P.PqIndex.build(index, dsub=3)
