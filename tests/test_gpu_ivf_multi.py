"""arx_ivf_search_multi / arx_ivf_search_multi_tuned (csrc/ivf.hip) and `ivf.IvfIndex.search_many` on the device (-m gpu): the IVF probe
search with a row filter per query and a score threshold per query.  Every comparison is exact: scores as uint32 bits, ids, `scanned`
and `hits` with array_equal, against the numpy restatement (`ivf.search_many_host`), against `arx_ivf_search` with one bitmap, against
the filtered and the range search over the probe bitmaps.  The lists are hand-built (no k-means involved), the shapes those of
tests/test_gpu_ivf.py: the smallest that cross every edge of a wave's 64-entry stretch."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.index import ShardIndex
from arxiv_rag_amd.where import pack_bitmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 63, 64, 65, 300, 507)                           # every edge of a wave's 64-entry stretch; 1000 rows
N, NQ, NPROBE, NF = 1000, 70, 3, 5
KS = (1, 10, 32)
INT32_MAX = 2 ** 31 - 1
BAD_Q = (7, 33)                                                 # the two queries whose filter_of is -1 and n_filters


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """(scores, ids[, scanned[, hits]]) device or numpy tuples equal bit for bit."""
    got = [g.cpu().numpy() if torch.is_tensor(g) else g for g in got]
    want = [g.cpu().numpy() if torch.is_tensor(g) else g for g in want]
    return len(got) == len(want) and np.array_equal(bits(got[0]), bits(want[0])) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def words_of(masks):
    return np.stack([pack_bitmap(m).view(np.int64) for m in masks])


_BASE = {}


def base(dim):
    """The base shard of one dim, its hand-built lists, queries, probes, filters and the host answers, computed once and shared."""
    if dim not in _BASE:
        rs = np.random.RandomState(dim)
        X = (rs.randn(N, dim) / np.sqrt(dim)).astype(np.float16)
        labels = rs.permutation(np.concatenate([np.full(m, c) for c, m in enumerate(SIZES)])).astype(np.int32)
        for row, want in ((10, 5), (500, 6)):                   # the two identical rows sit in different lists
            other = int(np.nonzero((labels == want) & ~np.isin(np.arange(N), (10, 500)))[0][0])
            labels[row], labels[other] = labels[other], labels[row]
        assert np.bincount(labels, minlength=7).tolist() == list(SIZES) and labels[10] == 5 and labels[500] == 6
        X[500] = X[10]
        order, start, _ = T.members_host(labels, len(SIZES))
        Q = (rs.randn(NQ, dim) / np.sqrt(dim)).astype(np.float16)
        Q[0] = X[10]
        probes = rs.randint(0, len(SIZES), (NQ, NPROBE)).astype(np.int32)
        probes[0] = (5, 6, 2)
        masks = np.stack([np.ones(N, bool), np.zeros(N, bool), rs.rand(N) < 0.5, rs.rand(N) < 0.01, (np.arange(N) >= 400) & (np.arange(N) < 525)])
        fo = rs.randint(0, NF, NQ).astype(np.int32)
        fo[0] = 0
        fo[list(BAD_Q)] = (-1, NF)
        w = dict(X=X, labels=labels, order=order, start=start, Q=Q, probes=probes, masks=masks, words=words_of(masks), fo=fo, host={},
                 dX=dev(X, np.float16), dorder=dev(order, np.int32), dstart=dev(start, np.int64), dQ=dev(Q, np.float16),
                 dprobes=dev(probes, np.int32), dwords=dev(words_of(masks), np.int64), dfo=dev(fo, np.int32))
        w["index"] = ShardIndex(w["dX"], prefilter=None)
        # every visible row of every query, ranked: the thresholds come from here
        w["full"] = I.search_many_host(X, order, start, probes, Q, N, allows=masks, filter_of=fo)
        _BASE[dim] = w
    return _BASE[dim]


def host(w, k, thr=None, key=None):
    """`search_many_host` under the base filters, cached per (k, key)."""
    if (k, key) not in w["host"]:
        w["host"][(k, key)] = I.search_many_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], k, allows=w["masks"], filter_of=w["fo"],
                                                 min_score=thr)
    return w["host"][(k, key)]


def run(w, k, sel=None, allows="base", fo=None, thr=None, probes=None, **kw):
    """`ivf_search_multi` over the base shard for the queries `sel` (default: all) -> device tensors."""
    sel = np.arange(NQ) if sel is None else np.asarray(sel)
    Q = w["dQ"] if len(sel) == NQ and (sel == np.arange(NQ)).all() else w["dQ"][dev(sel, np.int64)].contiguous()
    allows = w["dwords"] if isinstance(allows, str) else allows
    fo = w["fo"][sel] if fo is None else fo
    return I.ivf_search_multi(w["dX"], w["dorder"], w["dstart"], max(SIZES), Q, dev(w["probes"][sel] if probes is None else probes, np.int32), k,
                              allows=allows, filter_of=None if allows is None else dev(fo, np.int32),
                              min_score=None if thr is None else dev(thr, np.float32), **kw)


def thresholds(w, k):
    """{name: f32 [NQ]}: per query its own 1st, k-th and (k+1)-th best visible score (0 where it has fewer rows), -inf, +inf, NaN, and
    `mixed`, which gives query q the (q mod 6)-th of those."""
    s, n = w["full"][0], w["full"][2]
    at = lambda j: np.where(n > j, s[:, min(j, N - 1)], np.float32(0)).astype(np.float32)
    out = {"first": at(0), "kth": at(k - 1), "next": at(k), "-inf": np.full(NQ, -np.inf, np.float32), "+inf": np.full(NQ, np.inf, np.float32),
           "nan": np.full(NQ, np.nan, np.float32)}
    out["mixed"] = np.stack(list(out.values()))[np.arange(NQ) % 6, np.arange(NQ)]
    return out


# ---- 1: the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_every_answer_equals_the_definition(dim, k):
    w = base(dim)
    got, want = run(w, k), host(w, k)
    assert same(got, want)
    assert got[2].dtype == got[3].dtype == torch.int64 and np.array_equal(want[2], want[3]) and (want[2] > 0).any()
    for q in BAD_Q:                                             # filter_of outside [0, n_filters): nothing
        assert want[2][q] == 0 and (want[1][q] == -1).all()
    nofilter = run(w, k, allows=None)                           # allow == NULL: filter_of is ignored and may be NULL
    assert same(nofilter, I.search_many_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], k))


# ---- 2: one filter, no threshold: arx_ivf_search ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 768])
def test_one_filter_and_no_threshold_is_arx_ivf_search(dim):
    w = base(dim)
    for f in (2, 4):
        one = w["dwords"][f:f + 1].contiguous()
        for k in KS:
            old = I.ivf_search(w["dX"], w["dorder"], w["dstart"], max(SIZES), w["dQ"], w["dprobes"], k, allow=one[0])
            for rpb in (None, 64, 128, 1024):
                s, i, n, h = run(w, k, allows=one, fo=np.zeros(NQ, np.int32), rows_per_block=rpb)
                assert same((s, i, n), old) and torch.equal(h, n)


# ---- 3: the exact search's bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_it_equals_the_filtered_search_over_the_probe_bitmaps(dim, k):
    w = base(dim)
    got = run(w, k)
    maps = I.probe_bitmaps_host(w["order"], w["start"], w["probes"], N)
    ok = (w["fo"] >= 0) & (w["fo"] < NF)
    maps = np.where(ok[:, None], maps & w["words"][np.clip(w["fo"], 0, NF - 1)], 0)
    for a in range(0, NQ, 64):                                  # at most 64 bitmaps per call
        b = min(NQ, a + 64)
        s, i = w["index"].search_filtered_many(w["dQ"][a:b].contiguous(), dev(maps[a:b], np.int64),
                                               torch.arange(b - a, dtype=torch.int32, device=DEV), k, path=2)
        assert same((got[0][a:b], got[1][a:b]), (s, i))


# ---- 4: thresholds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_thresholds(dim, k):
    w = base(dim)
    fs, fi, fn, _ = w["full"]
    maps = I.probe_bitmaps_host(w["order"], w["start"], w["probes"], N)
    for name, thr in thresholds(w, k).items():
        got, want = run(w, k, thr=thr), host(w, k, thr, name)
        assert same(got, want), name
        s, i, n, h = (t.cpu().numpy() for t in got)
        count = ((fi >= 0) & (fs >= thr[:, None])).sum(axis=1)                          # the qualifying rows of the full ranking
        assert np.array_equal(h, count) and np.array_equal(n, fn), name
        assert (s[i >= 0] >= np.broadcast_to(thr[:, None], s.shape)[i >= 0]).all() and ((i >= 0).sum(axis=1) == np.minimum(h, k)).all(), name
        if name == "kth":
            assert (h[fn >= k] >= k).all()                      # the k-th row itself qualifies
        if name == "next":
            assert (h[fn > k] > k).all() and (fn > k).any()     # more hits than the list holds: an exact count above k
        if name == "first":                                     # the two identical rows tie at the top of query 0: a tie at the threshold is kept
            assert h[0] == 2 and i[0, 0] == 10 and (k == 1 or i[0, :3].tolist() == [10, 500, -1])
        if name in ("+inf", "nan"):
            assert (h == 0).all() and (i == -1).all()
        for q in range(NQ):                                     # the range search over the same rows, where it returns every hit
            if h[q] > k or not (0 <= w["fo"][q] < NF) or (dim == 768 and q % 4):      # (dim 768: every fourth query)
                continue
            allow = dev(maps[q] & w["words"][w["fo"][q]], np.int64)
            rs_, ri, rc = w["index"].search_range(w["dQ"][q:q + 1].contiguous(), float(thr[q]), max(int(h[q]), 1), allow=allow)
            m = int(h[q])
            assert int(rc[0]) == m and same((s[q, :m], i[q, :m]), (rs_[0, :m], ri[0, :m])), q


def test_a_nan_score_never_qualifies():
    """Rows holding +inf and -inf score NaN against a query that is non-zero there: under a threshold they are scanned, not hit."""
    w = base(64)
    X = w["X"].copy()
    nan_rows = np.nonzero(w["labels"] == 5)[0][:9]
    X[nan_rows, 0], X[nan_rows, 1] = np.inf, -np.inf
    Q = w["Q"].copy()
    Q[:, :2] = np.float16(0.25)
    probes = np.tile(np.array([[5, 2, 3]], np.int32), (4, 1))
    thr = np.array([-np.inf, -1.0, 0.0, np.nan], np.float32)
    with np.errstate(all="ignore"):
        want = I.search_many_host(X, w["order"], w["start"], probes, Q[:4], 10, min_score=thr)
    got = I.ivf_search_multi(dev(X, np.float16), w["dorder"], w["dstart"], max(SIZES), dev(Q[:4], np.float16), dev(probes, np.int32), 10,
                             min_score=dev(thr, np.float32))
    assert same(got, want)
    assert want[2].tolist() == [427] * 4 and want[3][0] == 427 - 9 and want[3][3] == 0 and not np.isin(want[1], nan_rows).any()


# ---- 5: a query does not depend on its batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 768])
def test_a_query_does_not_depend_on_its_batch(dim):
    w = base(dim)
    thr = thresholds(w, 10)["mixed"]
    want = [t.cpu().numpy() for t in run(w, 10, thr=thr)]
    assert same(want, host(w, 10, thr, "mixed"))
    rev = np.arange(NQ)[::-1].copy()
    assert same(run(w, 10, sel=rev, thr=thr[rev]), [a[rev] for a in want])
    for q in (0, 7, 20, 41, 69):                                # alone
        assert same(run(w, 10, sel=[q], thr=thr[[q]]), [a[[q]] for a in want])
    # among other filters and thresholds: the even queries keep theirs, the odd ones get new ones
    rs = np.random.RandomState(3)
    fo2, thr2 = w["fo"].copy(), thr.copy()
    fo2[1::2], thr2[1::2] = rs.randint(-1, NF + 1, NQ // 2), rs.randn(NQ // 2).astype(np.float32) * 0.1
    got = [t.cpu().numpy() for t in run(w, 10, fo=fo2, thr=thr2, rows_per_block=64)]
    assert same([a[0::2] for a in got], [a[0::2] for a in want])
    assert same(got, I.search_many_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], 10, allows=w["masks"], filter_of=fo2, min_score=thr2))
    many = np.arange(1025) % NQ                                 # crosses the internal batch of 1024 queries
    assert same(run(w, 10, sel=many, thr=thr[many]), [a[many] for a in want])


# ---- 6: bad device data ------------------------------------------------------------------------------------------------------------------
def test_bad_device_data_gives_the_defined_answer():
    """Wrong indices the kernels must ignore, each clamped or tested before it addresses anything: `filter_of` outside [0, n_filters)
    (ivf_scan_kernel tests it before the bitmap's base moves: the block then scores nothing), `start` negative, decreasing and beyond
    n_members (ivf_prepare_kernel clamps into [0, n_members] and takes the prefix maximum), `order` entries outside [0, n_rows) (the row
    test in ivf_scan_kernel before the row addresses the bitmap or the corpus), probes outside [0, n_lists) (length 0 in
    ivf_prepare_kernel)."""
    w = base(64)
    order = w["order"].copy()
    order[[0, 5, 70, 400, 999]] = (-5, N + 3, -5, N + 3, INT32_MAX)
    start = w["start"].copy()
    start[2], start[4], start[7] = -9, 60, 5000                 # negative, decreasing, beyond n_members
    mlr = int(np.diff(T.clamp_starts(start, N)).max())
    probes = w["probes"].copy()
    probes[3], probes[4, 0], probes[5, 2] = (-1, 7, INT32_MAX), -2 ** 31, 7
    fo = w["fo"].copy()
    fo[[1, 2, 3, 9]] = (INT32_MAX, -2 ** 31, 0, 1 << 20)
    thr = thresholds(w, 10)["mixed"]
    for k in (1, 10):
        for t in (None, thr):
            got = I.ivf_search_multi(w["dX"], dev(order, np.int32), dev(start, np.int64), mlr, w["dQ"], dev(probes, np.int32), k, allows=w["dwords"],
                                     filter_of=dev(fo, np.int32), min_score=None if t is None else dev(t, np.float32))
            assert same(got, I.search_many_host(w["X"], order, start, probes, w["Q"], k, allows=w["masks"], filter_of=fo, min_score=t))
    short = I.ivf_search_multi(w["dX"], dev(order, np.int32), dev(start, np.int64), mlr, w["dQ"], dev(probes, np.int32), 10,
                               allows=dev(words_of(w["masks"][:, :N - 100]), np.int64), filter_of=dev(fo, np.int32), n_rows=N - 100)
    assert same(short, I.search_many_host(w["X"][:N - 100], order, start, probes, w["Q"], 10, allows=w["masks"][:, :N - 100], filter_of=fo))


# ---- 7: dim 8192 and a long shard ----------------------------------------------------------------------------------------------------------
def test_dim_8192():
    rs = np.random.RandomState(8192)
    X = (rs.randn(300, 8192) / 90).astype(np.float16)
    labels = rs.randint(0, 3, 300).astype(np.int32)
    order, start, sizes = T.members_host(labels, 3)
    Q = (rs.randn(3, 8192) / 90).astype(np.float16)
    probes = np.array([[0, 2], [1, 1], [2, 0]], np.int32)
    masks = np.stack([rs.rand(300) < 0.5, rs.rand(300) < 0.2])
    fo, thr = np.array([0, 1, 2], np.int32), np.array([0.0, -np.inf, 0.0], np.float32)
    got = I.ivf_search_multi(dev(X, np.float16), dev(order, np.int32), dev(start, np.int64), int(sizes.max()), dev(Q, np.float16),
                             dev(probes, np.int32), 10, allows=dev(words_of(masks), np.int64), filter_of=dev(fo, np.int32), min_score=dev(thr, np.float32))
    want = I.search_many_host(X, order, start, probes, Q, 10, allows=masks, filter_of=fo, min_score=thr)
    assert same(got, want) and want[3][0] > 0 and want[3][2] == 0


def test_a_long_shard_with_more_partial_lists_than_one_merge_round():
    """70 000 rows at dim 64 in 40 lists, one of them holding 40 000 rows; two filters; rows_per_block = 64 puts more than 600 partial
    lists and counts behind one query (a merge round takes 512)."""
    rs = np.random.RandomState(77)
    n = 70000
    X = (rs.randn(n, 64) / 8).astype(np.float16)
    small = rs.multinomial(30000, np.ones(39) / 39)
    labels = rs.permutation(np.concatenate([np.full(40000, 17)] + [np.full(m, c if c < 17 else c + 1) for c, m in enumerate(small)]))
    order, start, sizes = T.members_host(labels.astype(np.int32), 40)
    Q = (rs.randn(6, 64) / 8).astype(np.float16)
    probes = np.stack([rs.permutation(40)[:8] for _ in range(6)]).astype(np.int32)
    probes[:5, 3] = 17
    probes[:5, 0] = np.where(probes[:5, 0] == 17, 16, probes[:5, 0])
    masks = np.stack([np.ones(n, bool), rs.rand(n) < 0.9])
    fo = np.array([0, 1, 0, 1, 2, 1], np.int32)
    thr = np.array([-np.inf, 0.0, 0.2, 0.35, 0.0, np.nan], np.float32)
    args = (dev(X, np.float16), dev(order, np.int32), dev(start, np.int64), int(sizes.max()), dev(Q, np.float16), dev(probes, np.int32))
    dw, dfo = dev(words_of(masks), np.int64), dev(fo, np.int32)
    for t in (None, thr):
        want = I.search_many_host(X, order, start, probes, Q, 10, allows=masks, filter_of=fo, min_score=t)
        assert want[2].max() / 64 > 600 and want[2][4] == 0
        for rpb in (None, 64, 4096):
            got = I.ivf_search_multi(*args, 10, allows=dw, filter_of=dfo, min_score=None if t is None else dev(t, np.float32), rows_per_block=rpb)
            assert same(got, want), rpb
    assert 10 < want[3][2] < want[2][2] and want[3][1] > 1 << 14         # counts far beyond k, exact


# ---- 8: the library's refusals ---------------------------------------------------------------------------------------------------------
def test_the_library_refuses_arguments_outside_its_limits():
    from arxiv_rag_amd import _lib
    w = base(64)
    args = (w["dX"], w["dorder"], w["dstart"], max(SIZES), w["dQ"], w["dprobes"])
    with pytest.raises(_lib.ArxError, match="n_filters=0"):
        I.ivf_search_multi(*args, 10, allows=w["dwords"], filter_of=w["dfo"], _n_filters=0)
    with pytest.raises(_lib.ArxError, match="filter_of"):
        I.ivf_search_multi(*args, 10, allows=w["dwords"], filter_of=None)
    with pytest.raises(_lib.ArxError, match="rows_per_block"):
        I.ivf_search_multi(*args, 10, allows=w["dwords"], filter_of=w["dfo"], rows_per_block=96)
    with pytest.raises(_lib.ArxError, match="unsupported shape.*k=33"):          # the host layer's own refusal (the workspace function says -1)
        I.ivf_search_multi(*args, 33, allows=w["dwords"], filter_of=w["dfo"])
    # a short workspace: the host layer would allocate a larger one, so the library is called directly; the buffer itself is large
    # enough, only the size it is told is arx_ivf_workspace_bytes' (short by the blocks' counts of qualifying rows)
    lib = _lib.load()
    need, old = (f(N, len(SIZES), NQ, NPROBE, 64, 10) for f in (lib.arx_ivf_multi_workspace_bytes, lib.arx_ivf_workspace_bytes))
    assert 0 < old < need
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    s, i = torch.empty((NQ, 10), dtype=torch.float32, device=DEV), torch.empty((NQ, 10), dtype=torch.int64, device=DEV)
    n, h = torch.empty(NQ, dtype=torch.int64, device=DEV), torch.empty(NQ, dtype=torch.int64, device=DEV)
    def direct(k, ws_bytes):
        return lib.arx_ivf_search_multi(w["dX"].data_ptr(), N, 64, w["dorder"].data_ptr(), N, w["dstart"].data_ptr(), len(SIZES), max(SIZES),
                                        w["dQ"].data_ptr(), NQ, w["dprobes"].data_ptr(), NPROBE, w["dwords"].data_ptr(), NF, w["dfo"].data_ptr(),
                                        None, k, s.data_ptr(), i.data_ptr(), n.data_ptr(), h.data_ptr(), 0, ws.data_ptr(), ws_bytes,
                                        torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.ArxError, match="workspace too small.*arx_ivf_multi_workspace_bytes"):
        _lib.check(direct(10, old), "arx_ivf_search_multi")
    with pytest.raises(_lib.ArxError, match=r"k=33 out of range 1\.\.32"):          # the library's own check of k, before anything is written
        _lib.check(direct(33, need), "arx_ivf_search_multi")


# ---- the index ---------------------------------------------------------------------------------------------------------------------------
def test_search_many_on_a_built_index():
    from arxiv_rag_amd.index import fill_clustered_rows
    X = fill_clustered_rows(20000, 256, seed=3, n_clusters=40, device=DEV)
    Q = fill_clustered_rows(16, 256, seed=3, n_clusters=40, device=DEV, row_base=1 << 30)
    ivf = I.IvfIndex.build(ShardIndex(X, prefilter=None), 32, iters=4, seed=1)
    rs = np.random.RandomState(2)
    masks = rs.rand(3, 20000) < 0.3
    fo = rs.randint(0, 3, 16).astype(np.int32)
    dw, dfo = dev(words_of(masks), np.int64), dev(fo, np.int32)
    probes = ivf.probe(Q, 4)
    Xh, order, start = X.cpu().numpy(), ivf.order.cpu().numpy(), ivf.start.cpu().numpy()
    plain = I.search_many_host(Xh, order, start, probes.cpu().numpy(), Q.cpu().numpy(), 10, allows=masks, filter_of=fo)
    thr = plain[0][:, 4].copy()                                 # every query's own 5th-best score
    for ms, want in ((None, plain), (thr, None), (float(thr[0]), None), (dev(thr, np.float32), None)):
        got = ivf.search_many(Q, 10, 4, allows=dw, filter_of=dfo, min_score=ms)
        if want is None:
            want = I.search_many_host(Xh, order, start, probes.cpu().numpy(), Q.cpu().numpy(), 10, allows=masks, filter_of=fo,
                                      min_score=ms.cpu().numpy() if torch.is_tensor(ms) else ms)
        assert same(got, want)
    assert (got[3].cpu().numpy() >= 5).all() and ivf._ws is not None
    ws = ivf._ws
    many = ivf.search_many(Q, 10, 4, allows=dw, filter_of=dfo)
    for f in range(3):                                          # one call per distinct filter gives the same rows
        sel = dev(np.nonzero(fo == f)[0], np.int64)
        if len(sel):
            assert same(ivf.search(Q[sel].contiguous(), 10, 4, allow=dw[f]), [t[sel] for t in many[:3]])
    assert ivf._ws is ws                                        # the cached workspace is reused
    for kw, part in ((dict(allows=dw), "filter_of"), (dict(allows=dw[0], filter_of=dfo), "2-d"), (dict(min_score=[0.1, 0.2]), "min_score has shape")):
        with pytest.raises(ValueError, match=part):
            ivf.search_many(Q, 10, 4, **kw)
    with pytest.raises(ValueError, match="nprobe=33 exceeds"):
        ivf.search_many(Q, 10, 33)


# ---- 9: the retrieval pipeline over a collection -----------------------------------------------------------------------------------------
def _collection_world():
    rs = np.random.RandomState(21)
    centres = rs.randn(12, 128)
    X = centres[rs.randint(0, 12, 3000)] + 0.4 * rs.randn(3000, 128)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    meta = [{"chunk_id": f"c{r}", "text": f"text {r} w{r % 7}", "section": ("Methods", "Results", "Discussion")[r % 3]} for r in range(3000)]
    return X, meta


WHERES = [None, {"section": "Methods"}, {"section": {"$in": ["Methods", "Results"]}}, None, {"section": "Results"}, {"section": "Methods"},
          {"section": "Nowhere"}, {"section": {"$in": ["Methods", "Results"]}}]
DOCS = [None, None, {"$contains": "w3"}, {"$contains": "w3"}, None, None, None, {"$contains": "w3"}]


def _check_retrieve(col, qe, stage):
    """`retrieve(nprobe=, ivf=col.ivf)` with a filter per query and a threshold per query, over the collection's own filters: against
    the host restatement under the bitmaps `RowFilters.per_query` builds (keep-bitmap and-ed in), and query by query against the
    single-`where` route (`IvfIndex.search`) and `col.query(nprobe=)`."""
    from arxiv_rag_amd.retrieval import retrieve
    q16 = dev(qe, np.float16)
    nq, n = len(WHERES), col.index.n_rows

    def go(q=q16, **kw):
        return retrieve(col.index, q, col._row_filters(), kw.pop("n_results", 10), nprobe=3, ivf=col.ivf, **kw)
    bitmaps, filter_of, _ = col._row_filters().per_query(nq, WHERES, DOCS)
    words = np.stack([b.cpu().numpy() for b in bitmaps])
    Xh, order, start = col.index.corpus[:n].cpu().numpy(), col.ivf.order.cpu().numpy(), col.ivf.start.cpu().numpy()
    probes = col.ivf.probe(q16, 3).cpu().numpy()

    def host(k, thr=None):
        return I.search_many_host(Xh, order, start, probes, qe, k, allows=words, filter_of=filter_of, min_score=thr)
    many = go(where=WHERES, where_document=DOCS)
    assert same((many.scores, many.ids, many.ivf_scanned, many.ivf_hits), host(10)), stage
    assert many.truncated is None and (many.ivf_scanned > 0).sum() >= 5 and many.ivf_scanned[6] == 0
    for qi in range(nq):                                        # query by query with a single where: the route that was there before
        one = go(q=q16[qi:qi + 1].contiguous(), where=WHERES[qi], where_document=DOCS[qi])
        assert one.ivf_hits is None and same((one.scores, one.ids, one.ivf_scanned), [a[qi:qi + 1] for a in (many.scores, many.ids, many.ivf_scanned)]), (stage, qi)
        hit = col.query(query_embeddings=qe[qi:qi + 1], n_results=10, nprobe=3, where=WHERES[qi], where_document=DOCS[qi])
        assert hit["indices"][0] == many.ids[qi][many.ids[qi] >= 0].tolist() and hit["ivf_scanned"] == [int(many.ivf_scanned[qi])]
    # min_score: every query's own 5th-best score (ties kept), one float, and both under a single where
    thr = np.where(many.ids[:, 4] >= 0, many.scores[:, 4], np.float32(0.5)).astype(np.float32)
    for ms, kw in ((thr, dict(where=WHERES, where_document=DOCS)), (0.55, dict(where=WHERES, where_document=DOCS))):
        hit, want = go(min_score=ms, **kw), host(10, ms)
        assert same((hit.scores, hit.ids, hit.ivf_scanned, hit.ivf_hits), want), stage
        assert hit.truncated == (want[3] > 10).tolist() and ((hit.ids >= 0).sum(axis=1) == np.minimum(want[3], 10)).all()
    assert (hit.ivf_hits < hit.ivf_scanned).any()
    one_where = go(where=WHERES[2], where_document=DOCS[2], min_score=0.55)
    w2, _ = col._row_filters().allow_of(WHERES[2], DOCS[2])
    assert same((one_where.scores, one_where.ids, one_where.ivf_scanned, one_where.ivf_hits),
                I.search_many_host(Xh, order, start, probes, qe, 10, allows=w2.cpu().numpy()[None], filter_of=np.zeros(nq, np.int64), min_score=0.55))
    # the candidate list of a reranker (width n_candidates) and MMR on it
    cand = go(where=WHERES, where_document=DOCS, n_results=5, n_candidates=32, reranked=True, min_score=thr)
    want = host(32, thr)
    assert same((cand.scores, cand.ids, cand.ivf_scanned, cand.ivf_hits), want) and cand.truncated == (want[3] > 32).tolist()
    for kw in (dict(), dict(min_score=thr)):
        wide = go(where=WHERES, where_document=DOCS, n_results=5, n_candidates=32, reranked=True, **kw)
        mm = go(where=WHERES, where_document=DOCS, n_results=5, n_candidates=32, mmr_lambda=0.5, **kw)
        assert mm.ids.shape == (nq, 5) and np.array_equal(mm.ivf_hits, wide.ivf_hits) and mm.truncated == wide.truncated
        for qi in range(nq):
            got, pool = mm.ids[qi][mm.ids[qi] >= 0], wide.ids[qi][wide.ids[qi] >= 0]
            assert set(got) <= set(pool) and len(set(got)) == len(got) == min(5, len(pool)), (stage, qi)
    return many


def test_retrieve_with_filter_lists_and_thresholds_over_a_collection():
    from arxiv_rag_amd.mutation import unpack_rows
    from arxiv_rag_amd.retrieval import retrieve
    from arxiv_rag_amd.store import HipCollection
    X, meta = _collection_world()
    col = HipCollection(X[:2500], [dict(m) for m in meta[:2500]], capacity=3200, documents=True)
    col.build_ivf(16, iters=4, seed=2)
    qe = X[2600:2608]
    _check_retrieve(col, qe, "built")
    col.add(X[2500:3000], [dict(m) for m in meta[2500:3000]])
    added = _check_retrieve(col, qe, "added")
    assert (added.ids >= 2500).any()
    assert col.delete(where={"section": "Results"}) == 1000
    for stage in ("tombstoned", "compacted"):
        if stage == "compacted":
            col.compact()
        hit = _check_retrieve(col, qe, stage)
        live = np.ones(col.n_total, bool) if col._keep is None else unpack_rows(col._keep.cpu().numpy(), col.n_total)
        rows = hit.ids[hit.ids >= 0]
        assert live[rows].all() and all(col.metadata[r]["section"] != "Results" for r in rows) and hit.ivf_scanned[4] == 0
    q16 = dev(qe, np.float16)
    for kw, text in ((dict(where=WHERES, hybrid_alpha=0.5), "nprobe cannot be combined with hybrid_alpha: the BM25 keyword search has no inverted lists of topics"),
                     (dict(min_score=0.3, grouped=True), "nprobe cannot be combined with group_by: the grouped search reads every row")):
        with pytest.raises(ValueError) as e:
            retrieve(col.index, q16, col._row_filters(), 10, nprobe=3, ivf=col.ivf, **kw)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="k=33"):
        retrieve(col.index, q16, col._row_filters(), 33, nprobe=3, ivf=col.ivf, min_score=0.3)
    with pytest.raises(ValueError, match="nprobe cannot be combined with hybrid_alpha"):
        col.query(query_embeddings=qe, nprobe=3, hybrid_alpha=0.5)
