"""arx_ivf_search / arx_ivf_search_tuned (csrc/ivf.hip), `ivf.IvfIndex` and `HipCollection.query(nprobe=...)` on the device (-m gpu).
Every comparison is exact, on ids and on score bits: against the numpy restatement (`ivf.search_host`), against the existing filtered
search over the probe bitmaps, and against the exact search where every list is probed.  The lists of the kernel tests are hand-built
(no k-means involved)."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 63, 64, 65, 300, 507)                           # every edge of a wave's 64-entry stretch; 1000 rows
N, NQ, NPROBE = 1000, 70, 3
KS = (1, 10, 32)
INT32_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """(scores, ids[, scanned]) device or numpy tuples equal bit for bit."""
    got = [g.cpu().numpy() if torch.is_tensor(g) else g for g in got]
    return np.array_equal(bits(got[0]), bits(want[0])) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


_BASE = {}


def base(dim):
    """The base shard of one dim, its hand-built lists, queries, probes and the host answers, computed once and shared."""
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
        w = dict(X=X, labels=labels, order=order, start=start, Q=Q, probes=probes, host={},
                 dX=dev(X, np.float16), dorder=dev(order, np.int32), dstart=dev(start, np.int64), dQ=dev(Q, np.float16))
        w["index"] = ShardIndex(w["dX"], prefilter=None)
        _BASE[dim] = w
    return _BASE[dim]


def host(w, k):
    if k not in w["host"]:
        w["host"][k] = I.search_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], k)
    return w["host"][k]


def run(w, probes, k, Q=None, allow=None, **kw):
    return I.ivf_search(w["dX"], w["dorder"], w["dstart"], max(SIZES), w["dQ"] if Q is None else Q, dev(probes, np.int32), k,
                        allow=None if allow is None else dev(allow, np.int64), **kw)


# ---- hand-built lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_every_answer_equals_the_definition(dim, k):
    w = base(dim)
    got, want = run(w, w["probes"], k), host(w, k)
    assert same(got, want)
    assert (want[2] > 0).any() and got[2].dtype == torch.int64


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_it_equals_the_filtered_search_over_the_probe_bitmaps(dim, k):
    w = base(dim)
    got = run(w, w["probes"], k)
    maps = I.probe_bitmaps_host(w["order"], w["start"], w["probes"], N)
    for a in range(0, NQ, 64):                                  # at most 64 bitmaps per call
        b = min(NQ, a + 64)
        s, i = w["index"].search_filtered_many(w["dQ"][a:b].contiguous(), dev(maps[a:b], np.int64),
                                               torch.arange(b - a, dtype=torch.int32, device=DEV), k, path=2)
        assert same((got[0][a:b], got[1][a:b]), (s.cpu().numpy(), i.cpu().numpy()))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 768])
def test_probing_every_list_is_the_exact_search(dim, k):
    w = base(dim)
    got = run(w, np.tile(np.arange(7, dtype=np.int32), (NQ, 1)), k)
    s, i = w["index"].search(w["dQ"], k)
    assert same(got[:2], (s.cpu().numpy(), i.cpu().numpy())) and (got[2].cpu().numpy() == N).all()


@pytest.mark.parametrize("dim", [64, 768])
def test_ties_go_to_the_lower_row_and_a_probed_list_alone_is_seen(dim):
    w = base(dim)
    q = w["dQ"][:1].contiguous()
    s, i, _ = run(w, [[5, 6]], 10, Q=q)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert i[0, :2].tolist() == [10, 500] and bits(s)[0, 0] == bits(s)[0, 1]
    s1, i1, _ = run(w, [[6, 6]], 10, Q=q)
    assert i1.cpu().numpy()[0, 0] == 500 and 10 not in i1.cpu().numpy()[0] and bits(s1.cpu().numpy())[0, 0] == bits(s)[0, 0]


@pytest.mark.parametrize("dim", [64, 768])
def test_short_lists_invalid_probes_and_repeats(dim):
    w = base(dim)
    q = w["dQ"][:4].contiguous()
    s, i, n = (t.cpu().numpy() for t in run(w, [[1], [0], [1], [0]], 10, Q=q))          # lists of one row and of none
    assert n.tolist() == [1, 0, 1, 0] and (i[:, 1:] == -1).all() and np.isneginf(s[:, 1:]).all()
    assert i[0, 0] == int(w["order"][w["start"][1]]) and i[1, 0] == -1 and np.isneginf(s[1, 0])
    s, i, n = (t.cpu().numpy() for t in run(w, [[-1, 7, INT32_MAX]] * 4, 10, Q=q))
    assert (n == 0).all() and (i == -1).all() and np.isneginf(s).all()
    for k in KS:
        repeated = np.array([[5, 5, 2, 5], [3, 3, 3, 3], [2, 7, 2, -1], [4, 2, 4, 2]])
        rep = run(w, repeated, k, Q=q)
        ded = run(w, [[5, 2], [3, 3], [2, -1], [4, 2]], k, Q=q)
        assert same(rep, [t.cpu().numpy() for t in ded])
        assert same(rep, I.search_host(w["X"], w["order"], w["start"], repeated, w["Q"][:4], k))


@pytest.mark.parametrize("dim", [64, 768])
def test_allow_bitmaps(dim):
    from arxiv_rag_amd.where import pack_bitmap
    w = base(dim)
    mask = np.random.RandomState(5).rand(N) < 0.3
    for m in (mask, np.zeros(N, bool)):
        words = pack_bitmap(m).view(np.int64)
        for k in KS:
            got = run(w, w["probes"], k, allow=words)
            want = I.search_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], k, allow=words)
            assert same(got, want) and same(got, I.search_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], k, allow=m))
        assert m.any() or (got[2].cpu().numpy() == 0).all()


@pytest.mark.parametrize("dim", [64, 768])
def test_a_query_does_not_depend_on_its_batch(dim):
    w = base(dim)
    want = host(w, 10)
    perm = np.random.RandomState(9).permutation(NQ)
    got = run(w, w["probes"][perm], 10, Q=w["dQ"][dev(perm, np.int64)].contiguous())
    assert same(got, [a[perm] for a in want])
    five = np.array([3, 0, 69, 41, 17])
    got = run(w, w["probes"][five], 10, Q=w["dQ"][dev(five, np.int64)].contiguous())
    assert same(got, [a[five] for a in want])
    many = np.arange(1025) % NQ                                 # crosses the internal batch of 1024 queries
    got = run(w, w["probes"][many], 10, Q=w["dQ"][dev(many, np.int64)].contiguous())
    assert same(got, [a[many] for a in want])


_LONG = {}


def long_shard():
    """70 000 rows at dim 64 in 40 lists, one of them holding 40 000 rows."""
    if not _LONG:
        rs = np.random.RandomState(77)
        n = 70000
        X = (rs.randn(n, 64) / 8).astype(np.float16)
        small = rs.multinomial(30000, np.ones(39) / 39)
        labels = rs.permutation(np.concatenate([np.full(40000, 17)] + [np.full(m, c if c < 17 else c + 1) for c, m in enumerate(small)]))
        order, start, sizes = T.members_host(labels.astype(np.int32), 40)
        assert sizes[17] == 40000
        Q = (rs.randn(6, 64) / 8).astype(np.float16)
        probes = np.stack([rs.permutation(40)[:8] for _ in range(6)]).astype(np.int32)
        probes[:5, 3] = 17
        probes[:5, 0] = np.where(probes[:5, 0] == 17, 16, probes[:5, 0])
        _LONG.update(X=X, order=order, start=start, Q=Q, probes=probes, mlr=int(sizes.max()),
                     want=I.search_host(X, order, start, probes, Q, 10))
    return _LONG


def test_launch_shapes_and_long_merges_give_the_same_bits():
    w = long_shard()
    args = (dev(w["X"], np.float16), dev(w["order"], np.int32), dev(w["start"], np.int64), w["mlr"], dev(w["Q"], np.float16),
            dev(w["probes"], np.int32), 10)
    default = I.ivf_search(*args)
    assert same(default, w["want"])
    assert w["want"][2].max() / 64 > 600                       # rows_per_block = 64: more than 600 partial lists behind one query
    for rpb in (64, 256, 4096):
        assert same(I.ivf_search(*args, rows_per_block=rpb), w["want"])
    k32 = I.ivf_search(*args[:6], 32, rows_per_block=64)
    assert same(k32, I.search_host(w["X"], w["order"], w["start"], w["probes"], w["Q"], 32))


def test_dim_8192():
    rs = np.random.RandomState(8192)
    X = (rs.randn(300, 8192) / 90).astype(np.float16)
    labels = rs.randint(0, 3, 300).astype(np.int32)
    order, start, sizes = T.members_host(labels, 3)
    Q = (rs.randn(3, 8192) / 90).astype(np.float16)
    probes = np.array([[0, 2], [1, 1], [2, 0]], np.int32)
    got = I.ivf_search(dev(X, np.float16), dev(order, np.int32), dev(start, np.int64), int(sizes.max()), dev(Q, np.float16),
                       dev(probes, np.int32), 10)
    assert same(got, I.search_host(X, order, start, probes, Q, 10))


def test_bad_device_data_gives_the_defined_answer():
    """Entries of `order` outside [0, n_rows) keep their place and are skipped; `start` is read as `topics.clamp_starts` states.  The
    clamps are in ivf_prepare_kernel (every start value into [0, n_members], prefix maximum) and ivf_scan_kernel (the row test before
    the row addresses anything)."""
    w = base(64)
    order = w["order"].copy()
    order[[0, 5, 70, 400, 999]] = (-5, N + 3, -5, N + 3, INT32_MAX)
    start = w["start"].copy()
    start[2], start[4], start[7] = -9, 60, 5000                 # negative, decreasing, beyond n_members
    mlr = int(np.diff(T.clamp_starts(start, N)).max())
    for k in (1, 10):
        got = I.ivf_search(w["dX"], dev(order, np.int32), dev(start, np.int64), mlr, w["dQ"], dev(w["probes"], np.int32), k)
        assert same(got, I.search_host(w["X"], order, start, w["probes"], w["Q"], k))
    short = I.ivf_search(w["dX"], dev(order, np.int32), dev(start, np.int64), mlr, w["dQ"], dev(w["probes"], np.int32), 10, n_rows=N - 100)
    assert same(short, I.search_host(w["X"][:N - 100], order, start, w["probes"], w["Q"], 10))


def test_the_library_refuses_arguments_outside_its_limits():
    from arxiv_rag_amd import _lib
    w = base(64)
    for kw, field in ((dict(k=33), "k="), (dict(k=0), "k="), (dict(rows_per_block=96), "rows_per_block"), (dict(mlr=-1), "max_list_rows")):
        with pytest.raises(_lib.ArxError, match=field):
            I.ivf_search(w["dX"], w["dorder"], w["dstart"], kw.get("mlr", 507), w["dQ"], dev(w["probes"], np.int32), kw.get("k", 10),
                         rows_per_block=kw.get("rows_per_block"))
    with pytest.raises(_lib.ArxError, match="n_probe"):
        I.ivf_search(w["dX"], w["dorder"], w["dstart"], 507, w["dQ"], torch.zeros((NQ, 129), dtype=torch.int32, device=DEV), 10)
    with pytest.raises(_lib.ArxError, match="n_lists"):
        I.ivf_search(w["dX"], w["dorder"], torch.zeros(4098, dtype=torch.int64, device=DEV), 507, w["dQ"], dev(w["probes"], np.int32), 10)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_a_built_index_probes_and_searches_exactly():
    X = fill_clustered_rows(20000, 256, seed=3, n_clusters=40, device=DEV)
    Q = fill_clustered_rows(16, 256, seed=3, n_clusters=40, device=DEV, row_base=1 << 30)
    index = ShardIndex(X, prefilter=None)
    ivf = I.IvfIndex.build(index, 32, iters=4, seed=1)
    info = ivf.summary()
    assert info["n_lists"] == 32 and info["train_rows"] == 8192 and info["list_rows_max"] == ivf.max_list_rows and info["seconds"] > 0
    assert ivf.labels.dtype == torch.int32 and int(ivf.sizes.sum()) == 20000
    for nprobe in (4, 32):
        cs, ci = ShardIndex(ivf.centroids_f16, prefilter=None).search(Q, nprobe)
        assert np.array_equal(ivf.probe(Q, nprobe).cpu().numpy(), ci.cpu().numpy().astype(np.int32))
    probes = ivf.probe(Q, 4)
    got = ivf.search(Q, 10, 4)
    Xh, order, start = X.cpu().numpy(), ivf.order.cpu().numpy(), ivf.start.cpu().numpy()
    assert same(got, I.search_host(Xh, order, start, probes.cpu().numpy(), Q.cpu().numpy(), 10))
    s, i = index.search(Q, 10)
    full = ivf.search(Q, 10, 32)
    assert same(full[:2], (s.cpu().numpy(), i.cpu().numpy())) and (full[2].cpu().numpy() == 20000).all()
    again = I.IvfIndex.build(index, 32, iters=4, seed=1)
    assert torch.equal(again.order, ivf.order) and torch.equal(again.start, ivf.start)
    with pytest.raises(ValueError, match="nprobe=33 exceeds"):
        ivf.search(Q, 10, 33)


def test_probe_beyond_32_lists_uses_the_range_search():
    rs = np.random.RandomState(4)
    X = dev((rs.randn(4000, 64) / 8), np.float16)
    index = ShardIndex(X, prefilter=None)
    ivf = I.IvfIndex.build(index, 48, iters=2, seed=0)
    Q = X[:9].contiguous()
    p40, p32 = ivf.probe(Q, 40).cpu().numpy(), ivf.probe(Q, 32).cpu().numpy()
    assert p40.shape == (9, 40) and np.array_equal(p40[:, :32], p32) and all(len(set(r)) == 40 for r in p40.tolist())
    s, i = index.search(Q, 10)
    assert same(ivf.search(Q, 10, 48)[:2], (s.cpu().numpy(), i.cpu().numpy()))


class FakeReranker:
    def predict(self, pairs, batch_size=32, convert_to_numpy=True):
        return np.array([float(sum(map(ord, t)) % 13) for _, t in pairs], np.float32)


def _collection_world():
    rs = np.random.RandomState(21)
    centres = rs.randn(12, 128)
    X = centres[rs.randint(0, 12, 3000)] + 0.4 * rs.randn(3000, 128)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    meta = [{"chunk_id": f"c{r}", "text": f"text {r} w{r % 7}", "section": ("Methods", "Results", "Discussion")[r % 3]} for r in range(3000)]
    return X, meta


def test_collection_queries_through_the_index():
    from arxiv_rag_amd.mutation import unpack_rows
    from arxiv_rag_amd.store import HipCollection
    X, meta = _collection_world()
    col = HipCollection(X[:2500], [dict(m) for m in meta[:2500]], capacity=3200, documents=True)
    qe = X[2600:2608]
    with pytest.raises(ValueError, match="build_ivf"):
        col.query(query_embeddings=qe, nprobe=2)
    info = col.build_ivf(16, iters=4, seed=2)
    assert info["n_lists"] == 16 and info["list_rows_max"] >= info["list_rows_median"] >= info["list_rows_min"]
    for kw, part in ((dict(where=[None] * 8), "per-query"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(nprobe=17), "n_lists"), (dict(nprobe=0), "nprobe=0")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=qe, **{"nprobe": 2, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.query(query_embeddings=qe, nprobe=2)
    col.world = 1
    # where + where_document under the collection's bitmap
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    hit = col.query(query_embeddings=qe, n_results=10, nprobe=3, where=f, where_document=fd)
    words, _ = col._row_filters().allow_of(f, fd)
    ivf = col.ivf
    q16 = dev(qe, np.float16)
    want = I.search_host(X[:2500], ivf.order.cpu().numpy(), ivf.start.cpu().numpy(), ivf.probe(q16, 3).cpu().numpy(), qe, 10,
                         allow=words.cpu().numpy())
    assert hit["ivf_scanned"] == want[2].tolist()
    for qi in range(8):
        keep = want[1][qi] >= 0
        assert hit["indices"][qi] == want[1][qi][keep].tolist() and np.array_equal(bits(hit["scores"][qi]), bits(want[0][qi][keep]))
    # add, delete, compact: probing every list is the exact query, bit for bit; fewer lists return live rows of probed lists only
    col.add(X[2500:3000], [dict(m) for m in meta[2500:3000]])
    assert col.ivf.labels.shape[0] == 3000 and torch.equal(col.ivf.labels[:2500], ivf.labels[:2500])
    hl, _ = T.assign_exact_host(X[2500:3000], col.ivf.centroids_f16.cpu().numpy())
    assert np.array_equal(col.ivf.labels[2500:].cpu().numpy(), hl)
    assert col.delete(where={"section": "Discussion"}) == 1000
    for stage in ("tombstoned", "compacted"):
        if stage == "compacted":
            new_of = col.compact()
            assert col.ivf.labels.shape[0] == 2000 and np.array_equal(col.ivf.labels.cpu().numpy(), labels_before[new_of >= 0])
        labels_before = col.ivf.labels.cpu().numpy()
        exact, full = col.query(query_embeddings=qe, n_results=10), col.query(query_embeddings=qe, n_results=10, nprobe=16)
        assert full["indices"] == exact["indices"] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(full["scores"], exact["scores"]))
        assert full["ivf_scanned"] == [2000] * 8
        part = col.query(query_embeddings=qe, n_results=10, nprobe=2)
        probes = col.ivf.probe(q16, 2).cpu().numpy()
        live = np.ones(col.n_total, bool) if col._keep is None else unpack_rows(col._keep.cpu().numpy(), col.n_total)
        for qi in range(8):
            rows = part["indices"][qi]
            assert rows and all(live[r] and labels_before[r] in probes[qi] for r in rows)
            assert all(m["section"] != "Discussion" for m in part["metadatas"][qi] if "section" in m)
    # a reranker and MMR consume the IVF candidates
    texts = [f"query {j}" for j in range(8)]
    cand = col.query(query_embeddings=qe, n_results=32, nprobe=2)
    rr = col.query(query_embeddings=qe, query_texts=texts, n_results=5, n_candidates=32, nprobe=2, reranker=FakeReranker())
    mm = col.query(query_embeddings=qe, n_results=5, n_candidates=32, nprobe=2, mmr_lambda=0.5)
    for qi in range(8):
        assert set(rr["indices"][qi]) <= set(cand["indices"][qi]) and len(rr["rerank_scores"][qi]) == len(rr["indices"][qi]) == 5
        assert set(mm["indices"][qi]) <= set(cand["indices"][qi]) and len(set(mm["indices"][qi])) == 5
        assert len(mm["mmr_scores"][qi]) == 5 and rr["ivf_scanned"][qi] == cand["ivf_scanned"][qi] == mm["ivf_scanned"][qi]
