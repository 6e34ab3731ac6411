"""`arx_cluster_assign` on the device (-m gpu; INTEGRATION.md "Topics"): labels and scores against the numpy restatement
(`topics.assign_exact_host`) AND the exact k = 1 search (`topics.assign(how="search")`), bit for bit, at the shapes that reach every
edge of the kernel; the slow path, the launch shapes, padding, ties, the certificate, bad data, the refusals; `kmeans` on either assign
path; `predict`; `HipCollection.assign_topics` before and after add / delete / compact.  Every comparison is exact."""
import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

from arxiv_rag_amd import _lib
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.store import HipCollection
from tests import topics_fp64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARX_ERR_ARG = -1
U24 = 2.0 ** -24
SECTIONS = ["abstract", "Methods", "Results", "Discussion"]
_CACHE = {}

# (n, C, dim): every n of {1, 63, 64, 65, 257, 4099} and every C of {1, 2, 63, 64, 65, 257, 4096} at dim 64 and at dim 768; dim 8192
# with C = 2 and 65 (a row tile staged in chunks); dim 128; dim 2048 with more centroid tiles than one group holds
GRID = [(1, 1, 64), (63, 2, 64), (64, 63, 64), (65, 64, 64), (257, 65, 64), (4099, 257, 64), (4099, 4096, 64),
        (1, 257, 768), (63, 63, 768), (64, 64, 768), (65, 2, 768), (257, 4096, 768), (4099, 65, 768), (64, 1, 768),
        (65, 257, 128), (65, 2, 8192), (63, 65, 8192), (130, 600, 2048)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def mixed_rows(n, dim, seed):
    """Random fp16 rows with norms between 0.25 and 4."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * rs.uniform(0.25, 4.0, (n, 1))).astype(np.float16)


def measured_bound(c16):
    return float(np.linalg.norm(c16.astype(np.float64), axis=1).max()) * (1.0 + 1e-3)


def case(n, C, dim):
    """Rows, centroids and the host answer of a grid case, computed once."""
    key = (n, C, dim)
    if key not in _CACHE:
        X, Cn = mixed_rows(n, dim, 100 + n + C), mixed_rows(C, dim, 200 + n + C)
        labels, scores = T.assign_exact_host(X, Cn)
        _CACHE[key] = dict(X=X, C=Cn, labels=torch.from_numpy(labels), scores=torch.from_numpy(scores), bound=measured_bound(Cn),
                           xd=torch.from_numpy(X).to(DEV), cd=torch.from_numpy(Cn).to(DEV))
    return _CACHE[key]


def run(xd, cd, bound, tau_mult=None, rows_per_block=0):
    stats = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    labels, scores = T.cluster_assign(xd, cd, bound, tau_mult=tau_mult, rows_per_block=rows_per_block, stats=stats)
    return labels.cpu(), scores.cpu(), stats.cpu().tolist()


def same(got, labels, scores):
    return torch.equal(got[0], labels) and torch.equal(_bits(got[1]), _bits(scores))


@pytest.mark.parametrize("n,C,dim", GRID)
def test_fast_path_equals_the_host_and_the_search(n, C, dim):
    c = case(n, C, dim)
    got = run(c["xd"], c["cd"], c["bound"])
    print(f"n {n} C {C} dim {dim}: stats {got[2]}")
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and same(got, c["labels"], c["scores"])
    assert 0 <= got[2][0] <= n and got[2][1] == got[2][0] * C
    sl, ss = T.assign(c["xd"], c["cd"], c["bound"], how="search")
    assert same((sl.cpu(), ss.cpu()), c["labels"], c["scores"])


@pytest.mark.parametrize("n,C,dim", [(257, 65, 768), (65, 257, 64), (63, 65, 8192), (4099, 257, 64), (65, 2, 768)])
def test_slow_path_gives_the_same_bits(n, C, dim):
    c = case(n, C, dim)
    got = run(c["xd"], c["cd"], c["bound"], tau_mult=1e9)
    assert got[2] == [n, n * C] and same(got, c["labels"], c["scores"])
    assert same(run(c["xd"], c["cd"], c["bound"]), got[0], got[1])


@pytest.mark.parametrize("n,C,dim", [(4099, 257, 64), (257, 4096, 768), (63, 65, 8192), (130, 600, 2048), (65, 257, 128), (1, 1, 64)])
def test_every_launch_shape_gives_the_same_bits(n, C, dim):
    c = case(n, C, dim)
    for rpb in (0, 32, 64):
        for tau_mult in (None, 1.0, 4.0):
            assert same(run(c["xd"], c["cd"], c["bound"], tau_mult=tau_mult, rows_per_block=rpb), c["labels"], c["scores"]), (rpb, tau_mult)


@pytest.mark.parametrize("C", [65, 3])
@pytest.mark.parametrize("dim", [64, 768])
def test_padding_columns_never_win(C, dim):
    """Centroids without a negative component and rows = -centroid_j: every score is at most 0 and nearly all are negative, so a
    padding column counted as 0 would win the row."""
    Cn = np.abs(mixed_rows(C, dim, 31 + C))
    X = (-Cn[np.arange(4 * C + 1) % C]).astype(np.float16)
    labels, scores = T.assign_exact_host(X, Cn)
    assert (T.exact_scores_host(X, Cn) < 0).all()
    for rpb in (32, 64):
        got = run(torch.from_numpy(X).to(DEV), torch.from_numpy(Cn).to(DEV), measured_bound(Cn), rows_per_block=rpb)
        assert same(got, torch.from_numpy(labels), torch.from_numpy(scores)) and int(got[0].max()) < C and int(got[0].min()) >= 0


def test_ties():
    n, dim = 130, 128
    X = mixed_rows(n, dim, 5)
    xd = torch.from_numpy(X).to(DEV)
    # all centroids identical: every row ties, label 0, every row flagged
    Cn = np.repeat(mixed_rows(1, dim, 6), 40, axis=0)
    got = run(xd, torch.from_numpy(Cn).to(DEV), measured_bound(Cn))
    assert got[0].tolist() == [0] * n and got[2] == [n, n * 40]
    assert torch.equal(_bits(got[1]), _bits(torch.from_numpy(T.assign_exact_host(X, Cn)[1])))
    # two centroids one fp16 ulp apart in one dimension, rows on both sides of it (and rows with a zero there: exact ties)
    base = mixed_rows(1, dim, 7)[0]
    up = base.copy()
    up[17] = np.nextafter(up[17], np.float16(np.inf))
    Cn = np.stack([mixed_rows(1, dim, 8)[0] * np.float16(0.01), base, up])
    X2 = np.repeat(base[None, :], 96, axis=0)
    X2[:, 17] = np.repeat(np.array([8.0, -8.0, 0.0], np.float16), 32)
    labels, scores = T.assign_exact_host(X2, Cn)
    assert (labels[:32] == 2).all() and (labels[32:] == 1).all()
    got = run(torch.from_numpy(X2).to(DEV), torch.from_numpy(Cn).to(DEV), measured_bound(Cn))
    assert same(got, torch.from_numpy(labels), torch.from_numpy(scores)) and got[2][0] > 0
    # all-zero rows: label 0, score +0.0
    Cn = mixed_rows(9, dim, 9)
    got = run(torch.zeros((70, dim), dtype=torch.float16, device=DEV), torch.from_numpy(Cn).to(DEV), measured_bound(Cn))
    assert got[0].tolist() == [0] * 70 and _bits(got[1]).tolist() == [0] * 70


@pytest.mark.parametrize("C,dim", [(64, 64), (65, 768), (8, 128)])
def test_the_certificate_is_taken_on_separated_rows(C, dim):
    """x_i = e_c + noise against the centroids e_c.  First, from float64: best minus second is at least 8 tau_i for every row, with
    tau_i = (0.3125 dim + 4) 2^-24 |x_i| max_centroid_norm.  Then no row may be flagged."""
    rs = np.random.RandomState(C + dim)
    n = 1000
    which = rs.randint(0, C, n)
    Cn = np.eye(C, dim).astype(np.float16)
    X = (np.eye(C, dim)[which] + 0.01 * rs.randn(n, dim)).astype(np.float16)
    sc = np.sort(X.astype(np.float64) @ Cn.astype(np.float64).T, axis=1)
    bound = measured_bound(Cn)
    tau = (0.3125 * dim + 4) * U24 * np.linalg.norm(X.astype(np.float64), axis=1) * bound
    assert (sc[:, -1] - sc[:, -2] >= 8 * tau).all()
    got = run(torch.from_numpy(X).to(DEV), torch.from_numpy(Cn).to(DEV), bound)
    assert got[2] == [0, 0] and got[0].tolist() == which.tolist()
    labels, scores = T.assign_exact_host(X, Cn)
    assert same(got, torch.from_numpy(labels), torch.from_numpy(scores))


def test_rows_that_are_not_finite_get_a_label_and_nothing_else_is_touched():
    n, C, dim = 200, 37, 128
    X, Cn = mixed_rows(n, dim, 12), mixed_rows(C, dim, 13)
    bad = [0, 31, 32, 63, 64, 199]
    X[0, 3] = np.nan
    X[31, :] = np.inf
    X[32, 100] = -np.inf
    X[63, 0], X[63, 1] = np.inf, -np.inf
    X[64, :] = np.nan
    X[199, 127] = np.inf
    good = np.setdiff1d(np.arange(n), bad)
    labels, scores = T.assign_exact_host(X[good], Cn)
    lab_buf = torch.full((n + 8,), -12345, dtype=torch.int32, device=DEV)
    sc_buf = torch.full((n + 8,), -777.0, dtype=torch.float32, device=DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    T.cluster_assign(torch.from_numpy(X).to(DEV), torch.from_numpy(Cn).to(DEV), measured_bound(Cn), stats=stats,
                     out=(lab_buf[4:4 + n], sc_buf[4:4 + n]))
    lab, sc = lab_buf.cpu(), sc_buf.cpu()
    assert lab[:4].tolist() == [-12345] * 4 and lab[4 + n:].tolist() == [-12345] * 4
    assert sc[:4].tolist() == [-777.0] * 4 and sc[4 + n:].tolist() == [-777.0] * 4
    assert int(lab[4:4 + n].min()) >= 0 and int(lab[4:4 + n].max()) < C and stats[0].item() >= len(bad)
    assert same((lab[4:4 + n][good], sc[4:4 + n][good]), torch.from_numpy(labels), torch.from_numpy(scores))


def test_refusals_write_nothing():
    lib = _lib.load()
    n, C, dim = 64, 8, 128
    xd = torch.from_numpy(mixed_rows(n + 1, dim, 1)).to(DEV)
    cd = torch.from_numpy(mixed_rows(C + 1, dim, 2)).to(DEV)
    labels = torch.full((n + 4,), -5, dtype=torch.int32, device=DEV)
    scores = torch.full((n + 4,), -5.0, dtype=torch.float32, device=DEV)
    stats = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1024, dtype=torch.int32, device=DEV)
    ok = dict(rows=xd.data_ptr(), n_rows=n, dim=dim, cent=cd.data_ptr(), C=C, norm=1.5, labels=labels.data_ptr(), scores=scores.data_ptr(),
              stats=stats.data_ptr(), ws=ws.data_ptr(), ws_bytes=4096, tau_mult=0.0, rpb=0)

    def call(**kw):
        a = {**ok, **kw}
        rc = lib.arx_cluster_assign_tuned(a["rows"], a["n_rows"], a["dim"], a["cent"], a["C"], a["norm"], a["labels"], a["scores"], a["stats"],
                                          a["ws"], a["ws_bytes"], a["tau_mult"], a["rpb"], None)
        return rc, lib.arx_last_error().decode()

    cases = [(dict(dim=96), "dim"), (dict(dim=32), "dim"), (dict(dim=8256), "dim"), (dict(C=0), "C="), (dict(C=4097), "C="),
             (dict(n_rows=-1), "n_rows"), (dict(n_rows=1 << 31), "n_rows"), (dict(rows=None), "rows"), (dict(rows=xd.data_ptr() + 2), "rows"),
             (dict(cent=None), "centroids_f16"), (dict(cent=cd.data_ptr() + 8), "centroids_f16"), (dict(labels=None), "out_labels"),
             (dict(scores=None), "out_scores"), (dict(labels=labels.data_ptr() + 4), "out_labels"),
             (dict(scores=scores.data_ptr() + 4), "out_scores"), (dict(ws=None), "ws"), (dict(ws=ws.data_ptr() + 4), "ws"),
             (dict(ws_bytes=16 + 4 * n - 1), "ws_bytes"), (dict(norm=-1.0), "max_centroid_norm"), (dict(norm=float("inf")), "max_centroid_norm"),
             (dict(norm=float("nan")), "max_centroid_norm"), (dict(tau_mult=0.5), "tau_mult"), (dict(tau_mult=float("nan")), "tau_mult"),
             (dict(rpb=48), "rows_per_block"), (dict(rpb=-32), "rows_per_block")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == ARX_ERR_ARG and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert labels.cpu().tolist() == [-5] * (n + 4) and scores.cpu().tolist() == [-5.0] * (n + 4) and stats.cpu().tolist() == [-5, -5]
    assert ws.cpu().abs().sum().item() == 0
    rc, msg = call()                                             # the same arguments unchanged are accepted; norm 0 is the default bound
    assert rc == 0, msg
    assert call(norm=0.0)[0] == 0 and call(n_rows=0, rows=None, labels=None, scores=None)[0] == 0
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0, 0] and labels[n:].cpu().tolist() == [-5] * 4


# ---- k-means on either assign path, predict ---------------------------------------------------------------------------------------
def planted():
    if "planted" not in _CACHE:
        X, which, centres = R.planted(4096, 128, 8, 0.2, 7)
        _CACHE["planted"] = dict(X=X, which=which, centres=centres, dev=torch.from_numpy(X).to(DEV))
    return _CACHE["planted"]


def same_fit(a, b):
    assert a["iterations"] == b["iterations"] and a["changed"] == b["changed"] and a["objective"] == b["objective"]
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["sizes"], b["sizes"])
    assert torch.equal(_bits(a["centroids"]), _bits(b["centroids"]))
    assert torch.equal(a["centroids_f16"].view(torch.int16), b["centroids_f16"].view(torch.int16))


def test_kmeans_is_the_same_on_both_assign_paths():
    p = planted()
    same_fit(T.kmeans(p["dev"], 8, iters=20, seed=0), T.kmeans(p["dev"], 8, iters=20, seed=0, assign="search"))
    rows = [int(np.nonzero(p["which"] == c)[0][0]) for c in range(8)]
    init = p["X"][rows].astype(np.float32)
    init[5] = init[2]                                            # two identical init rows: every row ties between them
    a, b = T.kmeans(p["dev"], 8, iters=20, init=init), T.kmeans(p["dev"], 8, iters=20, init=init, assign="search")
    same_fit(a, b)
    one = T.kmeans(p["dev"], 8, iters=1, init=init)
    assert one["sizes"][5].item() == 0 and one["sizes"][2].item() > 0
    with pytest.raises(ValueError, match="assign"):
        T.kmeans(p["dev"], 8, assign="eager")


def test_predict_returns_the_labels_of_the_fit():
    p = planted()
    res = T.kmeans(p["dev"], 8, iters=20, seed=0)
    for cents in (res["centroids"], res["centroids"].cpu().numpy(), res["centroids_f16"]):
        labels, scores = T.predict(p["dev"], cents)
        assert torch.equal(labels, res["labels"]) and labels.dtype == torch.int32 and scores.dtype == torch.float32
    hl, hs = T.assign_exact_host(p["X"], res["centroids_f16"].cpu().numpy())
    assert same((labels.cpu(), scores.cpu()), torch.from_numpy(hl), torch.from_numpy(hs))
    assert res["objective"] == float(scores.to(torch.float64).mean().item())


# ---- HipCollection.assign_topics ------------------------------------------------------------------------------------------------------
def world():
    if "world" not in _CACHE:
        X, _, _ = R.planted(3000, 128, 6, 0.8, 11)
        rs = np.random.RandomState(5)
        meta = [{"chunk_id": f"c{r}", "paper_id": f"p{r // 4}", "section": SECTIONS[int(rs.randint(4))], "quality_score": 0.95,
                 "text": f"chunk {r} speaks of w{int(rs.randint(8))} and of w{int(rs.randint(8))}"} for r in range(3000)]
        _CACHE["world"] = dict(X=X, meta=meta)
    return _CACHE["world"]


def collection(rows=None, **kw):
    w = world()
    rows = np.arange(3000) if rows is None else np.asarray(rows)
    return HipCollection(w["X"][rows], [dict(w["meta"][r]) for r in rows], device=DEV, **kw)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_assign_topics_reproduces_the_fit_and_honours_the_filters():
    w = world()
    col = collection(documents=True)
    res = col.topics(6, iters=6, seed=3)
    got = col.assign_topics(res["centroids"])
    assert got["labels"].dtype == np.int32 and got["scores"].dtype == np.float32 and got["sizes"].dtype == np.int64
    assert np.array_equal(got["labels"], res["labels"]) and np.array_equal(got["sizes"], res["sizes"])
    hl, hs = T.assign_exact_host(w["X"], res["centroids"].astype(np.float16))
    assert np.array_equal(got["labels"], hl) and np.array_equal(np_bits(got["scores"]), np_bits(hs))
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    in_f = np.array([m["section"] in ("Methods", "Results") for m in w["meta"]])
    in_d = np.array(["w3" in m["text"] for m in w["meta"]])
    for allowed, kw in ((in_f, dict(where=f)), (in_d, dict(where_document=fd)), (in_f & in_d, dict(where=f, where_document=fd))):
        sub = col.assign_topics(res["centroids"], **kw)
        alone = collection(np.nonzero(allowed)[0]).assign_topics(res["centroids"])
        assert 0 < allowed.sum() < 3000 and (sub["labels"][~allowed] == -1).all() and np.isnan(sub["scores"][~allowed]).all()
        assert np.array_equal(sub["labels"][allowed], alone["labels"]) and np.array_equal(np_bits(sub["scores"][allowed]), np_bits(alone["scores"]))
        assert np.array_equal(sub["sizes"], alone["sizes"]) and np.array_equal(sub["labels"][allowed], got["labels"][allowed])
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.assign_topics(res["centroids"])
    col.world = 1
    with pytest.raises(ValueError, match="shape"):
        col.assign_topics(res["centroids"][:, :64])
    with pytest.raises(ValueError, match="store_as"):
        col.assign_topics(res["centroids"], store_as=3)


def test_assign_topics_after_add_delete_and_compact():
    w = world()
    col = collection(np.arange(2000), capacity=3000)
    res = col.topics(6, iters=6, seed=3, store_as="topic")
    new = np.arange(2000, 2300)
    col.add(w["X"][new], [dict(w["meta"][r]) for r in new])
    got = col.assign_topics(res["centroids"], store_as="topic")
    assert got["labels"].shape == (2300,) and np.array_equal(got["labels"][:2000], res["labels"])
    hl, hs = T.assign_exact_host(w["X"][new], res["centroids"].astype(np.float16))
    assert np.array_equal(got["labels"][2000:], hl) and np.array_equal(np_bits(got["scores"][2000:]), np_bits(hs))
    assert np.array_equal(got["sizes"], np.bincount(got["labels"], minlength=6))
    # store_as feeds facets and query(where=...)
    assert all(m["topic"] == lab for m, lab in zip(col.metadata, got["labels"].tolist()))
    facet = col.facets({"key": "topic", "kind": "number"}, top=None)[0]
    counts = dict(zip((int(v) for v in facet["values"]), facet["counts"]))
    assert [counts.get(t, 0) for t in range(6)] == got["sizes"].tolist() and facet["missing"] == 0
    for t in range(6):
        hit = col.query(query_embeddings=w["X"][2000:2004], n_results=10, where={"topic": t})
        assert all(got["labels"][r] == t for rows in hit["indices"] for r in rows) and (got["sizes"][t] == 0 or hit["indices"][0])
    # tombstones are -1, then gone
    gone = np.array([m["section"] == "Discussion" for m in col.metadata])
    assert col.delete(where={"section": "Discussion"}) == int(gone.sum()) > 0
    pending = col.assign_topics(res["centroids"])
    assert (pending["labels"][gone] == -1).all() and np.isnan(pending["scores"][gone]).all()
    assert np.array_equal(pending["labels"][~gone], got["labels"][~gone])
    assert np.array_equal(pending["sizes"], np.bincount(got["labels"][~gone], minlength=6))
    col.compact()
    after = col.assign_topics(res["centroids"])
    assert np.array_equal(after["labels"], got["labels"][~gone]) and np.array_equal(np_bits(after["scores"]), np_bits(got["scores"][~gone]))
