"""Topic clustering on the device (-m gpu; INTEGRATION.md "Topics"): `topics.kmeans` on planted clusters against the float64 Lloyd of
tests/topics_fp64.py, ties and empty clusters, and `HipCollection.topics` under every row filter against a collection built from the
allowed rows alone (bit for bit), `store_as`, the representatives, determinism and the refusals."""
import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

from arxiv_rag_amd import topics as T
from arxiv_rag_amd.store import HipCollection
from tests import topics_fp64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4 * 2.0 ** -11
SECTIONS = ["abstract", "Methods", "Results", "Discussion"]
_PLANTED, _WORLD = {}, {}


def planted():
    if not _PLANTED:
        X, which, centres = R.planted(4096, 128, 8, 0.2, 7)
        _PLANTED.update(X=X, which=which, centres=centres, dev=torch.from_numpy(X).to(DEV))
    return _PLANTED


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("how", ["one_row_per_centre", "default_seed_0"])
def test_planted_clusters_against_the_float64_lloyd(how):
    """n = 4096, dim = 128, C = 8: unit fp16 rows, eight orthonormal centres plus noise of relative norm 0.2.  The reference is float64
    Lloyd from the same init with its centroids rounded to fp16 before every assign.  A device centroid may differ from the
    reference's by one fp16 rounding per component, which moves a score by at most 2^-11 |x| |c|; the comparison is therefore valid
    where the reference's best-minus-second score is at least 4 x 2^-11 for every row at every assign, which is asserted first (the
    share of rows below the margin is capped at 0; on the CPU the reference shows 0.87 and 0.86 for these two inits)."""
    p = planted()
    X, n = p["X"], 4096
    if how == "one_row_per_centre":
        init = X[[int(np.nonzero(p["which"] == c)[0][0]) for c in range(8)]].astype(np.float32)
        kw = dict(init=init)
    else:
        init = X[np.sort(np.random.default_rng(0).choice(n, 8, replace=False))].astype(np.float32)
        kw = dict(seed=0)
    ref = R.lloyd(X, init, 20)
    assert len(ref) >= 2 and all(r["margin"] >= MARGIN for r in ref), [r["margin"] for r in ref]
    for t in range(1, len(ref) + 1):                             # the labels of every assign: the loop stopped after t of them
        res = T.kmeans(p["dev"], 8, iters=t, **kw)
        assert res["iterations"] == t and np.array_equal(res["labels"].cpu().numpy(), ref[t - 1]["labels"]), t
        assert np.array_equal(res["sizes"].cpu().numpy(), ref[t - 1]["sizes"]), t
        print(f"{how} assign {t}: objective {res['objective']:.9f} reference {ref[t - 1]['objective']:.9f}")
        assert abs(res["objective"] - ref[t - 1]["objective"]) <= 2e-3, t
        c = res["centroids"].cpu().numpy().astype(np.float64)
        # (|S - S64| <= gamma sum|x| <= gamma m max|x| and |S| is about m here: a few gamma per component after the division)
        assert np.abs(c - ref[t - 1]["centroids"]).max() <= 4 * R.sum_bound(n), t
        assert torch.equal(res["centroids_f16"].view(torch.int16), res["centroids"].half().view(torch.int16))
    full = T.kmeans(p["dev"], 8, iters=20, **kw)                 # stops by itself where the reference stops
    assert full["iterations"] == len(ref) and full["changed"][-1] == 0 and full["changed"][0] == n
    assert np.array_equal(full["labels"].cpu().numpy(), ref[-1]["labels"])
    host = T.kmeans_host(X, 8, iters=20, **kw)                   # the numpy restatement follows the same path
    assert host["changed"] == full["changed"] and np.array_equal(host["labels"], ref[-1]["labels"])
    assert np.array_equal(_bits(host["centroids"]), _bits(full["centroids"].cpu().numpy()))


def test_two_identical_init_rows_leave_the_higher_cluster_empty():
    """Centroids 2 and 5 start as the same vector u, a direction near planted centre 2 (cosine about 0.9).  Every row ties between
    them bit for bit and the lower one takes them all; centroid 5 is empty, keeps u through every update, and never wins a row back,
    because the updated centroid 2 (the members' mean direction) is nearer to every member than u is.  When the shared vector is
    itself a row of X (the second half), the higher centroid is empty in the assign that sees the two identical, keeps its value, and
    then scores 1 against that row and takes it back in the next assign: an empty cluster is not relocated, but it can win rows."""
    p = planted()
    X = p["X"]
    rows = [int(np.nonzero(p["which"] == c)[0][0]) for c in range(8)]
    init = X[rows].astype(np.float32)
    g = np.random.RandomState(3).randn(128)
    u = p["centres"][2] + 0.5 * g / np.linalg.norm(g)
    init[2] = init[5] = (u / np.linalg.norm(u)).astype(np.float32)
    res = T.kmeans(p["dev"], 8, iters=20, init=init)
    sizes = res["sizes"].cpu().numpy()
    assert sizes[5] == 0 and sizes[2] == (p["which"] == 2).sum() and sizes.sum() == 4096 and res["iterations"] >= 2
    assert np.array_equal(_bits(res["centroids"][5].cpu().numpy()), _bits(init[5]))
    assert not (res["labels"] == 5).any().item()
    ref = T.kmeans_host(X, 8, iters=20, init=init)
    assert np.array_equal(res["labels"].cpu().numpy(), ref["labels"]) and res["changed"] == ref["changed"]
    # two identical DATA rows as init: the higher one is empty in the assign that sees them identical and keeps its value
    init = X[rows].astype(np.float32)
    init[5] = init[2]
    one = T.kmeans(p["dev"], 8, iters=1, init=init)
    assert one["sizes"][5].item() == 0 and one["sizes"][2].item() > 0
    assert np.array_equal(_bits(one["centroids"].cpu().numpy()), _bits(init))
    more, host = T.kmeans(p["dev"], 8, iters=20, init=init), T.kmeans_host(X, 8, iters=20, init=init)
    assert np.array_equal(more["labels"].cpu().numpy(), host["labels"]) and more["changed"] == host["changed"]
    assert more["sizes"].cpu().numpy().tolist() == host["sizes"].tolist()


def test_as_many_clusters_as_rows_gives_every_size_one():
    rs = np.random.RandomState(2)
    x = rs.randn(200, 64)
    X = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    res = T.kmeans(torch.from_numpy(X).to(DEV), 200, iters=5)
    assert res["sizes"].cpu().numpy().tolist() == [1] * 200
    assert res["labels"].cpu().numpy().tolist() == list(range(200))


# ---- HipCollection.topics ------------------------------------------------------------------------------------------------------------
def world():
    """3000 unit rows of dim 128 around six centres (noise 0.8: several iterations), rows 100..149 copies of rows 0..49."""
    if not _WORLD:
        X, _, _ = R.planted(3000, 128, 6, 0.8, 11)
        X[100:150] = X[0:50]
        rs = np.random.RandomState(5)
        meta = [{"chunk_id": f"c{r}", "paper_id": f"p{r // 4}", "section": SECTIONS[int(rs.randint(4))], "quality_score": 0.95,
                 "text": f"chunk {r} speaks of w{int(rs.randint(8))} and of w{int(rs.randint(8))}"} for r in range(3000)]
        _WORLD.update(X=X, meta=meta)
    return _WORLD


def collection(rows=None, **kw):
    w = world()
    rows = np.arange(3000) if rows is None else np.asarray(rows)
    return HipCollection(w["X"][rows], [dict(w["meta"][r]) for r in rows], device=DEV, **kw)


def check_against_subset(col, allowed, n_topics=6, **filters):
    """`col.topics(**filters)` against `topics` of a collection built from the allowed rows alone: bit for bit."""
    allowed = np.asarray(allowed, dtype=bool)
    got = col.topics(n_topics, iters=6, seed=3, **filters)
    want = collection(np.nonzero(allowed)[0]).topics(n_topics, iters=6, seed=3)
    assert got["labels"].dtype == np.int32 and got["labels"].shape == allowed.shape
    assert (got["labels"][~allowed] == -1).all() and np.array_equal(got["labels"][allowed], want["labels"])
    assert (want["labels"] >= 0).all() and got["iterations"] == want["iterations"] > 1
    assert np.array_equal(_bits(got["centroids"]), _bits(want["centroids"])) and got["centroids"].dtype == np.float32
    assert got["objective"] == want["objective"] and np.array_equal(got["sizes"], want["sizes"])
    assert np.array_equal(got["sizes"], np.bincount(got["labels"][allowed], minlength=n_topics))
    return got


def test_where_and_where_document_equal_a_collection_of_the_allowed_rows():
    w = world()
    col = collection(documents=True)
    f = {"section": {"$in": ["Methods", "Results"]}}
    allowed = np.array([m["section"] in ("Methods", "Results") for m in w["meta"]])
    assert 1000 < allowed.sum() < 2000
    check_against_subset(col, allowed, where=f)
    with_doc = np.array(["w3" in m["text"] for m in w["meta"]])
    check_against_subset(col, with_doc, where_document={"$contains": "w3"})
    check_against_subset(col, allowed & with_doc, where=f, where_document={"$contains": "w3"})
    check_against_subset(collection(where_on_device=True), allowed, where=f)


def test_the_dedup_keep_bitmap_excludes_the_duplicates():
    col = collection(dedup_threshold=0.9995)
    keep = col._keep_mask
    assert not keep[100:150].any() and keep.sum() >= 2900
    check_against_subset(col, keep)


def test_tombstones_before_and_after_compact_and_after_add():
    w = world()
    col = collection(capacity=3100)
    gone = np.array([m["section"] == "Discussion" for m in w["meta"]])
    assert col.delete(where={"section": "Discussion"}) == int(gone.sum())
    before = check_against_subset(col, ~gone)                    # pending tombstones
    col.compact()
    after = col.topics(6, iters=6, seed=3)                       # compacted: the survivors are the collection
    assert np.array_equal(after["labels"], before["labels"][~gone]) and np.array_equal(_bits(after["centroids"]), _bits(before["centroids"]))
    assert after["objective"] == before["objective"]
    col.add(w["X"][:60], [{**w["meta"][r], "chunk_id": f"new{r}"} for r in range(60)])
    rows = np.concatenate([np.nonzero(~gone)[0], np.arange(60)])
    grown, fresh = col.topics(6, iters=6, seed=3), collection(rows).topics(6, iters=6, seed=3)
    assert np.array_equal(grown["labels"], fresh["labels"]) and np.array_equal(_bits(grown["centroids"]), _bits(fresh["centroids"]))


def test_store_as_feeds_facets_and_where():
    col = collection()
    f = {"section": {"$ne": "abstract"}}
    res = col.topics(5, where=f, iters=4, store_as="topic")
    labels = res["labels"]
    assert all(("topic" in m) == (lab >= 0) and (lab < 0 or m["topic"] == lab) for m, lab in zip(col.metadata, labels.tolist()))
    facet = col.facets({"key": "topic", "kind": "number"}, top=None)[0]
    counts = dict(zip((int(v) for v in facet["values"]), facet["counts"]))
    assert [counts.get(t, 0) for t in range(5)] == res["sizes"].tolist() and facet["missing"] == int((labels < 0).sum())
    q = world()["X"][:4]
    for t in range(5):
        hit = col.query(query_embeddings=q, n_results=10, where={"topic": t})
        assert all(labels[r] == t for rows in hit["indices"] for r in rows) and (res["sizes"][t] == 0 or hit["indices"][0])


def test_representatives_are_the_exact_search_of_the_centroids():
    w = world()
    col = collection()
    f = {"section": "Methods"}
    res = col.topics(4, where=f, iters=5, representatives=5)
    allow, _ = col._row_filters().allow_of(f, None)
    c16 = torch.from_numpy(res["centroids"]).to(DEV).half()
    s, i = col.index.search(c16, 5, allow=allow)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert len(res["representatives"]) == 4
    for t, rep in enumerate(res["representatives"]):
        assert rep["indices"] == i[t].tolist() and np.array_equal(_bits(np.array(rep["scores"], np.float32)), _bits(s[t]))
        assert rep["ids"] == [f"c{r}" for r in i[t]] and rep["documents"] == [w["meta"][r]["text"] for r in i[t]]
        assert rep["labels"] == res["labels"][i[t]].tolist() and all(w["meta"][r]["section"] == "Methods" for r in i[t])
    none = col.topics(4, iters=2, representatives=0)
    assert all(rep["ids"] == [] for rep in none["representatives"])


def test_the_cli_step_writes_topics_json(tmp_path):
    import json
    from types import SimpleNamespace
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    w = world()
    chunks = [{"chunk_id": m["chunk_id"], "text": m["text"], "metadata": {"section": m["section"]}} for m in w["meta"]]
    shard = SimpleNamespace(rows=torch.from_numpy(w["X"]).to(DEV), lo=0)
    f = {"section": {"$in": ["Methods", "Results"]}}
    out = GEN.topic_clusters(chunks, shard, 6, iters=6, seed=3, where=f, output_dir=str(tmp_path))
    assert json.loads((tmp_path / "topics.json").read_text()) == out
    want = collection().topics(6, where=f, iters=6, seed=3)
    assert out["sizes"] == want["sizes"].tolist() and out["objective"] == want["objective"] and out["iterations"] == want["iterations"]
    assert out["representatives"] == [rep["ids"] for rep in want["representatives"]] and (out["n_topics"], out["iters"], out["seed"]) == (6, 6, 3)


def test_two_calls_give_identical_bits():
    col = collection()
    a, b = (col.topics(7, where={"section": {"$ne": "Results"}}, iters=8, seed=4) for _ in range(2))
    assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(_bits(a["centroids"]), _bits(b["centroids"]))
    assert a["objective"] == b["objective"] and a["iterations"] == b["iterations"] and np.array_equal(a["sizes"], b["sizes"])
    assert a["representatives"] == b["representatives"]
    x = torch.from_numpy(world()["X"]).to(DEV)
    r1, r2 = (T.kmeans(x, 9, iters=8, seed=1) for _ in range(2))
    assert torch.equal(r1["centroids"].view(torch.int32), r2["centroids"].view(torch.int32)) and r1["changed"] == r2["changed"]
    assert torch.equal(r1["labels"], r2["labels"]) and r1["objective"] == r2["objective"]


def test_refusals():
    col = collection()
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.topics(4)
    col.world = 1
    with pytest.raises(ValueError, match="representatives"):
        col.topics(4, representatives=33)
    n_methods = sum(m["section"] == "Methods" for m in world()["meta"])
    with pytest.raises(ValueError, match="n_clusters"):
        col.topics(n_methods + 1, where={"section": "Methods"})
    with pytest.raises(ValueError, match="n_clusters"):
        col.topics(0)
    with pytest.raises(ValueError, match="iters"):
        col.topics(4, iters=0)
    x = torch.zeros((10, 96), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="dim"):
        T.kmeans(x, 2)
    assert all("topic" not in m for m in col.metadata)           # nothing was stored or kept
