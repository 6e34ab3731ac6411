"""`graph.GraphIndex.build`, `HipCollection.build_graph` / `query(graph_ef=...)` and the graph's life under delete / add / compact on
the device (-m gpu; INTEGRATION.md "Graph search").  Every comparison is exact; recall is not asserted anywhere (it depends on the data)."""
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import graph as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, DIM = 4096, 128                                               # (fill_clustered_rows makes rows of a multiple of 128 dims)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_state = {}


def shard():
    """4096 clustered rows, their ShardIndex and the exact graph of seed 0, built once."""
    if not _state:
        from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows
        X = fill_clustered_rows(N, DIM, 11, 16, device=DEV)
        idx = ShardIndex(X)
        _state.update(X=X, idx=idx, g=G.GraphIndex.build(idx, degree=32, iters=3))
    return _state["X"], _state["idx"], _state["g"]


def _meta(n, words=None):
    text = (lambda r: f"text {r} w{r % 7}") if words is None else (lambda r: " ".join(words[(r * 5 + j) % len(words)] for j in range(6)) + f" w{r % 7}")
    return [{"chunk_id": f"c{r}", "text": text(r), "section": ("Methods", "Results", "Discussion")[r % 3]} for r in range(n)]


def _same_hits(hit, want_s, want_i, want_n):
    assert hit["graph_scored"] == [int(v) for v in want_n]
    for qi in range(len(hit["indices"])):
        keep = want_i[qi] >= 0
        assert hit["indices"][qi] == want_i[qi][keep].tolist(), qi
        assert np.array_equal(bits(hit["scores"][qi]), bits(want_s[qi][keep])), qi


def test_build_is_deterministic_and_equals_the_restatement():
    from arxiv_rag_amd.ivf import IvfIndex
    X, idx, g = shard()
    again = G.GraphIndex.build(idx, degree=32, iters=3)
    assert torch.equal(again.neighbors, g.neighbors) and torch.equal(again.medoid, g.medoid)
    info = g.summary()
    assert info["rows"] == N and info["degree"] == 32 and info["entry_lists"] == 64 and info["approximate"] is False
    assert info["edges"] == int((g.neighbors >= 0).sum()) > N * 16 and info["seconds"] > 0
    knn = G.knn_lists(idx)
    assert knn.shape == (N, 31) and not bool((knn == torch.arange(N, device=DEV)[:, None]).any())
    knn_h = knn.cpu().numpy()
    for degree in (8, 16, 32):
        assert np.array_equal(G.assemble_device(knn, degree).cpu().numpy(), G.assemble_host(knn_h, degree)), degree
    assert torch.equal(G.assemble_device(knn, 32), g.neighbors)
    short = knn_h[:40, :9].copy()                                 # a shard smaller than the lists are wide: -1 padded, rows past it dropped
    short[short >= 40] = -1
    assert np.array_equal(G.assemble_device(torch.from_numpy(short).to(DEV), 16).cpu().numpy(), G.assemble_host(short, 16))
    ivf = IvfIndex.build(idx, 16, iters=3)
    via = G.GraphIndex.build(idx, degree=32, ivf=ivf, nprobe=16)  # every list probed: the exact lists
    assert torch.equal(via.neighbors, g.neighbors) and via.n_entry_lists == 16 and via.summary()["approximate"] is True
    assert torch.equal(via.centroids_f16, ivf.centroids_f16)
    for bad in (dict(degree=40), dict(degree=12), dict(n_entry_lists=0), dict(nprobe=4), dict(ivf=ivf)):
        with pytest.raises(ValueError):
            G.GraphIndex.build(idx, **bad)


def test_index_search_equals_the_restatement_from_its_own_entries():
    X, idx, g = shard()
    q = X[100:108].contiguous()
    ent = g.entries(q, 8)
    assert ent.shape == (8, 8) and ent.dtype == torch.int32
    s, i, scored, expanded = g.search(q, 10, 64, counters=True)
    want = G.search_host(X.cpu().numpy(), g.neighbors.cpu().numpy(), q.cpu().numpy(), ent.cpu().numpy(), 10, 64, 64)
    assert np.array_equal(i.cpu().numpy(), want[1]) and np.array_equal(bits(s.cpu().numpy()), bits(want[0]))
    assert np.array_equal(scored.cpu().numpy(), want[2]) and np.array_equal(expanded.cpu().numpy(), want[3])
    for bad, part in ((dict(k=33, ef=64), "k=33"), (dict(k=10, ef=9), "ef=9"), (dict(k=10, ef=64, max_iters=300), "visited table"),
                      (dict(k=10, ef=64, n_entries=0), "n_entries")):
        with pytest.raises(ValueError, match=part):
            g.search(q, **bad)
    assert g.search(q, 10, 512)[1].shape == (8, 10)               # max_iters defaults to what the visited table admits (255 here)


def test_collection_queries_through_the_graph():
    from arxiv_rag_amd.retrieval import retrieve
    from arxiv_rag_amd.store import HipCollection
    X, _, _ = shard()
    Xh = X.cpu().numpy()
    col = HipCollection(Xh[:2000], _meta(2000), capacity=2200, documents=True)
    qe = Xh[3000:3008]
    q16 = torch.from_numpy(qe).to(DEV)
    with pytest.raises(ValueError, match="build_graph"):
        col.query(query_embeddings=qe, graph_ef=64)
    info = col.build_graph(degree=16, iters=3)
    assert info["rows"] == 2000 and info["degree"] == 16 and info["entry_lists"] == 45
    col.build_pq(dsub=8, iters=2)
    col.build_binary()
    col.build_ivf(4)
    for kw, part in ((dict(where=[None] * 8), "per-query"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(nprobe=2), "nprobe"), (dict(binary_candidates=40), "binary_candidates"),
                     (dict(pq_candidates=40), "pq_candidates"), (dict(boost_weight=0.5), "boost_weight"), (dict(graph_ef=513), "graph_ef=513"),
                     (dict(graph_ef=5), "below k=10"), (dict(n_results=5, n_candidates=32, mmr_lambda=0.5, graph_ef=20), "below k=32"),
                     (dict(graph_entries=33), "graph_entries"), (dict(n_results=40), "width")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=qe, **{"graph_ef": 64, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.query(query_embeddings=qe, graph_ef=64)
    with pytest.raises(ValueError, match="world == 1"):
        col.build_graph()
    col.world = 1
    with pytest.raises(ValueError, match="degree=40"):
        col.build_graph(degree=40)
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    for where, where_document in ((None, None), (f, None), (f, fd)):
        hit = col.query(query_embeddings=qe, n_results=10, graph_ef=64, where=where, where_document=where_document)
        allow, _ = col._row_filters().allow_of(where, where_document)
        s, i, n = col.graph.search(q16, 10, 64, allow=allow)
        _same_hits(hit, s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())
        got = retrieve(col.index, q16, col._row_filters(), 10, where=where, where_document=where_document, graph_ef=64, graph=col.graph)
        _same_hits(hit, got.scores, got.ids, got.graph_scored)
        if where is not None:
            assert all(m["section"] != "Discussion" for ms in hit["metadatas"] for m in ms)
    # delete: the keep-bitmap hides the row, the walk still crosses it and finds what lay behind it
    before = col.query(query_embeddings=qe, n_results=10, graph_ef=64)
    top = [rows[0] for rows in before["indices"]]
    assert col.delete(ids=[f"c{r}" for r in sorted(set(top))]) == len(set(top))
    after = col.query(query_embeddings=qe, n_results=10, graph_ef=64)
    for qi in range(8):
        assert not set(top) & set(after["indices"][qi])
        assert [r for r in before["indices"][qi] if r not in top] == after["indices"][qi][:len([r for r in before["indices"][qi] if r not in top])]
    assert after["graph_scored"] == before["graph_scored"]       # the same walk
    # add and compact make the graph stale
    col.add(Xh[2000:2100], _meta(2100)[2000:])
    with pytest.raises(ValueError, match="stale"):
        col.query(query_embeddings=qe, graph_ef=64)
    assert col.query(query_embeddings=qe, n_results=10)["indices"]                          # the other searches go on
    col.build_graph(degree=16, iters=3)
    assert col.graph.n_rows == 2100 and not col.graph.stale and "graph_scored" in col.query(query_embeddings=qe, n_results=10, graph_ef=64)
    col.compact()
    with pytest.raises(ValueError, match="stale"):
        col.query(query_embeddings=qe, graph_ef=64)


def test_mmr_and_the_golden_reranker_consume_the_list():
    from arxiv_rag_amd.mmr import mmr_select
    from arxiv_rag_amd.rerank import rerank_candidates, reorder_by_rerank
    from arxiv_rag_amd.store import HipCollection
    from tests.test_gpu_range_search import _golden_reranker
    model, words = _golden_reranker()
    X, _, _ = shard()
    Xh = X.cpu().numpy()
    meta = _meta(1000, words)
    col = HipCollection(Xh[:1000], [dict(m) for m in meta], capacity=1100)
    col.build_graph(degree=16, iters=2)
    qe = Xh[3000:3004]
    q16 = torch.from_numpy(qe).to(DEV)
    texts = [" ".join(words[j * 3:j * 3 + 4]) for j in range(4)]
    cs, ci, cn = (t.cpu().numpy() for t in col.graph.search(q16, 32, 64))
    cand = col.query(query_embeddings=qe, n_results=32, graph_ef=64)
    _same_hits(cand, cs, ci, cn)
    rr = col.query(query_embeddings=qe, query_texts=texts, n_results=5, n_candidates=32, graph_ef=64, reranker=model)
    sc = rerank_candidates(lambda pairs: model.predict(pairs, batch_size=32, convert_to_numpy=True), texts, ci,
                           {int(j): meta[int(j)]["text"] for j in np.unique(ci) if j >= 0})
    picked = reorder_by_rerank(ci, sc, 5)
    mm = col.query(query_embeddings=qe, n_results=5, n_candidates=32, graph_ef=64, mmr_lambda=0.5)
    order = mmr_select(col.index, q16, torch.from_numpy(ci).to(DEV), 5, 0.5)[0].cpu().numpy()
    for qi in range(4):
        assert rr["indices"][qi] == [int(j) for _, j, _ in picked[qi]] and rr["graph_scored"][qi] == cn[qi]
        assert np.array_equal(bits(rr["scores"][qi]), bits([cs[qi, p] for p, _, _ in picked[qi]]))
        assert np.allclose(rr["rerank_scores"][qi], [v for _, _, v in picked[qi]], rtol=0, atol=1e-6)
        assert mm["indices"][qi] == ci[qi][order[qi]].tolist() and mm["graph_scored"][qi] == cn[qi] and len(mm["mmr_scores"][qi]) == 5


def test_cli_graph_flags_write_the_hits_of_search_queries(tmp_path, monkeypatch):
    """--graph-ef adds `graph_scored` to every entry of search_results.json, whose hits are those `search_queries(graph_ef=)` returns
    for the same shard; without the flag the file's bytes are what they were."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=30, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text(" ".join(words[:6]) + "\n" + " ".join(words[6:12]) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
              "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    out = tmp_path / "embeddings_saved"
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    plain_bytes = (out / "search_results.json").read_bytes()
    plain = json.loads(plain_bytes)
    seen = {}
    real = GEN.search_queries

    def spy(*a, **kw):
        seen["kw"], seen["out"] = {k: kw[k] for k in ("graph_ef", "graph_degree", "graph_entries") if k in kw}, real(*a, **kw)
        return seen["out"]
    monkeypatch.setattr(GEN, "search_queries", spy)
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--graph-ef", "512", "--graph-degree", "16", "--graph-entries", "4"]) == 0
    got = json.loads((out / "search_results.json").read_text())
    assert seen["kw"] == {"graph_ef": 512, "graph_degree": 16, "graph_entries": 4}
    assert got == json.loads(json.dumps(seen["out"])) and len(got) == len(plain) == 2     # the file holds what search_queries returned
    for g, p in zip(got, plain):
        assert set(g) == set(p) | {"graph_scored"} and g["graph_scored"] >= len(g["results"]) > 0 and "graph_scored" not in p
        assert all(set(a) == set(b) for a, b in zip(g["results"], p["results"]))
        exact = {h["index"]: h["score"] for h in p["results"]}
        assert all(h["score"] == exact[h["index"]] for h in g["results"] if h["index"] in exact)       # the exact search's score bits
        assert g["results"][0]["score"] <= p["results"][0]["score"]
    monkeypatch.setattr(GEN, "search_queries", real)
    assert GEN.main(common + ["--graph-ef", "5"]) == 2           # below the ten rows the search returns: refused
    assert GEN.main(common + ["--graph-ef", "64", "--graph-degree", "12"]) == 2
    assert GEN.main(common + ["--graph-ef", "64", "--pq-candidates", "40"]) == 2
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    assert (out / "search_results.json").read_bytes() == plain_bytes
