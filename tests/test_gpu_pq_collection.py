"""`HipCollection.build_pq` / `query(pq_candidates=...)`, the add / delete / compact lifecycle of the codes and the CLI's
`--pq-candidates` on the device (-m gpu; INTEGRATION.md "Product-quantised search").  Every comparison is exact."""
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import pq as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N0, N1 = 500, 640                                               # rows at first, rows after `add`


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _world(words=None):
    rs = np.random.RandomState(33)
    centres = rs.randn(12, 128)
    X = centres[rs.randint(0, 12, N1)] + 0.4 * rs.randn(N1, 128) + 1.5          # a strong shared component: the centre matters
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    text = (lambda r: f"text {r} w{r % 7}") if words is None else (lambda r: " ".join(words[(r * 5 + j) % len(words)] for j in range(6)) + f" w{r % 7}")
    meta = [{"chunk_id": f"c{r}", "text": text(r), "section": ("Methods", "Results", "Discussion")[r % 3]} for r in range(N1)]
    return X, meta


def _same_hits(hit, want_s, want_i, want_n):
    assert hit["pq_count"] == want_n.tolist()
    for qi in range(len(hit["indices"])):
        keep = want_i[qi] >= 0
        assert hit["indices"][qi] == want_i[qi][keep].tolist(), qi
        assert np.array_equal(bits(hit["scores"][qi]), bits(want_s[qi][keep])), qi


def _host_search(col, X, qe, k, R, words):
    pi = col.pq
    lut = P.lut_host(qe, pi.codebooks.cpu().numpy())
    return P.search_host(X, pi.codes.cpu().numpy(), lut, qe, k, R, allow=None if words is None else words.cpu().numpy())


def test_collection_queries_through_the_codes():
    from arxiv_rag_amd.retrieval import retrieve
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700, documents=True)
    qe = X[600:608]
    q16 = dev(qe, np.float16)
    with pytest.raises(ValueError, match="build_pq"):
        col.query(query_embeddings=qe, pq_candidates=40)
    info = col.build_pq(dsub=8, iters=3)
    assert info == {"rows": N0, "dsub": 8, "bytes_per_row": 16, "code_bytes": N0 * 16, "centre": "mean", "trained": True}
    col.build_binary()
    col.build_ivf(4)
    # every refusal fires before a launch: nothing below reaches the device
    for kw, part in ((dict(where=[None] * 8), "per-query"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(nprobe=2), "nprobe"), (dict(binary_candidates=40), "binary_candidates"),
                     (dict(boost_weight=0.5), "boost_weight"), (dict(pq_candidates=257), "n_candidates=257"),
                     (dict(pq_candidates=5), "below k=10"), (dict(n_results=5, n_candidates=32, mmr_lambda=0.5, pq_candidates=20), "below k=32")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=qe, **{"pq_candidates": 40, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.query(query_embeddings=qe, pq_candidates=40)
    with pytest.raises(ValueError, match="world == 1"):
        col.build_pq()
    col.world = 1
    for bad in (dict(dsub=3), dict(dsub=128), dict(centre="median"), dict(codebooks=np.zeros((16, 255, 8), np.float32)),
                dict(codebooks=np.full((16, 256, 8), np.nan, np.float32))):
        with pytest.raises(ValueError):
            col.build_pq(**bad)
    # no filter, where, where + where_document: the collection's bitmap goes to the code scan
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    for where, where_document in ((None, None), (f, None), (f, fd)):
        hit = col.query(query_embeddings=qe, n_results=10, pq_candidates=40, where=where, where_document=where_document)
        words, _ = col._row_filters().allow_of(where, where_document)
        s, i, n = col.pq.search(q16, 10, 40, allow=words)
        _same_hits(hit, s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())
        _same_hits(hit, *_host_search(col, X[:N0], qe, 10, 40, words))
        got = retrieve(col.index, q16, col._row_filters(), 10, where=where, where_document=where_document, pq_candidates=40, pq=col.pq)
        _same_hits(hit, got.scores, got.ids, got.pq_count)
        if where is not None:
            assert all(m["section"] != "Discussion" for ms in hit["metadatas"] for m in ms)
    # every visible row a candidate: the exact query
    exact, full = col.query(query_embeddings=qe, n_results=10, where=f, where_document=fd), \
        col.query(query_embeddings=qe, n_results=10, where=f, where_document=fd, pq_candidates=256)
    assert full["indices"] == exact["indices"] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(full["scores"], exact["scores"]))
    # given codebooks are kept as they are
    kept = col.pq.codebooks.cpu().numpy()
    again = col.build_pq(dsub=8, codebooks=kept, centre=col.pq.centre.cpu().numpy())
    assert again["trained"] is False and again["centre"] == "given" and np.array_equal(col.pq.codebooks.cpu().numpy(), kept)


def test_mmr_and_the_golden_reranker_consume_the_candidates():
    from arxiv_rag_amd.mmr import mmr_select
    from arxiv_rag_amd.rerank import rerank_candidates, reorder_by_rerank
    from arxiv_rag_amd.store import HipCollection
    from tests.test_gpu_range_search import _golden_reranker
    model, words = _golden_reranker()
    X, meta = _world(words)
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700)
    col.build_pq(dsub=8, iters=2)
    qe = X[600:604]
    texts = [" ".join(words[j * 3:j * 3 + 4]) for j in range(4)]
    cs, ci, cn = _host_search(col, X[:N0], qe, 32, 64, None)    # the restatement's 32 candidates of every query
    cand = col.query(query_embeddings=qe, n_results=32, pq_candidates=64)
    _same_hits(cand, cs, ci, cn)
    rr = col.query(query_embeddings=qe, query_texts=texts, n_results=5, n_candidates=32, pq_candidates=64, reranker=model)
    sc = rerank_candidates(lambda pairs: model.predict(pairs, batch_size=32, convert_to_numpy=True), texts, ci,
                           {int(j): meta[int(j)]["text"] for j in np.unique(ci)})
    picked = reorder_by_rerank(ci, sc, 5)
    mm = col.query(query_embeddings=qe, n_results=5, n_candidates=32, pq_candidates=64, mmr_lambda=0.5)
    order = mmr_select(col.index, dev(qe, np.float16), dev(ci, np.int64), 5, 0.5)[0].cpu().numpy()      # MMR over the restatement's list
    for qi in range(4):
        assert rr["indices"][qi] == [int(j) for _, j, _ in picked[qi]] and rr["pq_count"][qi] == 64
        assert np.array_equal(bits(rr["scores"][qi]), bits([cs[qi, p] for p, _, _ in picked[qi]]))
        assert np.allclose(rr["rerank_scores"][qi], [v for _, _, v in picked[qi]], rtol=0, atol=1e-6)
        assert mm["indices"][qi] == ci[qi][order[qi]].tolist() and mm["pq_count"][qi] == 64 and len(mm["mmr_scores"][qi]) == 5


def test_dedup_keep_bitmap_restricts_the_candidates():
    from arxiv_rag_amd.mutation import unpack_rows
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    X = X[:N0].copy()
    X[100:140] = X[0:40]                                         # forty exact duplicates
    col = HipCollection(X, [dict(m) for m in meta[:N0]], dedup_threshold=0.999)
    col.build_pq(iters=2)
    qe = X[:8]
    hit = col.query(query_embeddings=qe, n_results=10, pq_candidates=40)
    keep = unpack_rows(col._keep.cpu().numpy(), N0)
    assert not keep[100:140].any() and all(keep[r] for rows in hit["indices"] for r in rows)
    s, i, n = col.pq.search(dev(qe, np.float16), 10, 40, allow=col._keep)
    _same_hits(hit, s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())


def test_add_delete_compact_keep_the_codes_of_a_fresh_encode():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700)
    col.build_pq(dsub=8, iters=2)
    centre, cb = col.pq.centre.clone(), col.pq.codebooks.clone()
    qe = X[600:608]
    col.add(X[N0:N1], [dict(m) for m in meta[N0:N1]])
    assert col.pq.codes.shape == (N1, 16) and torch.equal(col.pq.centre, centre) and torch.equal(col.pq.codebooks, cb)
    assert np.array_equal(col.pq.codes.cpu().numpy(), P.encode_host(X, cb.cpu().numpy(), centre.cpu().numpy()))
    assert col.delete(where={"section": "Discussion"}) == (N1 + 0) // 3
    tomb = col.query(query_embeddings=qe, n_results=10, pq_candidates=40)
    assert all(m["section"] != "Discussion" for ms in tomb["metadatas"] for m in ms) and tomb["pq_count"] == [40] * 8
    new_of = col.compact()
    keep = new_of >= 0
    assert np.array_equal(col.pq.codes.cpu().numpy(), P.encode_host(X[keep], cb.cpu().numpy(), centre.cpu().numpy()))
    fresh = HipCollection(X[keep], [dict(m) for m, k in zip(meta, keep.tolist()) if k], capacity=700)
    fresh.build_pq(dsub=8, centre=centre.cpu().numpy(), codebooks=cb.cpu().numpy())
    assert torch.equal(col.pq.codes, fresh.pq.codes) and col.pq.codes.shape[0] == int(keep.sum())
    for kw in (dict(n_results=10, pq_candidates=40), dict(n_results=32, pq_candidates=256),
               dict(n_results=10, pq_candidates=40, where={"section": "Methods"})):
        a, b = col.query(query_embeddings=qe, **kw), fresh.query(query_embeddings=qe, **kw)
        assert a["ids"] == b["ids"] and a["indices"] == b["indices"] and a["pq_count"] == b["pq_count"]
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["scores"], b["scores"]))
    # the tombstoned collection answered what the compacted one answers, row numbers apart
    after = col.query(query_embeddings=qe, n_results=10, pq_candidates=40)
    assert after["ids"] == tomb["ids"] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(after["scores"], tomb["scores"]))


def test_cli_pq_candidates_end_to_end(tmp_path, monkeypatch):
    """--pq-candidates adds `pq_count` to every entry of search_results.json; without the flag the file's bytes are what they were."""
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
    n_rows = len(json.loads((out / "metadata.json").read_text()))
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--pq-candidates", "256", "--pq-dsub", "8", "--pq-centre", "mean"]) == 0
    got = json.loads((out / "search_results.json").read_text())
    assert len(got) == len(plain) == 2
    for g, p in zip(got, plain):
        assert set(g) == set(p) | {"pq_count"} and g["pq_count"] == min(256, n_rows) and "pq_count" not in p
        assert len(g["results"]) == len(p["results"]) and all(set(a) == set(b) for a, b in zip(g["results"], p["results"]))
        if n_rows <= 256:                                        # every row a candidate: the exact search's hits
            assert g["results"] == p["results"]
        else:
            assert g["results"][0]["score"] <= p["results"][0]["score"]
    assert GEN.main(common + ["--pq-candidates", "5"]) == 2      # below the ten rows the search returns: refused
    assert GEN.main(common + ["--pq-candidates", "40", "--pq-dsub", "3"]) == 2
    assert GEN.main(common + ["--pq-candidates", "40", "--binary-candidates", "40"]) == 2
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    assert (out / "search_results.json").read_bytes() == plain_bytes
