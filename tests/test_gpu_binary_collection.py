"""`HipCollection.build_binary` / `query(binary_candidates=...)`, the add / delete / compact lifecycle of the codes and the CLI's
`--binary-candidates` on the device (-m gpu; INTEGRATION.md "Binary-code search").  Every comparison is exact."""
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import binary as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N0, N1 = 500, 640                                               # rows at first, rows after `add`


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class FakeReranker:
    def predict(self, pairs, batch_size=32, convert_to_numpy=True):
        return np.array([float(sum(map(ord, t)) % 13) for _, t in pairs], np.float32)


def _world():
    rs = np.random.RandomState(33)
    centres = rs.randn(12, 128)
    X = centres[rs.randint(0, 12, N1)] + 0.4 * rs.randn(N1, 128) + 1.5          # a strong shared component: the centre matters
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    meta = [{"chunk_id": f"c{r}", "text": f"text {r} w{r % 7}", "section": ("Methods", "Results", "Discussion")[r % 3]} for r in range(N1)]
    return X, meta


def _same_hits(hit, want_s, want_i, want_n):
    assert hit["binary_count"] == want_n.tolist()
    for qi in range(len(hit["indices"])):
        keep = want_i[qi] >= 0
        assert hit["indices"][qi] == want_i[qi][keep].tolist(), qi
        assert np.array_equal(bits(hit["scores"][qi]), bits(want_s[qi][keep])), qi


def test_collection_queries_through_the_codes():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700, documents=True)
    qe = X[600:608]
    q16 = dev(qe, np.float16)
    with pytest.raises(ValueError, match="build_binary"):
        col.query(query_embeddings=qe, binary_candidates=40)
    info = col.build_binary()
    assert info == {"rows": N0, "words_per_row": 2, "code_bytes": N0 * 16, "centre": "mean"}
    for kw, part in ((dict(where=[None] * 8), "per-query"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(nprobe=2), "nprobe"), (dict(binary_candidates=257), "n_candidates=257"),
                     (dict(binary_candidates=5), "below k=10"), (dict(n_results=5, n_candidates=32, mmr_lambda=0.5, binary_candidates=20), "below k=32")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=qe, **{"binary_candidates": 40, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.query(query_embeddings=qe, binary_candidates=40)
    col.world = 1
    # no filter, where, where + where_document: the collection's bitmap goes to the Hamming scan
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    for where, where_document in ((None, None), (f, None), (f, fd)):
        hit = col.query(query_embeddings=qe, n_results=10, binary_candidates=40, where=where, where_document=where_document)
        words, _ = col._row_filters().allow_of(where, where_document)
        s, i, n = col.binary.search(q16, 10, 40, allow=words)
        _same_hits(hit, s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())
        hs, hi, hn = B.search_host(X[:N0], col.binary.codes.cpu().numpy().view(np.uint64), col.binary.pack(q16).cpu().numpy().view(np.uint64), qe, 10, 40,
                                   allow=None if words is None else words.cpu().numpy())
        _same_hits(hit, hs, hi, hn)
        if where is not None:
            assert all(m["section"] != "Discussion" for ms in hit["metadatas"] for m in ms)
    # every visible row a candidate: the exact query
    exact, full = col.query(query_embeddings=qe, n_results=10, where=f, where_document=fd), \
        col.query(query_embeddings=qe, n_results=10, where=f, where_document=fd, binary_candidates=256)
    assert full["indices"] == exact["indices"] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(full["scores"], exact["scores"]))
    # a reranker and MMR consume the binary candidates
    texts = [f"query {j}" for j in range(8)]
    cand = col.query(query_embeddings=qe, n_results=32, binary_candidates=64)
    rr = col.query(query_embeddings=qe, query_texts=texts, n_results=5, n_candidates=32, binary_candidates=64, reranker=FakeReranker())
    mm = col.query(query_embeddings=qe, n_results=5, n_candidates=32, binary_candidates=64, mmr_lambda=0.5)
    for qi in range(8):
        assert set(rr["indices"][qi]) <= set(cand["indices"][qi]) and len(rr["rerank_scores"][qi]) == len(rr["indices"][qi]) == 5
        assert set(mm["indices"][qi]) <= set(cand["indices"][qi]) and len(set(mm["indices"][qi])) == 5
        assert len(mm["mmr_scores"][qi]) == 5 and rr["binary_count"][qi] == cand["binary_count"][qi] == mm["binary_count"][qi] == 64


def test_dedup_keep_bitmap_restricts_the_candidates():
    from arxiv_rag_amd.mutation import unpack_rows
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    X = X[:N0].copy()
    X[100:140] = X[0:40]                                         # forty exact duplicates
    col = HipCollection(X, [dict(m) for m in meta[:N0]], dedup_threshold=0.999)
    col.build_binary()
    qe = X[:8]
    hit = col.query(query_embeddings=qe, n_results=10, binary_candidates=40)
    keep = unpack_rows(col._keep.cpu().numpy(), N0)
    assert not keep[100:140].any() and all(keep[r] for rows in hit["indices"] for r in rows)
    s, i, n = col.binary.search(dev(qe, np.float16), 10, 40, allow=col._keep)
    _same_hits(hit, s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())


def test_add_delete_compact_keep_the_codes_of_a_fresh_build():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700)
    col.build_binary()
    centre = col.binary.centre.clone()
    qe = X[600:608]
    col.add(X[N0:N1], [dict(m) for m in meta[N0:N1]])
    assert col.binary.codes.shape == (N1, 2) and torch.equal(col.binary.centre, centre)
    assert np.array_equal(col.binary.codes.cpu().numpy().view(np.uint64), B.pack_host(X, centre.cpu().numpy()))
    assert col.delete(where={"section": "Discussion"}) == (N1 + 0) // 3
    tomb = col.query(query_embeddings=qe, n_results=10, binary_candidates=40)
    assert all(m["section"] != "Discussion" for ms in tomb["metadatas"] for m in ms) and tomb["binary_count"] == [40] * 8
    new_of = col.compact()
    keep = new_of >= 0
    fresh = HipCollection(X[keep], [dict(m) for m, k in zip(meta, keep.tolist()) if k], capacity=700)
    fresh.build_binary(centre=centre.cpu().numpy())
    assert torch.equal(col.binary.codes, fresh.binary.codes) and col.binary.codes.shape[0] == int(keep.sum())
    for kw in (dict(n_results=10, binary_candidates=40), dict(n_results=32, binary_candidates=256),
               dict(n_results=10, binary_candidates=40, where={"section": "Methods"})):
        a, b = col.query(query_embeddings=qe, **kw), fresh.query(query_embeddings=qe, **kw)
        assert a["ids"] == b["ids"] and a["indices"] == b["indices"] and a["binary_count"] == b["binary_count"]
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["scores"], b["scores"]))
    # the tombstoned collection answered what the compacted one answers, row numbers apart
    after = col.query(query_embeddings=qe, n_results=10, binary_candidates=40)
    assert after["ids"] == tomb["ids"] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(after["scores"], tomb["scores"]))


def test_cli_binary_candidates_end_to_end(tmp_path, monkeypatch):
    """--binary-candidates adds `binary_count` to every entry of search_results.json; without the flag the file's bytes are what they
    were, run after run."""
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
    assert GEN.main(common + ["--binary-candidates", "256", "--binary-centre", "mean"]) == 0
    got = json.loads((out / "search_results.json").read_text())
    assert len(got) == len(plain) == 2
    for g, p in zip(got, plain):
        assert set(g) == set(p) | {"binary_count"} and g["binary_count"] == min(256, n_rows) and "binary_count" not in p
        assert len(g["results"]) == len(p["results"]) and all(set(a) == set(b) for a, b in zip(g["results"], p["results"]))
        if n_rows <= 256:                                        # every row a candidate: the exact search's hits
            assert g["results"] == p["results"]
        else:
            assert g["results"][0]["score"] <= p["results"][0]["score"]
    assert GEN.main(common + ["--binary-candidates", "5"]) == 2  # below the ten rows the search returns: refused
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    assert (out / "search_results.json").read_bytes() == plain_bytes
