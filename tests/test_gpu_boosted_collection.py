"""`HipCollection.set_boost` / `query(boost_weight=...)`, the add / delete / compact lifecycle of the prior and the CLI's `--boost-key` on
the device (-m gpu; INTEGRATION.md "Boosted search").  Every comparison is exact: float bits through a uint32 view, ids equal."""
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import boost as BO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N0, N1 = 500, 640                                               # rows at first, rows after `add`
SPEC = {"key": "quality_score", "missing": 0.0}
DECAY = {"key": "year", "decay": "exp", "origin": 2024, "half_life": 3.0, "missing": 0.0}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class FakeReranker:
    def predict(self, pairs, batch_size=32, convert_to_numpy=True):
        return np.array([float(sum(map(ord, t)) % 13) for _, t in pairs], np.float32)


def _world():
    rs = np.random.RandomState(41)
    centres = rs.randn(12, 128)
    X = centres[rs.randint(0, 12, N1)] + 0.6 * rs.randn(N1, 128)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)
    X[N1 - 1] = X[3]                                             # a copy of row 3 among the rows `add` brings (dedup_threshold hides it)
    meta = [{"chunk_id": f"c{r}", "text": f"text {r} w{r % 7}", "section": ("Methods", "Results", "Discussion")[r % 3],
             "quality_score": float(rs.rand()), "year": int(2010 + rs.randint(0, 16))} for r in range(N1)]
    for r in (5, 77, 300):
        del meta[r]["quality_score"]                             # missing keys take the spec's `missing`
    return X, meta


def _same(hit, want, n_results=None):
    """`hit`: a query's dict; `want`: `boosted_host`'s (scores, base, ids)."""
    ws, wb, wi = want
    for qi in range(len(hit["indices"])):
        keep = wi[qi] >= 0
        assert hit["indices"][qi] == wi[qi][keep].tolist(), qi
        assert np.array_equal(bits(hit["scores"][qi]), bits(ws[qi][keep])), qi
        assert np.array_equal(bits(hit["base_scores"][qi]), bits(wb[qi][keep])), qi
        assert np.array_equal(bits(hit["distances"][qi]), bits(2.0 - 2.0 * ws[qi][keep])), qi


def test_end_to_end_from_a_spec_and_from_an_array_and_with_filters():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], documents=True)
    qe = X[600:608]
    before = col.query(query_embeddings=qe, n_results=10)
    with pytest.raises(ValueError, match="set_boost"):
        col.query(query_embeddings=qe, boost_weight=0.1)
    prior = BO.prior_from_metadata(meta[:N0], SPEC)
    info = col.set_boost(SPEC)
    assert info == {"rows": N0, "max_abs_prior": float(np.abs(prior).max()), "non_finite": 0}
    assert np.array_equal(bits(col._prior().cpu().numpy()), bits(prior)) and prior[5] == 0.0
    weights = np.array([0.0, 0.02, 0.2, 5.0, -0.2, 0.02, 0.2, 0.02], np.float32)
    f, fd = {"section": {"$in": ["Methods", "Results"]}}, {"$contains": "w3"}
    for where, where_document in ((None, None), (f, None), (None, fd), (f, fd)):
        words, _ = col._row_filters().allow_of(where, where_document)
        allow = None if words is None else words.cpu().numpy()
        for w in (0.1, weights):
            hit = col.query(query_embeddings=qe, n_results=10, boost_weight=w, where=where, where_document=where_document)
            _same(hit, BO.boosted_host(X[:N0], qe, prior, w, 10, allow))
    assert col.query(query_embeddings=qe, n_results=10) == before            # without boost_weight nothing changed
    # weight 0: the plain query's rows and scores
    zero = col.query(query_embeddings=qe, n_results=10, boost_weight=0.0)
    assert zero["indices"] == before["indices"] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(zero["base_scores"], before["scores"]))
    # an array (numpy, then a tensor), with a hidden row
    arr = BO.prior_from_metadata(meta[:N0], DECAY)
    arr[before["indices"][0][0]] = np.nan
    for given in (arr, torch.from_numpy(arr), torch.from_numpy(arr).to(DEV)):
        assert col.set_boost(given)["non_finite"] == 1
        hit = col.query(query_embeddings=qe, n_results=10, boost_weight=weights)
        _same(hit, BO.boosted_host(X[:N0], qe, arr, weights, 10))
        assert before["indices"][0][0] not in hit["indices"][0]
    assert col.set_boost(DECAY)["max_abs_prior"] <= 1.0
    _same(col.query(query_embeddings=qe, n_results=10, boost_weight=0.3), BO.boosted_host(X[:N0], qe, BO.prior_from_metadata(meta[:N0], DECAY), 0.3, 10))
    # MMR and a reranker consume the boosted list: its rows, the boosted and the base score of each
    col.set_boost(SPEC)
    want = BO.boosted_host(X[:N0], qe, prior, 0.2, 32)
    for kw in (dict(mmr_lambda=0.5), dict(reranker=FakeReranker(), query_texts=[f"q{j}" for j in range(8)])):
        hit = col.query(query_embeddings=qe, n_results=5, n_candidates=32, boost_weight=0.2, **kw)
        for qi in range(8):
            pos = [want[2][qi].tolist().index(r) for r in hit["indices"][qi]]
            assert len(pos) == 5 and np.array_equal(bits(hit["scores"][qi]), bits(want[0][qi][pos]))
            assert np.array_equal(bits(hit["base_scores"][qi]), bits(want[1][qi][pos]))
    assert col.set_boost(None) is None
    with pytest.raises(ValueError, match="set_boost"):
        col.query(query_embeddings=qe, boost_weight=0.1)
    assert col.query(query_embeddings=qe, n_results=10) == before


def test_every_refusal_is_a_value_error_before_any_launch():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700)
    qe = X[600:608]
    col.set_boost(SPEC)
    for kw, part in ((dict(where=[None] * 8), "per-query"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(nprobe=2), "nprobe"), (dict(binary_candidates=40), "binary_candidates"),
                     (dict(boost_weight=float("nan")), "finite"), (dict(boost_weight=float("inf")), "finite"), (dict(boost_weight=[0.1, 0.2]), "shape"),
                     (dict(boost_weight="x"), "number"), (dict(n_results=33), "k=33")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=qe, **{"boost_weight": 0.1, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="world == 1"):
        col.query(query_embeddings=qe, boost_weight=0.1)
    col.world = 1
    for bad, part in (({"key": "section"}, "not a number"), ({"key": "year", "decay": "exp", "origin": 2024, "half_life": 0}, "half_life"),
                      (np.zeros(N0 - 1, np.float32), "shape"), (np.zeros(N0, np.int64), "floats"), ({"missing": 0.0}, "key")):
        with pytest.raises(ValueError, match=part):
            col.set_boost(bad)
    col.set_boost(np.full(N0, 3e38, np.float32))
    with pytest.raises(ValueError, match="not finite"):
        col.query(query_embeddings=qe, boost_weight=2.0)
    with pytest.raises(ValueError, match="boost="):                             # an array prior: `add` needs the new rows' values
        col.add(X[N0:N0 + 2], [dict(m) for m in meta[N0:N0 + 2]])
    with pytest.raises(ValueError, match="shape"):
        col.add(X[N0:N0 + 2], [dict(m) for m in meta[N0:N0 + 2]], boost=np.zeros(3, np.float32))
    assert col.n_total == N0
    col.set_boost(SPEC)
    with pytest.raises(ValueError, match="spec"):
        col.add(X[N0:N0 + 2], [dict(m) for m in meta[N0:N0 + 2]], boost=np.zeros(2, np.float32))
    col.set_boost(None)
    with pytest.raises(ValueError, match="set_boost"):
        col.add(X[N0:N0 + 2], [dict(m) for m in meta[N0:N0 + 2]], boost=np.zeros(2, np.float32))
    assert col.n_total == N0


def test_dedup_threshold_hides_the_duplicates_from_the_boosted_search():
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    col = HipCollection(X, [dict(m) for m in meta], dedup_threshold=0.999)
    assert col._keep_mask is not None and not col._keep_mask[N1 - 1] and col._keep_mask[3]
    col.set_boost(SPEC)
    prior = BO.prior_from_metadata(meta, SPEC)
    qe = np.concatenate([X[3:4], X[600:607]])
    for where in (None, {"section": "Methods"}):
        words, _ = col._row_filters().allow_of(where, None)
        hit = col.query(query_embeddings=qe, n_results=10, boost_weight=0.05, where=where)
        _same(hit, BO.boosted_host(X, qe, prior, 0.05, 10, words.cpu().numpy()))
        assert all(N1 - 1 not in rows for rows in hit["indices"])
    assert 3 in col.query(query_embeddings=qe, n_results=10, boost_weight=0.05)["indices"][0]


@pytest.mark.parametrize("kind", ["spec", "array"])
def test_add_delete_and_compact_carry_the_prior(kind):
    from arxiv_rag_amd.store import HipCollection
    X, meta = _world()
    X = X.copy(); X[N1 - 1] = X[N1 - 2] * np.float16(-1.0)       # (no duplicate here)
    prior = BO.prior_from_metadata(meta, SPEC) if kind == "spec" else np.random.RandomState(9).randn(N1).astype(np.float32)
    col = HipCollection(X[:N0], [dict(m) for m in meta[:N0]], capacity=700, documents=True)
    col.set_boost(SPEC if kind == "spec" else prior[:N0])
    qe = X[600:608]
    weights = np.array([0.0, 0.02, 0.2, 5.0, -0.2, 0.02, 0.2, 0.02], np.float32)
    _same(col.query(query_embeddings=qe, n_results=10, boost_weight=weights), BO.boosted_host(X[:N0], qe, prior[:N0], weights, 10))
    # add
    col.add(X[N0:N1], [dict(m) for m in meta[N0:N1]], **({} if kind == "spec" else {"boost": prior[N0:N1]}))
    assert np.array_equal(bits(col._prior().cpu().numpy()), bits(prior)) and col._boost_max == float(np.abs(prior).max())
    hit = col.query(query_embeddings=qe, n_results=10, boost_weight=weights)
    _same(hit, BO.boosted_host(X, qe, prior, weights, 10))
    assert any(r >= N0 for rows in hit["indices"] for r in rows)
    # delete: the keep-bitmap hides the rows
    assert col.delete(where={"section": "Discussion"}) == N1 // 3
    keep = np.array([m["section"] != "Discussion" for m in meta])
    tomb = col.query(query_embeddings=qe, n_results=10, boost_weight=weights)
    _same(tomb, BO.boosted_host(X, qe, prior, weights, 10, keep))
    _same(col.query(query_embeddings=qe, n_results=10, boost_weight=weights, where={"section": "Methods"}, where_document={"$contains": "w3"}),
          BO.boosted_host(X, qe, prior, weights, 10, keep & np.array([m["section"] == "Methods" and "w3" in m["text"] for m in meta])))
    # compact: the prior moves with the rows; the answers are those of a collection built fresh from the survivors
    new_of = col.compact()
    assert np.array_equal(new_of >= 0, keep)
    assert np.array_equal(bits(col._prior().cpu().numpy()), bits(prior[keep])) and col._prior().shape[0] == int(keep.sum())
    fresh = HipCollection(X[keep], [dict(m) for m, k in zip(meta, keep.tolist()) if k], capacity=700, documents=True)
    fresh.set_boost(SPEC if kind == "spec" else prior[keep])
    assert col._boost_max == fresh._boost_max
    for kw in (dict(n_results=10), dict(n_results=32), dict(n_results=10, where={"section": "Methods"}), dict(n_results=10, where_document={"$contains": "w3"})):
        a, b = col.query(query_embeddings=qe, boost_weight=weights, **kw), fresh.query(query_embeddings=qe, boost_weight=weights, **kw)
        assert a["ids"] == b["ids"] and a["indices"] == b["indices"]
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["scores"], b["scores"]))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["base_scores"], b["base_scores"]))
    after = col.query(query_embeddings=qe, n_results=10, boost_weight=weights)
    _same(after, BO.boosted_host(X[keep], qe, prior[keep], weights, 10))
    assert after["ids"] == tomb["ids"] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(after["scores"], tomb["scores"]))


def test_cli_boost_key_end_to_end(tmp_path, monkeypatch):
    """--boost-key / --boost-weight rank search_results.json by the boosted score and add `base_score` to every hit; without the flags
    the file's bytes are what they were."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=30, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text(" ".join(words[:6]) + "\n" + " ".join(words[6:12]) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
              "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    out = tmp_path / "embeddings_saved"
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    plain_bytes = (out / "search_results.json").read_bytes()
    plain = json.loads(plain_bytes)
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--boost-key", "quality_score", "--boost-weight", "0"]) == 0
    zero = json.loads((out / "search_results.json").read_text())
    for g, p in zip(zero, plain):                                # weight 0: the plain hits, each with its cosine as base_score too
        assert [{k: v for k, v in h.items() if k != "base_score"} for h in g["results"]] == p["results"]
        assert all(h["base_score"] == h["score"] for h in g["results"])
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--boost-key", "quality_score", "--boost-weight", "0.5"]) == 0
    got = json.loads((out / "search_results.json").read_text())
    quality = {m.get("chunk_id"): m.get("quality_score") for m in json.loads((out / "metadata.json").read_text())}
    assert len(got) == len(plain) == 2
    for g in got:
        assert len(g["results"]) == 10
        sc = [h["score"] for h in g["results"]]
        assert sc == sorted(sc, reverse=True)
        for h in g["results"]:
            qv = quality.get(h["chunk_id"])
            if qv is not None:
                assert np.float32(h["score"]) == np.float32(np.float32(h["base_score"]) + np.float32(0.5) * np.float32(qv)), h
    assert [h["index"] for g in got for h in g["results"]] != [h["index"] for p in plain for h in p["results"]]
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--boost-key", "quality_score", "--boost-weight", "0.5", "--boost-decay-origin", "1.0", "--boost-half-life", "0.25"]) == 0
    assert all("base_score" in h for g in json.loads((out / "search_results.json").read_text()) for h in g["results"])
    assert GEN.main(common + ["--boost-key", "quality_score"]) == 2
    assert GEN.main(common + ["--boost-key", "quality_score", "--boost-weight", "0.5", "--min-score", "0.1"]) == 2
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common) == 0
    assert (out / "search_results.json").read_bytes() == plain_bytes
