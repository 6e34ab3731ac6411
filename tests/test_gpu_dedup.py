"""Near-duplicate detection on the device (-m gpu): `dedup.find_duplicates` against the float64 definition, `HipCollection(dedup_threshold=...)`
on the tiny golden model with repeated texts, and the CLI's `--dedup-threshold`."""
import json

import numpy as np
import pytest

from tests.helpers import pass_b_budget

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _unit(rs, shape):
    x = rs.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def test_find_duplicates_equals_the_float64_definition(hip):
    """2 000 x 128: 1 700 unit rows, 150 exact copies and 150 near copies (noise of norm 0.05: cosine 0.9988 to the original, 0.9975 to
    another near copy of it), shuffled.  The inputs are built so that no pair lies anywhere near the threshold 0.95 — asserted first, in
    float64 on the fp16 values: every pair is >= 0.99 or <= 0.5, where the fp32 score error at D = 128 is below 1e-6."""
    from arxiv_rag_amd.dedup import duplicates_from_nearest, find_duplicates, nearest_earlier_f64
    from arxiv_rag_amd.index import ShardIndex
    rs = np.random.RandomState(3)
    n_base, n_exact, n_near, d, thr = 1700, 150, 150, 128, 0.95
    base = _unit(rs, (n_base, d))
    src_e, src_n = rs.randint(0, n_base, size=n_exact), rs.randint(0, 40, size=n_near)      # near copies: a few of each of 40 originals
    near = base[src_n] + 0.05 * _unit(rs, (n_near, d))
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    group = np.concatenate([np.arange(n_base), src_e, src_n])                               # the original a row descends from
    rows = np.concatenate([base, base[src_e], near])
    perm = rs.permutation(rows.shape[0])
    rows16, group = rows[perm].astype(np.float16), group[perm]
    x = rows16.astype(np.float64)
    e = x @ x.T
    same = group[:, None] == group[None, :]
    assert e[same].min() >= 0.99 and e[~same].max() <= 0.5, (e[same].min(), e[~same].max())
    s64, i64 = nearest_earlier_f64(rows16)
    want = duplicates_from_nearest(s64, i64, thr)
    first = np.array([np.nonzero(group == g)[0][0] for g in group])
    assert np.array_equal(want >= 0, np.arange(len(group)) != first) and (want >= 0).sum() == n_exact + n_near
    idx = ShardIndex(torch.from_numpy(rows16).cuda())
    dup_of, scores = find_duplicates(idx, thr)
    assert dup_of.dtype == np.int64 and dup_of.shape == (2000,)
    assert np.array_equal(dup_of >= 0, want >= 0), "the set of duplicates differs from the float64 definition"
    # the row each duplicate points at: the float64 nearest earlier row, or one that float64 cannot tell from it within the fp32 budget
    flagged = np.nonzero(want >= 0)[0]
    budget = 2 * pass_b_budget(d) * 1.01 ** 2
    assert (dup_of[flagged] < flagged).all()
    assert (e[flagged, dup_of[flagged]] >= s64[flagged] - budget).all()
    assert np.abs(scores[flagged].astype(np.float64) - e[flagged, dup_of[flagged]]).max() <= budget
    assert scores[0] == -np.inf and np.abs(scores[1:].astype(np.float64) - s64[1:]).max() <= budget
    # bit-identical rows (an original and its exact copies) tie, and the tie goes to the lowest earlier one; a near copy scores 0.9988
    # against them, an identical row its squared norm, 1 to within 1e-3
    exact = np.concatenate([np.ones(n_base + n_exact, bool), np.zeros(n_near, bool)])[perm]
    checked = 0
    for g_ in np.unique(group):
        members = np.nonzero((group == g_) & exact)[0]
        assert all(np.array_equal(rows16[r], rows16[members[0]]) for r in members)
        for r in members[1:]:
            assert dup_of[r] == members[0], (r, members, dup_of[r])
            checked += 1
    assert checked == n_exact


def _tiny_text_model():
    from arxiv_rag_amd import config as CFG
    from arxiv_rag_amd.encoder import HipSentenceEncoder
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from tests.helpers import synthetic_vocab
    from pathlib import Path
    g = np.load(Path(__file__).parent / "golden" / "tiny-mpnet.npz")
    cfg = CFG.TINY_MPNET
    sd = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    vocab = synthetic_vocab(cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1]
    return HipSentenceEncoder(cfg, sd, WordPieceTokenizer.from_vocab(vocab, cfg)), words


def _texts_with_repeats(words, n_distinct=60, seed=5):
    """`n_distinct` random texts, then 25 repeats of some of them (several of text 7) scattered behind their first occurrence."""
    rs = np.random.RandomState(seed)
    texts = [" ".join(rs.choice(words, size=rs.randint(8, 30))) for _ in range(n_distinct)]
    assert len(set(texts)) == n_distinct
    for j, src in enumerate([7, 7, 7, 7] + rs.randint(0, n_distinct, size=21).tolist()):
        texts.insert(rs.randint(n_distinct, len(texts) + 1), texts[src])
    first = [texts.index(t) for t in texts]
    return texts, first


THRESHOLD = 0.99      # repeated texts give bit-identical rows (score = the fp16 row's squared norm, 1 +- 2^-8); distinct texts stay below 0.97


def _assert_separated(emb, first):
    """The property of the INPUTS the tests below rely on, in float64: rows of distinct texts score <= 0.97, of equal texts >= 0.995."""
    x = np.asarray(emb).astype(np.float16).astype(np.float64)
    e = x @ x.T
    same = np.array(first)[:, None] == np.array(first)[None, :]
    assert e[same].min() >= 0.995 and e[~same].max() <= 0.97, (e[same].min(), e[~same].max())


def test_collection_dedup_threshold_on_the_tiny_golden_model(hip):
    from arxiv_rag_amd.store import HipCollection
    model, words = _tiny_text_model()
    texts, first = _texts_with_repeats(words)
    n = len(texts)
    emb = np.asarray(model.encode(texts, normalize_embeddings=True, convert_to_numpy=True), np.float32)
    _assert_separated(emb, first)
    meta = [{"chunk_id": f"c{r}", "text": t, "paper_id": f"p{r % 3}", "section": "abstract" if r % 2 else "body", "quality_score": 1.0}
            for r, t in enumerate(texts)]
    plain = HipCollection(emb, meta)
    coll = HipCollection(emb, meta, dedup_threshold=THRESHOLD)
    repeats = [r for r in range(n) if first[r] != r]
    assert len(repeats) == 25 and plain.duplicates == []
    assert [(e["index"], e["chunk_id"], e["duplicate_of_index"], e["duplicate_of"]) for e in coll.duplicates] == \
        [(r, f"c{r}", first[r], f"c{first[r]}") for r in repeats]
    assert all(abs(e["score"] - 1.0) < 2.0 ** -7 for e in coll.duplicates)
    # queries: the repeated texts' own rows (their copies score highest) and a few others
    q = emb[[7, repeats[0], repeats[5], first[repeats[9]], 11]].astype(np.float16)
    base = plain.query(query_embeddings=q, n_results=10)
    assert any(r in repeats for rows in base["indices"] for r in rows), "the plain answers hold no repeat: the test shows nothing"
    out = coll.query(query_embeddings=q, n_results=10)
    assert all(r not in repeats for rows in out["indices"] for r in rows) and all(len(rows) == 10 for rows in out["indices"])
    # ... and they are the plain search's answers with the repeats struck out (the scores of the kept rows unchanged)
    wide = plain.query(query_embeddings=q, n_results=32)
    for b in range(q.shape[0]):
        kept = [(r, s) for r, s in zip(wide["indices"][b], wide["scores"][b]) if r not in repeats]
        if len(kept) >= 10:
            assert out["indices"][b] == [r for r, _ in kept[:10]] and out["scores"][b] == [s for _, s in kept[:10]], b
    where = {"section": "abstract"}
    outw = coll.query(query_embeddings=q, n_results=10, where=where)
    assert all(r not in repeats and meta[r]["section"] == "abstract" for rows in outw["indices"] for r in rows)
    assert all(len(rows) == 10 for rows in outw["indices"])
    assert any(r in repeats for rows in plain.query(query_embeddings=q, n_results=10, where=where)["indices"] for r in rows)
    outm = coll.query(query_embeddings=q, n_results=5, n_candidates=16, mmr_lambda=0.5)
    assert all(r not in repeats for rows in outm["indices"] for r in rows) and all(len(rows) == 5 for rows in outm["indices"])
    assert "mmr_scores" in outm
    # where_document composes the same way
    docs = HipCollection(emb, meta, documents=True, dedup_threshold=THRESHOLD)
    word = texts[repeats[0]].split()[0]
    outd = docs.query(query_embeddings=q, n_results=10, where_document={"$contains": word})
    assert all(r not in repeats and word in texts[r] for rows in outd["indices"] for r in rows) and outd["indices"][0]
    outdw = docs.query(query_embeddings=q, n_results=10, where_document={"$contains": word}, where=where)
    assert all(r not in repeats and word in texts[r] and meta[r]["section"] == "abstract" for rows in outdw["indices"] for r in rows)
    # without the parameter nothing changes
    assert HipCollection(emb, meta, dedup_threshold=None).query(query_embeddings=q, n_results=10) == base
    # refusals
    with pytest.raises(ValueError, match="hybrid_alpha"):
        coll.query(query_embeddings=q, query_texts=["a"] * 5, hybrid_alpha=0.5)
    for bad in (0.0, 1.5, float("nan"), -1.0):
        with pytest.raises(ValueError, match="dedup_threshold"):
            HipCollection(emb, meta, dedup_threshold=bad)
    with pytest.raises(ValueError, match="world"):
        HipCollection(emb, meta, rank=0, world=2, dedup_threshold=THRESHOLD)
    model.encoder.close()


def _write_chunk_tree(root, texts):
    """Stage-3 output files (the schema of tests.helpers.make_chunk_tree) holding `texts` in order, seven chunks per paper."""
    root.mkdir(parents=True, exist_ok=True)
    for f in range(0, len(texts), 7):
        pid = f"0704.{f // 7:04d}"
        chunks = [{"chunk_id": f"{pid}_chunk_{c}", "text": t,
                   "metadata": {"quality_score": 0.95, "paper_id": pid, "section": "Methods", "chunk_index": c}}
                  for c, t in enumerate(texts[f:f + 7])]
        (root / f"{pid}.json").write_text(json.dumps({"paper_id": pid, "chunks": chunks}))


def test_cli_dedup_threshold_writes_duplicates_json_and_leaves_the_other_files_alone(hip, tmp_path, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    model, words = _tiny_text_model()
    texts, _ = _texts_with_repeats(words, seed=6)
    _write_chunk_tree(tmp_path / "in", texts)
    queries = [texts[7], texts[20], " ".join(words[:6])]
    (tmp_path / "queries.txt").write_text("\n".join(queries) + "\n")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = [str(tmp_path / "in"), "--min-quality", "0.0", "--skip-chroma", "--batch-size", "16", "--queries", str(tmp_path / "queries.txt"),
            "--top-k", "10"]
    outs = {}
    for tag, extra in (("plain", []), ("dedup", ["--dedup-threshold", str(THRESHOLD)])):
        (tmp_path / tag).mkdir()
        monkeypatch.chdir(tmp_path / tag)
        assert GEN.main(base + extra, model_factory=lambda name: model) == 0
        d = tmp_path / tag / "embeddings_saved"
        outs[tag] = {f: (d / f).read_bytes() for f in ("embeddings.npy", "metadata.json", "index.json")}
        outs[tag]["hits"] = json.loads((d / "search_results.json").read_text())
        assert (d / "duplicates.json").exists() == bool(extra)
    for f in ("embeddings.npy", "metadata.json", "index.json"):
        assert outs["plain"][f] == outs["dedup"][f], f
    meta = json.loads(outs["plain"]["metadata.json"])
    emb = np.load(tmp_path / "plain" / "embeddings_saved" / "embeddings.npy")
    got_texts = [m["text"] for m in meta]
    assert sorted(got_texts) == sorted(texts)
    first = [got_texts.index(t) for t in got_texts]
    _assert_separated(emb, first)
    repeats = [r for r in range(len(first)) if first[r] != r]
    dj = json.loads((tmp_path / "dedup" / "embeddings_saved" / "duplicates.json").read_text())
    assert set(dj) == {"threshold", "n_chunks", "n_duplicates", "duplicates"}
    assert dj["threshold"] == THRESHOLD and dj["n_chunks"] == len(texts) and dj["n_duplicates"] == len(repeats) == 25
    assert [(e["index"], e["chunk_id"], e["duplicate_of_index"], e["duplicate_of"]) for e in dj["duplicates"]] == \
        [(r, meta[r]["chunk_id"], first[r], meta[first[r]]["chunk_id"]) for r in repeats]
    assert all(set(e) == {"index", "chunk_id", "duplicate_of_index", "duplicate_of", "score"} and abs(e["score"] - 1.0) < 2.0 ** -7
               for e in dj["duplicates"])
    # the search of the same run skips them; the run without the flag returns some
    assert any(h["index"] in repeats for r in outs["plain"]["hits"] for h in r["results"])
    for plain_r, r in zip(outs["plain"]["hits"], outs["dedup"]["hits"]):
        assert all(h["index"] not in repeats for h in r["results"]) and len(r["results"]) == 10
        kept = [(h["index"], h["score"]) for h in plain_r["results"] if h["index"] not in repeats]
        assert [(h["index"], h["score"]) for h in r["results"]][:len(kept)] == kept
    model.encoder.close()
    GEN._model, GEN._model_name = None, None
