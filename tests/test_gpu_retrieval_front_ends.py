"""`HipCollection.query` and `search_queries` are two front ends of one retrieval pipeline (`arxiv_rag_amd/retrieval.py`): over the same
fp16 rows, the same queries and the same filters they must return the same rows in the same order with bit-identical cosine scores, and
their extra fields must agree, in every mode both offer.  One corpus of 300 rows x 128 (the rows a tiny in-process encoder wrote into a
`ShardSink`, with ten near-duplicates copied in), 4 queries."""
import dataclasses
import math

import numpy as np
import pytest

from arxiv_rag_amd import config as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, NQ, K = 300, 4, 10
SECTIONS = ("abstract", "Introduction", "Methods", "Results")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.hub import load_sentence_encoder
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import synthetic_vocab
    root = tmp_path_factory.mktemp("front_ends")
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    save_hf_dir(root / "emb", cfg, seeded_state_dict(cfg, seed=1, std=0.05))
    (root / "emb" / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n", encoding="utf-8")
    model = load_sentence_encoder(str(root / "emb"))
    assert model.get_sentence_embedding_dimension() == 128
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:120]
    rs = np.random.RandomState(11)
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(N)]
    chunks = [{"chunk_id": f"c{j}", "text": t, "metadata": {"paper_id": f"p{j // 7:03d}", "section": SECTIONS[int(rs.randint(4))],
                                                            "quality_score": float(rs.rand()), "year": int(1950 + rs.randint(75))}}
              for j, t in enumerate(texts)]
    sink = GEN.ShardSink(model, 0, N)
    model.encode(texts, batch_size=64, normalize_embeddings=True, device_f16_out=sink.rows)
    sink.rows[200:210] = sink.rows[20:30]                      # near-duplicates: a collection built with dedup_threshold drops rows 200..209
    torch.cuda.synchronize()
    emb = sink.rows.cpu().numpy()
    meta = [{"chunk_id": c["chunk_id"], "text": c["text"], **c["metadata"]} for c in chunks]
    kw = dict(device="cuda:0", keyword=True, tokenizer=model.tokenizer, documents=True, group_key="paper_id", hybrid_filters=True)
    qs = [" ".join(rs.choice(words, size=5)) for _ in range(NQ)]
    qd = torch.empty((NQ, 128), dtype=torch.float16, device="cuda")
    model.encode(qs, batch_size=256, normalize_embeddings=True, device_f16_out=qd, low_latency=True)      # as search_queries encodes them
    out = dict(GEN=GEN, model=model, chunks=chunks, sink=sink, qs=qs, Q=qd.cpu().numpy(), words=words, root=root, emb=emb,
               col=HipCollection(emb, meta, **kw), dev=HipCollection(emb, meta, where_on_device=True, **kw),
               dedup=HipCollection(emb, meta, dedup_threshold=0.999, **kw))
    yield out
    model.encoder.close()


def _same_float(a, b):
    """A collection writes nan where the CLI's hits hold null."""
    return (b is None and math.isnan(a)) or a == b


def _compare(name, got, hits, fields=()):
    """`got`: the collection's dict; `hits`: search_queries' list.  Rows, order and score bits; then the named extra fields."""
    assert len(hits) == NQ
    for q in range(NQ):
        res = hits[q]["results"]
        assert got["indices"][q] == [h["index"] for h in res], (name, q)
        assert got["ids"][q] == [h["chunk_id"] for h in res], (name, q)
        assert len(got["scores"][q]) == len(res) and all(_same_float(a, h["score"]) for a, h in zip(got["scores"][q], res)), (name, q)
        for theirs, ours in fields:
            assert all(_same_float(a, h[ours]) for a, h in zip(got[theirs][q], res)), (name, q, ours)
    return [len(h["results"]) for h in hits]


def test_both_front_ends_return_the_same_rows_and_score_bits_in_every_mode(world):
    w = world
    GEN, qs, Q = w["GEN"], w["qs"], w["Q"]
    one = {"$and": [{"section": {"$in": ["abstract", "Methods"]}}, {"year": {"$gte": 1965}}]}
    doc = {"$contains": w["words"][3]}
    per_query = [{"year": {"$gte": 1990}}, None, {"section": "Results"}, {"year": {"$gte": 1990}}]      # a repeated filter and a None entry
    hybrid = (("hybrid_scores", "hybrid_score"), ("keyword_scores", "keyword_score"))

    def both(name, col="col", fields=(), search=None, **kw):
        got = w[col].query(query_embeddings=Q, query_texts=qs, n_results=K, **kw)
        hits = GEN.search_queries(w["model"], w["chunks"], w["sink"], qs, top_k=K, output_dir=str(w["root"]), **(kw if search is None else search))
        return got, hits, _compare(name, got, hits, fields)

    _, _, n = both("plain")
    assert n == [K] * NQ
    got, _, n = both("where", where=one)
    assert n == [K] * NQ and all(w["chunks"][r]["metadata"]["section"] in ("abstract", "Methods") for rows in got["indices"] for r in rows)
    on_dev, _, _ = both("where + where_on_device", col="dev", where=one, search=dict(where=one, where_on_device=True))
    assert on_dev["indices"] == got["indices"] and on_dev["scores"] == got["scores"]
    got, _, n = both("where_document", where_document=doc)
    assert all(n) and all(doc["$contains"] in w["chunks"][r]["text"] for rows in got["indices"] for r in rows)
    keep = w["dedup"]._keep_mask
    assert keep.sum() == N - 10 and not keep[200:210].any()
    got, _, _ = both("keep-mask", col="dedup", search=dict(keep_mask=keep))
    assert not any(200 <= r < 210 for rows in got["indices"] for r in rows)
    got, _, _ = both("per-query where", where=per_query)
    assert got["indices"][0] != got["indices"][3] or got["scores"][0] != got["scores"][3]            # (same filter, different queries)
    assert all(w["chunks"][r]["metadata"]["section"] == "Results" for r in got["indices"][2])
    got, hits, _ = both("mmr_lambda", fields=(("mmr_scores", "mmr_score"),), mmr_lambda=0.5)
    assert all("mmr_score" in h for r in hits for h in r["results"])
    # grouped: the papers, their order and the chunks of each
    got, hits, _ = both("group_by", group_by=True, chunks_per_group=2, search=dict(group_by_paper=True, chunks_per_paper=2))
    for q in range(NQ):
        res = hits[q]["results"]
        papers = [h["paper_id"] for h in res]
        assert got["group_keys"][q] == list(dict.fromkeys(papers)) and len(got["group_keys"][q]) == K, q
        assert got["group_sizes"][q] == [papers.count(p) for p in got["group_keys"][q]], q
        assert [h["paper_rank"] for h in res] == [1 + got["group_keys"][q].index(p) for p in papers], q
    # a threshold between the queries' 11th best scores: some lists are cut at K, some end before
    table = np.sort(Q.astype(np.float32) @ w["emb"].astype(np.float32).T, axis=1)[:, ::-1]
    thr = float(np.median(table[:, K]))
    got, hits, n = both("min_score", min_score=thr)
    assert got["truncated"] == [h["truncated"] for h in hits]
    assert True in got["truncated"] and False in got["truncated"] and min(n) < K
    both("hybrid_alpha", fields=hybrid, hybrid_alpha=0.7)
    got, _, _ = both("hybrid_alpha + hybrid_filters + where", fields=hybrid, hybrid_alpha=0.7, where=one,
                     search=dict(hybrid_alpha=0.7, where=one, hybrid_filters=True))
    assert all(w["chunks"][r]["metadata"]["section"] in ("abstract", "Methods") for rows in got["indices"] for r in rows)
    both("hybrid_alpha + hybrid_filters + per-query where", fields=hybrid, hybrid_alpha=0.7, where=per_query,
         search=dict(hybrid_alpha=0.7, where=per_query, hybrid_filters=True))
