"""`search_queries(nprobe=, ivf_lists=)` with a `where` list and with `min_score` (-m gpu): one IVF call per batch
(`IvfIndex.search_many`), against the same function called query by query with a single `where`, which goes the way it went before
(`IvfIndex.search`).  300 rows x 128 written by a tiny in-process encoder, 4 queries."""
import dataclasses

import numpy as np
import pytest

from arxiv_rag_amd import config as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, NQ, K = 300, 4, 10
SECTIONS = ("abstract", "Introduction", "Methods", "Results")
IVF = dict(nprobe=3, ivf_lists=8, ivf_iters=4, ivf_seed=1)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.hub import load_sentence_encoder
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import synthetic_vocab
    root = tmp_path_factory.mktemp("ivf_multi")
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    save_hf_dir(root / "emb", cfg, seeded_state_dict(cfg, seed=1, std=0.05))
    (root / "emb" / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n", encoding="utf-8")
    model = load_sentence_encoder(str(root / "emb"))
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:120]
    rs = np.random.RandomState(11)
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(N)]
    chunks = [{"chunk_id": f"c{j}", "text": t, "metadata": {"section": SECTIONS[int(rs.randint(4))], "year": int(1950 + rs.randint(75))}}
              for j, t in enumerate(texts)]
    sink = GEN.ShardSink(model, 0, N)
    model.encode(texts, batch_size=64, normalize_embeddings=True, device_f16_out=sink.rows)
    torch.cuda.synchronize()
    qs = [" ".join(rs.choice(words, size=5)) for _ in range(NQ)]
    yield dict(GEN=GEN, model=model, chunks=chunks, sink=sink, qs=qs, root=root)
    model.encoder.close()


def test_search_queries_with_a_where_list_and_a_threshold_through_the_index(world):
    w = world

    def search(qs, **kw):
        return w["GEN"].search_queries(w["model"], w["chunks"], w["sink"], qs, top_k=K, output_dir=str(w["root"]), **IVF, **kw)
    wheres = [{"year": {"$gte": 1990}}, None, {"section": "Results"}, {"year": {"$gte": 1990}}]
    many = search(w["qs"], where=wheres)
    for q in range(NQ):                                         # query by query with a single where: the same hits, score bits and rows scored
        one = search(w["qs"][q:q + 1], where=wheres[q])[0]
        assert "ivf_hits" not in one and one["results"] == many[q]["results"] and one["ivf_scanned"] == many[q]["ivf_scanned"]
        assert many[q]["ivf_hits"] == many[q]["ivf_scanned"] and "truncated" not in many[q] and len(many[q]["results"]) == min(K, many[q]["ivf_scanned"])
    assert all(w["chunks"][h["index"]]["metadata"]["section"] == "Results" for h in many[2]["results"]) and many[2]["results"]
    # a threshold between the 3rd and the 4th score of query 0: its list is cut there, every list holds rows at or above it only
    s0 = [h["score"] for h in many[0]["results"]]
    assert len(s0) >= 4 and s0[2] > s0[3]
    floor = (s0[2] + s0[3]) / 2
    cut = search(w["qs"], where=wheres, min_score=floor)
    assert cut[0]["results"] == many[0]["results"][:3] and cut[0]["ivf_hits"] == 3 and cut[0]["truncated"] is False
    for q in range(NQ):
        want = [h for h in many[q]["results"] if h["score"] >= np.float32(floor)]
        assert cut[q]["ivf_scanned"] == many[q]["ivf_scanned"] and cut[q]["ivf_hits"] <= cut[q]["ivf_scanned"]
        assert cut[q]["truncated"] == (cut[q]["ivf_hits"] > K)
        if not cut[q]["truncated"]:
            assert cut[q]["results"] == want and cut[q]["ivf_hits"] == len(want)
    low = search(w["qs"], min_score=-1.0)                        # every visible row qualifies: the plain IVF answer, with the counts
    plain = search(w["qs"])
    for q in range(NQ):
        assert low[q]["results"] == plain[q]["results"] and low[q]["ivf_hits"] == low[q]["ivf_scanned"] == plain[q]["ivf_scanned"]
        assert low[q]["truncated"] == (low[q]["ivf_scanned"] > K) and "ivf_hits" not in plain[q] and "truncated" not in plain[q]
    with pytest.raises(ValueError, match="nprobe cannot be combined with group_by"):
        search(w["qs"], where=wheres, group_by_paper=True)
