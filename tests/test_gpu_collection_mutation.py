"""A mutable `HipCollection` (`capacity=...`) against one built fresh from the same rows: M is grown by `add` and shrunk by `delete`,
F is built immutable from the survivors in order.  Before `compact()` M returns F's scores bit for bit and F's rows through the
survivors' index map; after it, F's results with equal indices, the hybrid query's included.  The comparisons are exact: a difference
would mean a score's bits depend on the row's position in the shard."""
import dataclasses

import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

from arxiv_rag_amd import config as C
from tests.helpers import synthetic_vocab

pytestmark = pytest.mark.gpu
SECTIONS = ("abstract", "Introduction", "Methods", "Results")
N, D, NQ = 3000, 128, 8                                         # dim 128: the int8 pre-filter is on


def _world():
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from oracle import search_oracle as SO
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:120]
    rs = np.random.RandomState(7)
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(N)]
    texts[5], texts[1500] = "", ""
    emb = SO.unit_rows_f16(N, D, 1).astype(np.float32)
    meta = [{"chunk_id": f"c{j}", "text": t, "paper_id": f"p{j // 8:04d}", "section": SECTIONS[int(rs.randint(4))],
             "quality_score": float(rs.rand()), "year": int(1950 + rs.randint(75))} for j, t in enumerate(texts)]
    qs = [" ".join(rs.choice(words, size=4)) for _ in range(NQ)]
    Q = SO.unit_rows_f16(NQ, D, 2).astype(np.float32)
    return dict(tok=tok, words=words, texts=texts, emb=emb, meta=meta, qs=qs, Q=Q, rs=rs)


def _queries(w):
    words = w["words"]
    per_query = [{"year": {"$gte": 1960 + 5 * j}} if j % 3 else None for j in range(NQ)]
    return {
        "plain": dict(n_results=10),
        "where": dict(n_results=10, where={"year": {"$gte": 1980}}),
        "where_document": dict(n_results=10, where_document={"$contains": words[7]}),
        "regex": dict(n_results=10, where_document={"$regex": words[9][:2] + "[a-z]+ " + words[11][:1]}),
        "both": dict(n_results=10, where={"section": {"$in": ["Methods", "Results"]}}, where_document={"$not_contains": words[3]}),
        "per_query": dict(n_results=10, where=per_query),
        "min_score": dict(n_results=50, min_score=0.15),
        "mmr": dict(n_results=8, n_candidates=24, mmr_lambda=0.5),
        "group_by": dict(n_results=6, group_by=True, chunks_per_group=3),
    }


def _same(got, want, what, index_map=None):
    """`got` is `want`, every float's every bit (repr: nan == nan); `index_map`: want's rows are named through it."""
    assert got.keys() == want.keys(), what
    for key in want:
        if key == "indices" and index_map is not None:
            assert got[key] == [[int(index_map[i]) for i in row] for row in want[key]], (what, key)
        else:
            assert repr(got[key]) == repr(want[key]), (what, key)


@pytest.mark.parametrize("build_on_device", [False, True])
def test_grown_and_shrunk_collection_answers_as_one_built_fresh(build_on_device):
    from arxiv_rag_amd.store import HipCollection
    w = _world()
    emb, meta, words, rs = w["emb"], w["meta"], w["words"], w["rs"]
    kw = dict(device="cuda:0", keyword=True, tokenizer=w["tok"], documents=True, document_regex=True, group_key="paper_id",
              hybrid_filters=True, keyword_build_on_device=build_on_device)
    a, b = 1003, 2000                                            # row 1003 is inside paper p0125: the first add continues its run
    given = list(meta[:a])
    M = HipCollection(emb[:a], given, capacity=N, **kw)
    given.clear()                                                # the collection owns a copy of the list
    assert len(M.metadata) == a and M.count() == a
    M.add(emb[a:b], meta[a:b])
    M.add(emb[b:], meta[b:])
    assert M.count() == N and M.index.n_rows == N and M.index.max_run_rows == 8

    base = {name: M.query(query_embeddings=w["Q"], **q) for name, q in _queries(w).items()}
    with pytest.raises(ValueError, match=f"{N} rows \\+ 1 new rows exceed capacity={N}"):
        M.add(emb[:1], [{"chunk_id": "extra"}])
    for name, q in _queries(w).items():                          # the refused add left every query unchanged
        _same(M.query(query_embeddings=w["Q"], **q), base[name], ("after a refused add", name))
    with pytest.raises(ValueError, match="duplicate id 'c7'"):
        HipCollection(emb[:10], meta[:9] + [meta[7]], capacity=20, device="cuda:0")
    with pytest.raises(ValueError, match="world == 1"):
        HipCollection(emb[:10], meta[:10], capacity=20, world=2, device="cuda:0")

    # about a fifth of the rows: by ids, by a `where`, by a `where_document`
    by_id = sorted(rs.choice(N, size=200, replace=False).tolist())
    gone = np.zeros(N, bool)
    gone[by_id] = True
    assert M.delete(ids=[f"c{j}" for j in by_id]) == 200
    old = np.array([m["year"] < 1955 for m in meta])
    assert M.delete(where={"year": {"$lt": 1955}}) == int((old & ~gone).sum())
    gone |= old
    has = np.array([words[5] in m["text"] for m in meta])
    assert M.delete(where_document={"$contains": words[5]}) == int((has & ~gone).sum())
    gone |= has
    assert 0.15 < gone.mean() < 0.3 and M.count() == int((~gone).sum())
    with pytest.raises(ValueError, match="unknown id"):
        M.delete(ids=[f"c{by_id[0]}"])
    surv = np.nonzero(~gone)[0]
    F = HipCollection(emb[surv], [meta[r] for r in surv], **{**kw, "hybrid_filters": False})
    assert F.count() == M.count()

    for name, q in _queries(w).items():
        _same(M.query(query_embeddings=w["Q"], **q), F.query(query_embeddings=w["Q"], **q), ("before compact", name), index_map=surv)
    ids = [f"c{r}" for r in surv[[0, 17, len(surv) - 1]]]
    assert M.get(ids) == F.get(ids)

    mapping = M.compact()
    want_map = np.where(~gone, np.cumsum(~gone) - 1, -1)
    assert mapping.dtype == np.int64 and np.array_equal(mapping, want_map)
    assert M.count() == F.count() == M.index.n_rows and M._keep is None and M.get(ids) == F.get(ids)
    assert M.metadata == F.metadata
    for name, q in _queries(w).items():
        _same(M.query(query_embeddings=w["Q"], **q), F.query(query_embeddings=w["Q"], **q), ("after compact", name))
    hybrid = dict(query_embeddings=w["Q"], query_texts=w["qs"], n_results=10, n_candidates=20, hybrid_alpha=0.7)
    got, want = M.query(**hybrid), F.query(**hybrid)
    _same(got, want, "hybrid after compact")
    assert "hybrid_scores" in got and "keyword_scores" in got
    assert torch.equal(M.keyword.post_w.view(torch.int32), F.keyword.post_w.view(torch.int32))     # the rebuilt index is the fresh one
    assert torch.equal(M.keyword.term_ptr, F.keyword.term_ptr) and torch.equal(M.keyword.post_row, F.keyword.post_row)
    assert np.array_equal(M.compact(), np.arange(M.count()))    # nothing tombstoned: the identity

    # and it can grow again: a withdrawn paper's key may come back, the rows land behind the survivors
    back = [dict(meta[r], chunk_id=f"again{r}") for r in by_id[:5]]
    M.add(emb[by_id[:5]], [dict(m, paper_id="p-new") for m in back])
    F2 = HipCollection(np.concatenate([emb[surv], emb[by_id[:5]]]), [meta[r] for r in surv] + [dict(m, paper_id="p-new") for m in back],
                       **{**kw, "hybrid_filters": False})
    for name in ("plain", "where_document", "group_by"):
        q = _queries(w)[name]
        _same(M.query(query_embeddings=w["Q"], **q), F2.query(query_embeddings=w["Q"], **q), ("after compact and add", name))
    _same(M.query(**hybrid), F2.query(**hybrid), "hybrid after compact and add")


def test_dedup_is_extended_over_added_rows_only():
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    n, first = 600, 400
    emb = SO.unit_rows_f16(n, D, 3).astype(np.float32)
    emb[300:305] = emb[100:105]                                  # near-copies inside the first build,
    emb[450:460] = emb[10:20]                                    # of earlier rows in the added batch,
    emb[500:505] = emb[470:475]                                  # and of rows of the same batch
    emb[520] = emb[452]                                          # a copy of a copy: flagged onto the earliest
    meta = [{"chunk_id": f"c{j}", "text": f"t{j}", "year": 1950 + j % 70} for j in range(n)]
    Q = SO.unit_rows_f16(NQ, D, 4).astype(np.float32)
    M = HipCollection(emb[:first], meta[:first], capacity=n, dedup_threshold=0.999, device="cuda:0")
    assert len(M.duplicates) == 5
    M.add(emb[first:], meta[first:])
    F = HipCollection(emb, meta, dedup_threshold=0.999, device="cuda:0")
    assert len(F.duplicates) == 21 and repr(M.duplicates) == repr(F.duplicates)
    assert np.array_equal(M._keep_mask, F._keep_mask)
    for q in (dict(n_results=32), dict(n_results=10, where={"year": {"$gte": 1980}}), dict(n_results=100, min_score=0.1)):
        _same(M.query(query_embeddings=Q, **q), F.query(query_embeddings=Q, **q), q)
    with pytest.raises(ValueError, match="dedup_threshold"):
        M.delete(ids=["c3"])
    assert M.count() == n
