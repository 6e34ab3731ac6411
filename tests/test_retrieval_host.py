"""Host side of the shared retrieval pipeline (`arxiv_rag_amd/retrieval.py`, CPU): `RowFilters` on cpu tensors against a direct numpy
statement of every bitmap and count, the shared refusals in each front end's order, the chunk-count check of `search_queries`, and the
places the pipeline is stated once."""
import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
SIZES = (1, 63, 64, 65, 130)
WHERE = {"$or": [{"section": "Methods"}, {"year": {"$gte": 2010}}]}


def _shard(n, lo=0):
    rs = np.random.RandomState(n)
    meta = [{"section": ("abstract", "Methods", "Results")[int(rs.randint(3))], "year": int(2000 + rs.randint(20))} for _ in range(lo + n)]
    return meta, rs.rand(n) < 0.7


def _expect(meta, lo, n, where, keep):
    """The direct statement: evaluate the mask, and it with the keep-mask, pack, sum."""
    from arxiv_rag_amd.where import compile_where, evaluate, pack_bitmap
    if where is None and keep is None:
        return None, None
    mask = np.ones(n, bool) if where is None else evaluate(compile_where(where), meta, lo, lo + n)
    if keep is not None:
        mask = mask & keep
    return pack_bitmap(mask).view(np.int64), int(mask.sum())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lo", (0, 3))
def test_allow_of_is_the_packed_mask_and_its_sum(n, lo):
    from arxiv_rag_amd.retrieval import RowFilters
    meta, keep = _shard(n, lo)
    for where in (WHERE, None):
        for k in (keep, None):
            f = RowFilters(meta, "cpu", lo, lo + n, keep_mask=k)
            words, count = f.allow_of(where)
            want, total = _expect(meta, lo, n, where, k)
            if want is None:
                assert words is None and count is None
                continue
            assert words.dtype == torch.int64 and words.is_contiguous() and tuple(words.shape) == ((n + 63) // 64,)
            assert np.array_equal(words.numpy(), want) and count == total and type(count) is int, (n, where, k is not None)
    # a keep-bitmap the front end already holds on the device is the one that comes back
    held = torch.from_numpy(_expect(meta, lo, n, None, keep)[0].copy())
    assert RowFilters(meta, "cpu", lo, lo + n, keep_mask=keep, keep_words=held).allow_of(None)[0] is held


@pytest.mark.parametrize("n", SIZES)
def test_per_query_builds_one_bitmap_per_distinct_filter(n):
    from arxiv_rag_amd.retrieval import RowFilters
    meta, keep = _shard(n)
    other = {"year": {"$lt": 2005}}
    per_query = [WHERE, None, other, dict(WHERE), None, other]   # repeated filters (an equal dict is the same filter) and None entries
    for k in (keep, None):
        for count_both in (True, False):                         # (only a where and-ed with a where_document is ever left uncounted)
            bitmaps, filter_of, counts = RowFilters(meta, "cpu", keep_mask=k, count_both=count_both).per_query(len(per_query), per_query)
            assert list(filter_of) == [0, 1, 2, 0, 1, 2] and len(bitmaps) == len(counts) == 3
            for words, count, where in zip(bitmaps, counts, (WHERE, None, other)):
                want, total = _expect(meta, 0, n, where, k)
                if want is None:                                 # no filter at all for these queries: every row of the shard
                    want, total = np.full((n + 63) // 64, -1, np.int64), n
                assert np.array_equal(words.numpy(), want) and count == total, (n, where, k is not None)
    # a single dict (or None) is every query's filter
    bitmaps, filter_of, counts = RowFilters(meta, "cpu", keep_mask=keep).per_query(4, WHERE, None)
    want, total = _expect(meta, 0, n, WHERE, keep)
    assert list(filter_of) == [0] * 4 and len(bitmaps) == 1 and np.array_equal(bitmaps[0].numpy(), want) and counts == [total]


def test_a_list_of_the_wrong_length_is_refused_as_ever():
    from arxiv_rag_amd.retrieval import RowFilters
    meta, _ = _shard(10)
    with pytest.raises(ValueError) as e:
        RowFilters(meta, "cpu").per_query(3, [WHERE, None])
    assert str(e.value) == "where has 2 entries for 3 queries: a list needs one entry (a filter or None) per query"
    with pytest.raises(ValueError) as e:
        RowFilters(meta, "cpu").per_query(2, [WHERE, None], [None])
    assert str(e.value) == "where_document has 1 entries for 2 queries: a list needs one entry (a filter or None) per query"
    with pytest.raises(ValueError, match=r"where\[1\] must be a filter dict or None, got str"):
        RowFilters(meta, "cpu").per_query(2, [WHERE, "x"])


def test_a_front_end_without_texts_raises_its_own_refusal_before_any_filter_is_compiled():
    from arxiv_rag_amd.retrieval import RowFilters

    def no_texts():
        raise ValueError("no texts here")
    meta, _ = _shard(10)
    with pytest.raises(ValueError, match="no texts here"):
        RowFilters(meta, "cpu", documents=no_texts).per_query(2, [{"$bad": 1}, None], [None, {"$contains": "a"}])


NO_FILTER = " with hybrid_alpha: the BM25 keyword search has no row filter"
MMR = "mmr_lambda cannot be combined with reranker or hybrid_alpha: MMR re-orders the cosine search's candidates only"


def test_shared_refusals_come_in_the_front_ends_order_and_are_lifted_by_hybrid_filters():
    from arxiv_rag_amd.retrieval import check_shared_query

    def refusal(**kw):
        args = dict(hybrid_alpha=None, hybrid_filters=False, reranker=None, mmr_lambda=None, n_fetch=32, fetch_refusal="fetch!")
        with pytest.raises(ValueError) as e:
            check_shared_query(kw.pop("n_results", 10), **{**args, **kw})
        return str(e.value)
    first, late = (("A cannot be combined", False), ("B cannot be queried", True)), (("C cannot be combined", True), ("D cannot be combined", True))
    assert refusal(hybrid_alpha=0.5, filters_first=first, filters=late) == "B cannot be queried" + NO_FILTER
    assert refusal(hybrid_alpha=0.5, filters=late) == "C cannot be combined" + NO_FILTER
    assert refusal(hybrid_alpha=0.5, mmr_lambda=0.5, filters=late) == MMR                      # the filters after the mmr checks ...
    assert refusal(hybrid_alpha=0.5, mmr_lambda=0.5, filters_first=first) == "B cannot be queried" + NO_FILTER      # ... those before them
    assert refusal(hybrid_alpha=0.5, hybrid_filters=True, mmr_lambda=0.5, filters_first=first, filters=late) == MMR
    check_shared_query(10, hybrid_alpha=0.5, hybrid_filters=True, reranker=None, mmr_lambda=None, n_fetch=32, fetch_refusal="", filters_first=first,
                       filters=late)
    check_shared_query(10, hybrid_alpha=None, hybrid_filters=False, reranker=None, mmr_lambda=None, n_fetch=5, fetch_refusal="", filters=late)
    assert refusal(reranker=object(), mmr_lambda=0.5) == MMR
    assert refusal(mmr_lambda=1.5) == "mmr_lambda=1.5 must be in [0, 1]"
    assert refusal(mmr_lambda=float("nan")) == "mmr_lambda=nan must be in [0, 1]"
    for kw in (dict(n_fetch=9), dict(n_fetch=33), dict(n_results=0)):
        assert refusal(mmr_lambda=0.5, **kw) == "fetch!"
    check_shared_query(10, hybrid_alpha=None, hybrid_filters=False, reranker=None, mmr_lambda=0.0, n_fetch=10, fetch_refusal="fetch!")


def test_both_front_ends_word_the_fetch_refusal_as_ever(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.store import HipCollection
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError) as e:
        GEN.search_queries(None, [], None, ["q"], top_k=10, mmr_lambda=0.5, mmr_fetch_k=5)
    assert str(e.value) == "mmr_fetch_k=5 must be in [top_k, 32] (top_k=10)"
    coll = object.__new__(HipCollection)
    coll._keep = None
    with pytest.raises(ValueError) as e:
        coll.query(query_embeddings=np.zeros((1, 8)), n_results=10, n_candidates=5, mmr_lambda=0.5)
    assert str(e.value) == "n_candidates=5 must be in [n_results, 32] (the search's k limit) and n_results at least 1"


def test_chunk_count_check_names_the_first_mode_that_is_on():
    from arxiv_rag_amd.generate_embeddings_parallel import check_chunk_count
    chunks = [{}] * 5
    check_chunk_count(7, chunks)
    check_chunk_count(5, chunks, where={}, keep_mask=np.ones(5, bool), where_document={}, group_by_paper=True)
    cases = ((dict(where={}, where_document={}, group_by_paper=True), "where: 5 chunks for the shard's 7 rows"),
             (dict(where=[None] * 3), "where: 5 chunks for the shard's 7 rows"),
             (dict(keep_mask=np.ones(6, bool), where_document={}), "keep_mask: 6 entries for the shard's 7 rows"),
             (dict(keep_mask=np.ones(7, bool), where_document={}), "where_document: 5 chunks for the shard's 7 rows"),
             (dict(group_by_paper=True), "group_by_paper: 5 chunks for the shard's 7 rows"))
    for kw, text in cases:
        with pytest.raises(ValueError) as e:
            check_chunk_count(7, chunks, **kw)
        assert str(e.value) == text, kw


def test_the_pipeline_is_stated_once():
    src = {p.name: p.read_text() for p in (ROOT / "arxiv_rag_amd").glob("*.py")}
    for gone in ("_allow_of", "_and_with_of", "_bitmaps_on_device", "_per_query_bitmaps"):
        assert gone not in src["store.py"], gone
    gen = src["generate_embeddings_parallel.py"]
    body = gen[gen.index("def search_queries("):gen.index("def build_parser(")]
    for name in ("evaluate", "pack_bitmap", "DocumentStore", "MetadataColumns", "distinct_filters"):
        assert not re.search(rf"import[^\n]*\b{name}\b", body), name
    for text in ("the BM25 keyword search has no row filter\")", "mmr_lambda cannot be combined with reranker or hybrid_alpha", "mmr_lambda={mmr_lambda} must be in",
                 "for the shard's {n_rows} rows", "allow has {allow.shape[0]} words"):
        assert sum(s.count(text) for s in src.values()) == 1, text
