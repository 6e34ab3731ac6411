"""Hybrid search on the device: arx_bm25_search_wide (csrc/bm25.hip), arx_hybrid_fuse (csrc/fuse.hip), KeywordIndex.search_wide,
keyword.fuse_device, HipCollection(hybrid_on_device=True) and the CLI's --hybrid-on-device.

Every comparison is bit-exact against a definition that lives in the tree: the wide BM25 top-n against the f32 sum of the stored
impacts in ascending term order, ranked (score desc, row asc), and against `KeywordIndex.search` for n <= 32; the fusion against
`keyword.fuse`.  There is no tolerance anywhere in this file."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import config as C
from tests import bm25_fp64 as R
from tests.helpers import synthetic_vocab

pytestmark = pytest.mark.gpu

V = 48                                      # a small vocabulary: thousands of rows score above zero and many scores tie
EVERY, ABSENT, RARE = V - 1, V - 2, V - 3   # a term in every row / in none / planted by hand
NS = (1, 32, 33, 50, 1023, 1024)
SIZES = (1, 63, 1025, 12289, 30000)         # one row, a partial bitmap word, one 1024-row tile + 1, two default tiles, many blocks


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_CORPUS = {}


def corpus(n_rows):
    """(index, queries, reference) of one shard size, built once.  Documents are 1-4 terms of a 45-term Zipf vocabulary plus the term
    every row holds: few distinct (tf, dl) pairs, hence many equal scores.  RARE is planted in at most 5 rows."""
    if n_rows not in _CORPUS:
        from arxiv_rag_amd.keyword import KeywordIndex
        docs = [d[:1 + r % 4] + [EVERY] for r, d in enumerate(R.zipf_corpus(n_rows, V - 3, 4, seed=n_rows))]
        for r in sorted({0, n_rows // 3, n_rows // 2, n_rows - 2, n_rows - 1} & set(range(n_rows))):
            docs[r] = docs[r] + [RARE]
        idx = KeywordIndex(pieces=docs, vocab_size=V, idx_base=1 << 33)
        df = idx.stats.df
        top = [int(t) for t in np.argsort(-df[:V - 3])[:6] if df[t] > 0]
        qs = [sorted(top[:2]) or [EVERY], sorted(top), [EVERY], [RARE], sorted([RARE, ABSENT]), [ABSENT], []]
        _CORPUS[n_rows] = (idx, qs, [definition(idx, q) for q in qs])
    return _CORPUS[n_rows]


def definition(idx, terms):
    """-> (s32 [n_rows]: the f32 sum of the stored impacts in ascending term order; order: every candidate row by (score desc, row asc))."""
    P = idx.n_postings
    tp, rows, w = idx.term_ptr.cpu().numpy(), idx.post_row.cpu().numpy().view(np.uint32)[:P].astype(np.int64), idx.post_w.cpu().numpy()[:P]
    s32 = np.zeros(idx.n_rows, np.float32); has = np.zeros(idx.n_rows, bool)
    for t in sorted(terms):
        if 0 <= t < len(tp) - 1:
            a, b = tp[t], tp[t + 1]
            s32[rows[a:b]] += w[a:b]
            has[rows[a:b]] = True
    cand = np.flatnonzero(has)
    return s32, cand[np.lexsort((cand, -s32[cand].astype(np.float64)))]


def expected(idx, ref, n, ok=None):
    s32, order = ref
    if ok is not None:
        order = order[ok[order]]
    order = order[:n]
    s = np.full(n, -np.inf, np.float32); i = np.full(n, -1, np.int64)
    s[:len(order)], i[:len(order)] = s32[order], order + idx.idx_base
    return s, i


def same_bits(got_s, got_i, exp_s, exp_i):
    return np.array_equal(got_s.view(np.int32), exp_s.view(np.int32)) and np.array_equal(got_i, exp_i)


def host(pair):
    return [t.cpu().numpy() for t in pair]


# ---- wide BM25 against the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", SIZES)
def test_wide_topn_equals_the_definition_bit_for_bit(hip, n_rows):
    idx, qs, refs = corpus(n_rows)
    lists = {}
    for n in NS:
        s, i = lists[n] = host(idx.search_wide(qs, n))
        assert s.shape == (len(qs), n) and i.shape == (len(qs), n)
        for qi in range(len(qs)):
            es, ei = expected(idx, refs[qi], n)
            assert same_bits(s[qi], i[qi], es, ei), (n_rows, n, qi)
        assert (i[-1] == -1).all() and np.isneginf(s[-1]).all()              # the empty query
        assert (i[-2] == -1).all() and np.isneginf(s[-2]).all()              # only a term without postings
        m = min(n, n_rows)
        assert (i[2, :m] >= (1 << 33)).all() and (i[2, m:] == -1).all()      # the term in every row: min(n, rows) hits, global ids
        planted = len(refs[3][1])
        assert 1 <= planted <= 5 and (i[3, :min(n, planted)] >= 0).all() and (i[3, planted:] == -1).all()     # fewer candidates than n: pads
        assert same_bits(s[4], i[4], s[3], i[3])                             # a term without postings adds nothing
    for m, n in ((1, 32), (32, 33), (33, 50), (50, 1023), (1023, 1024)):     # the m-list is a prefix of the n-list
        assert same_bits(lists[n][0][:, :m], lists[n][1][:, :m], lists[m][0], lists[m][1]), (m, n)
    for n in (1, 10, 32):                                                    # n <= 32: KeywordIndex.search, exactly
        assert same_bits(*host(idx.search_wide(qs, n)), *host(idx.search(qs, n))), n


def test_wide_every_row_with_the_same_score_gives_the_first_rows(hip):
    from arxiv_rag_amd.keyword import KeywordIndex
    doc = [3, 9, 9, 27, EVERY]
    for n_rows in (40, 25000):
        idx = KeywordIndex(pieces=[list(doc) for _ in range(n_rows)], vocab_size=V, idx_base=7)
        for n in (33, 1024):
            s, i = host(idx.search_wide([[3, 9], [EVERY], [ABSENT, EVERY]], n))
            m = min(n, n_rows)
            for q in range(3):
                assert i[q, :m].tolist() == list(range(7, 7 + m)) and (i[q, m:] == -1).all(), (n_rows, n, q)
                assert len(set(s[q, :m].tolist())) == 1 and s[q, 0] > 0 and np.isneginf(s[q, m:]).all(), (n_rows, n, q)


def test_wide_term_outside_the_vocabulary_has_no_postings(hip, monkeypatch):
    """`pack_query_terms` refuses such a term on the host; here it is let through, and the kernel's own bound (t < vocab) must hold."""
    from arxiv_rag_amd import keyword as KW
    idx, qs, refs = corpus(1025)
    pack = KW.pack_query_terms
    monkeypatch.setattr(KW, "pack_query_terms", lambda lists, vocab: pack(lists, vocab + 1000))
    s, i = host(idx.search_wide([qs[0] + [V, V + 999], [V + 5]], 50))
    assert same_bits(s[0], i[0], *expected(idx, refs[0], 50))
    assert (i[1] == -1).all() and np.isneginf(s[1]).all()


def test_wide_bits_do_not_depend_on_the_launch_shape_or_the_batch(hip):
    """30 tiles of 1024 rows at n = 1024 are 30720 partial keys per query: far beyond the 4096 arx_topk_merge takes."""
    idx, qs, refs = corpus(30000)
    for n in (50, 1024):
        base = host(idx.search_wide(qs, n))
        for qi in range(len(qs)):
            assert same_bits(base[0][qi], base[1][qi], *expected(idx, refs[qi], n)), (n, qi)
        for tile in (1024, 2048, 0):
            for blocks in (1, 2, 3, 0):
                got = host(idx.search_wide(qs, n, tile_rows=tile, max_blocks=blocks))
                assert same_bits(*got, *base), (n, tile, blocks)
        alone = host(idx.search_wide([qs[1]], n))
        batch = host(idx.search_wide([qs[0], qs[3], qs[1], qs[2], qs[1]], n))
        for pos in (2, 4):
            assert same_bits(batch[0][pos], batch[1][pos], alone[0][0], alone[1][0]), (n, pos)


# ---- wide BM25 under a filter ----------------------------------------------------------------------------------------------------------
def test_wide_filtered_equals_the_definition_over_the_allowed_rows(hip):
    from arxiv_rag_amd.where import pack_bitmap
    idx, qs, refs = corpus(30000)
    n_rows = idx.n_rows
    rs = np.random.RandomState(8)
    eighth = np.zeros(n_rows, bool); eighth[n_rows // 2: n_rows // 2 + n_rows // 8] = True
    masks = [np.ones(n_rows, bool), eighth, rs.rand(n_rows) < 0.01]
    allow = torch.from_numpy(np.stack([pack_bitmap(m) for m in masks]).view(np.int64)).to(hip)
    queries = [qs[1], qs[1], qs[1], qs[2], qs[2], qs[0], qs[1], qs[2]]
    filter_of = [0, 1, 2, 2, 1, 0, -1, len(masks)]            # the last two: outside [0, n_filters) -> no row
    fo = torch.tensor(filter_of, dtype=torch.int32, device=hip)
    which = [1, 1, 1, 2, 2, 0, 1, 2]                          # refs[] entry of each slot's query: frequent terms, the term in every row
    for n in (32, 50, 1024):
        for kw in (dict(), dict(tile_rows=1024, max_blocks=3), dict(tile_rows=2048)):
            s, i = host(idx.search_wide(queries, n, allow=allow, filter_of=fo, **kw))
            for slot, (f, w) in enumerate(zip(filter_of, which)):
                ok = masks[f] if 0 <= f < len(masks) else np.zeros(n_rows, bool)
                assert same_bits(s[slot], i[slot], *expected(idx, refs[w], n, ok)), (n, kw, slot)
            assert (i[-2:] == -1).all() and np.isneginf(s[-2:]).all()
            assert (i[2] >= 0).sum() == min(n, int((masks[2] & (refs[1][0] > 0)).sum()))
    assert same_bits(*host(idx.search_wide(queries, 32, allow=allow, filter_of=fo)), *host(idx.search(queries, 32, allow=allow, filter_of=fo)))
    one = host(idx.search_wide(queries[:3], 50, allow=allow[1]))             # a single [W] bitmap, no filter_of: bitmap 0 for every query
    for slot in range(3):
        assert same_bits(one[0][slot], one[1][slot], *expected(idx, refs[1], 50, masks[1])), slot


# ---- fusion against keyword.fuse -------------------------------------------------------------------------------------------------------
def random_lists(rs, nq, n_dense, n_kw, base=0, pool=None, pads=True):
    """Two lists per query with distinct ids inside a list and partial overlap between them; some tails are pads (-inf, -1)."""
    pool = pool or 3 * max(n_dense, n_kw)
    ds = rs.standard_normal((nq, n_dense)).astype(np.float32); ks = (rs.rand(nq, n_kw) * 20).astype(np.float32)
    di = np.stack([rs.choice(pool, size=n_dense, replace=False) for _ in range(nq)]).astype(np.int64) + base
    ki = np.stack([rs.choice(pool, size=n_kw, replace=False) for _ in range(nq)]).astype(np.int64) + base
    ds, ks = -np.sort(-ds, axis=1), -np.sort(-ks, axis=1)
    if pads:
        for q in range(nq):
            a, b = rs.randint(0, n_dense + 1), rs.randint(0, n_kw + 1)
            if q % 3 == 1:
                ds[q, a:], di[q, a:] = -np.inf, -1
            if q % 3 == 2:
                ks[q, b:], ki[q, b:] = -np.inf, -1
    return ds, di, ks, ki


def check_fuse(hip, ds, di, ks, ki, alpha, k, what=""):
    from arxiv_rag_amd.keyword import fuse, fuse_device
    exp = fuse(ds, di, ks, ki, alpha, k)
    got = host(fuse_device(*(torch.from_numpy(np.ascontiguousarray(a)).to(hip) for a in (ds, di, ks, ki)), alpha, k))
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.float32 and got[3].dtype == np.float32
    assert np.array_equal(got[0].view(np.int64), exp[0].view(np.int64)), what            # the f64 bit patterns
    assert np.array_equal(got[1], exp[1]), what
    for g, e in ((got[2], exp[2]), (got[3], exp[3])):                                      # NaNs by position, bits elsewhere
        assert np.array_equal(np.isnan(g), np.isnan(e)), what
        assert np.array_equal(g[~np.isnan(g)].view(np.int32), e[~np.isnan(e)].view(np.int32)), what
    return got


@pytest.mark.parametrize("shape", [(32, 32, 10), (50, 50, 50), (7, 1024, 100), (1024, 1024, 1024)])
def test_fuse_random_lists_every_alpha(hip, shape):
    n_dense, n_kw, k = shape
    rs = np.random.RandomState(sum(shape))
    lists = random_lists(rs, 5, n_dense, n_kw)
    for alpha in (0.0, 0.3, 0.7, 1.0):
        check_fuse(hip, *lists, alpha, k, (shape, alpha))


def test_fuse_edge_lists(hip):
    rs = np.random.RandomState(1)
    ds, di, ks, ki = random_lists(rs, 4, 20, 30, pads=False)
    ds[0], di[0] = -np.inf, -1                                 # an all-pad dense list
    ks[1], ki[1] = -np.inf, -1                                 # an all-pad keyword list
    ds[2, 1:], di[2, 1:] = -np.inf, -1                         # a one-member list
    ks[3] = np.float32(2.5)                                    # a list whose scores are all equal
    for alpha in (0.0, 0.3, 0.7, 1.0):
        got = check_fuse(hip, ds, di, ks, ki, alpha, 64, alpha)            # k larger than the union: pads
        assert (got[1][:, 50:] == -1).all() and np.isneginf(got[0][:, 50:]).all() and np.isnan(got[2][:, 50:]).all()
    both = np.full((1, 4), -1, np.int64)
    got = check_fuse(hip, np.full((1, 4), -np.inf, np.float32), both, np.full((1, 4), -np.inf, np.float32), both, 0.7, 8)
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and np.isnan(got[2]).all() and np.isnan(got[3]).all()
    check_fuse(hip, ds[:, :1], di[:, :1], ks[:, :1], ki[:, :1], 0.7, 1)     # the smallest call


def test_fuse_ties_resolve_to_the_lower_row_and_ids_beyond_32_bits(hip):
    big = (1 << 32) + 5
    pat = np.array([[3.0, 2.0, 1.0, 0.0]], np.float32)
    di = np.array([[big + 7, big + 1, big - 9, big + 3]], np.int64)       # around 2^32 + 5, on both sides of 2^32
    ki = np.array([[big - 2, big + 6, big + 2, big - 8]], np.int64)
    got = check_fuse(hip, pat, di, pat * 4 + 1, ki, 0.5, 8)                 # the same normalised pattern on both sides
    assert got[1][0].tolist() == [big - 2, big + 7, big + 1, big + 6, big - 9, big + 2, big - 8, big + 3]
    assert all(got[0][0, j] == got[0][0, j + 1] for j in (0, 2, 4, 6)) and got[0][0, 0] == 0.5 and got[0][0, 7] == 0.0     # four ties
    # ids that differ only above bit 32 are different rows; the same row in both lists is one row
    di2 = np.array([[5, (1 << 32) + 5, (1 << 33) + 5, 6]], np.int64)
    ki2 = np.array([[(1 << 32) + 5, 5 + (1 << 34), 6, 7]], np.int64)
    got = check_fuse(hip, pat, di2, pat, ki2, 0.5, 8)
    assert sorted(got[1][0][got[1][0] >= 0].tolist()) == sorted({5, (1 << 32) + 5, (1 << 33) + 5, 6, 5 + (1 << 34), 7})
    rs = np.random.RandomState(3)
    check_fuse(hip, *random_lists(rs, 3, 50, 50, base=(1 << 32) - 40, pool=120), 0.7, 50)


def test_fuse_one_query_many_queries_and_independence_of_the_batch(hip):
    from arxiv_rag_amd.keyword import fuse_device
    rs = np.random.RandomState(2)
    lists = random_lists(rs, 65, 50, 50)
    got = check_fuse(hip, *lists, 0.7, 50)
    one = check_fuse(hip, *(a[17:18] for a in lists), 0.7, 50)
    for g, o in zip(got, one):
        assert np.array_equal(g[17:18], o, equal_nan=True)
    dev = [torch.from_numpy(a).to(hip) for a in lists]
    with pytest.raises(ValueError):
        fuse_device(*dev, 1.5, 10)
    with pytest.raises(ValueError):
        fuse_device(*dev, 0.5, 1025)
    with pytest.raises(ValueError):
        fuse_device(dev[0], dev[1][:, :7], dev[2], dev[3], 0.5, 10)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
class _RecordingReranker:
    def __init__(self):
        self.pairs, self.calls = [], []

    def predict(self, pairs, batch_size=32, convert_to_numpy=True, **kw):
        self.pairs.extend(pairs)
        self.calls.append((len(pairs), batch_size))
        return np.array([float(len(t)) for _, t in pairs], np.float32)


@pytest.fixture(scope="module")
def collections(hip):
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from oracle import search_oracle as SO
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    rs = np.random.RandomState(4)
    N, D = 400, 128
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(N)]
    qs = [" ".join(rs.choice(words, size=4)) for _ in range(6)]
    emb = SO.unit_rows_f16(N, D, 1).astype(np.float32)
    Q = SO.unit_rows_f16(len(qs), D, 2).astype(np.float32)
    meta = [{"chunk_id": f"c{j}", "text": t, "paper_id": "p", "section": "ab"[j % 2], "quality_score": 1.0} for j, t in enumerate(texts)]
    mk = lambda **kw: HipCollection(emb, meta, device="cuda:0", keyword=True, tokenizer=tok, **kw)
    return dict(host=mk(), dev=mk(hybrid_on_device=True), host_f=mk(hybrid_filters=True), dev_f=mk(hybrid_filters=True, hybrid_on_device=True),
                Q=Q, qs=qs, texts=texts, emb=emb, meta=meta)


def same_result(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key in ("scores", "distances", "hybrid_scores", "keyword_scores", "rerank_scores"):
            assert len(a[key]) == len(b[key])
            for x, y in zip(a[key], b[key]):
                x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
                assert np.array_equal(x.view(np.int64), y.view(np.int64)) or np.array_equal(x, y, equal_nan=True), key
        else:
            assert a[key] == b[key], key


def test_collection_with_the_flag_equals_the_default_path_up_to_32_candidates(hip, collections):
    from arxiv_rag_amd.store import HipCollection
    c = collections
    call = dict(query_embeddings=c["Q"], query_texts=c["qs"])
    for kw in (dict(n_results=10, hybrid_alpha=0.7), dict(n_results=32, hybrid_alpha=0.3), dict(n_results=5, hybrid_alpha=0.7, n_candidates=20),
               dict(n_results=10, hybrid_alpha=1.0), dict(n_results=10, hybrid_alpha=0.0), dict(n_results=10)):
        same_result(c["dev"].query(**call, **kw), c["host"].query(**call, **kw))
    a, b = _RecordingReranker(), _RecordingReranker()
    same_result(c["dev"].query(**call, n_results=3, hybrid_alpha=0.7, reranker=a, n_candidates=20),
                c["host"].query(**call, n_results=3, hybrid_alpha=0.7, reranker=b, n_candidates=20))
    assert a.pairs == b.pairs and a.calls == b.calls
    for where in ({"section": "a"}, [{"section": "a"}, None, {"section": "b"}, {"section": "a"}, None, {"section": "b"}]):
        got = c["dev_f"].query(**call, n_results=10, hybrid_alpha=0.7, where=where)
        same_result(got, c["host_f"].query(**call, n_results=10, hybrid_alpha=0.7, where=where))
        if isinstance(where, dict):
            assert all(r % 2 == 0 for rows in got["indices"] for r in rows)
    # the refusals that need nothing but the arguments, on a live collection
    with pytest.raises(ValueError, match=r"must be in \[n_results, 32\]"):
        c["host"].query(**call, hybrid_alpha=0.7, n_candidates=33)
    with pytest.raises(ValueError, match="at most 1024"):
        c["dev"].query(**call, hybrid_alpha=0.7, n_candidates=1025)
    with pytest.raises(ValueError, match="per-query filter lists"):
        c["dev_f"].query(**call, hybrid_alpha=0.7, n_candidates=50, where=[{"section": "a"}] * 6)
    with pytest.raises(ValueError, match="hybrid_on_device=True needs keyword=True"):
        HipCollection(c["emb"], c["meta"], device="cuda:0", hybrid_on_device=True)


def test_collection_with_50_candidates_equals_fuse_of_the_range_list_and_the_wide_keyword_list(hip, collections):
    from arxiv_rag_amd.keyword import fuse
    from arxiv_rag_amd.ranging import thresholds
    from arxiv_rag_amd.where import pack_bitmap
    c = collections
    col, Q, qs = c["dev"], c["Q"], c["qs"]
    qd = torch.from_numpy(Q.astype(np.float16)).to(hip)
    call = dict(query_embeddings=Q, query_texts=qs)
    n = 50
    ds, di, _ = host(col.index.search_range(qd, thresholds(float("-inf"), len(qs)), n))
    ks, ki = host(col.keyword.search_wide(qs, n))
    assert (di >= 0).all() and np.array_equal(ds[:, :32], host(col.index.search(qd, 32))[0])      # the range list has the search's bits
    K = 20
    got = col.query(**call, n_results=K, hybrid_alpha=0.7, n_candidates=n)
    f, fi, fd, fk = fuse(ds, di, ks, ki, 0.7, K)
    for qi in range(len(qs)):
        assert got["indices"][qi] == fi[qi].tolist() and got["hybrid_scores"][qi] == f[qi].tolist(), qi
        assert np.array_equal(np.asarray(got["scores"][qi], np.float32), fd[qi], equal_nan=True), qi
        assert np.array_equal(np.asarray(got["keyword_scores"][qi], np.float32), fk[qi], equal_nan=True), qi
        assert got["documents"][qi] == [c["texts"][r] for r in fi[qi]]
    # under a filter both long lists hold allowed rows only
    mask = np.array([m["section"] == "a" for m in c["meta"]])
    allow = torch.from_numpy(pack_bitmap(mask).view(np.int64)).to(hip)
    ds, di, _ = host(c["dev_f"].index.search_range(qd, thresholds(float("-inf"), len(qs)), n, allow=allow, n_allowed=int(mask.sum())))
    ks, ki = host(c["dev_f"].keyword.search_wide(qs, n, allow=allow))
    got = c["dev_f"].query(**call, n_results=K, hybrid_alpha=0.7, n_candidates=n, where={"section": "a"})
    f, fi, fd, fk = fuse(ds, di, ks, ki, 0.7, K)
    assert got["indices"] == [r.tolist() for r in fi] and all(mask[r] for rows in got["indices"] for r in rows)
    # with a reranker the cross-encoder receives the fused top 50, 32 pairs at a time
    rr = _RecordingReranker()
    ds, di, _ = host(col.index.search_range(qd, thresholds(float("-inf"), len(qs)), n))
    ks, ki = host(col.keyword.search_wide(qs, n))
    f, fi, fd, fk = fuse(ds, di, ks, ki, 0.7, n)
    b = col.query(**call, n_results=10, hybrid_alpha=0.7, reranker=rr, n_candidates=n)
    assert rr.calls and all(bs <= 32 for _, bs in rr.calls)
    for qi in range(len(qs)):
        handed = [t for q, t in rr.pairs if q == qs[qi]]
        assert len(handed) == n and sorted(handed) == sorted(c["texts"][r] for r in fi[qi]), qi
        best = sorted(fi[qi].tolist(), key=lambda r: (-len(c["texts"][r]), fi[qi].tolist().index(r)))[:10]
        assert b["indices"][qi] == best and b["hybrid_scores"][qi] == [f[qi, fi[qi].tolist().index(r)] for r in best]


def test_cli_hybrid_on_device(hip, tmp_path, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import make_chunk_tree
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    P = GEN.build_parser()
    recipe = ["in", "--queries", "q", "--hybrid-alpha", "0.7", "--rerank-model", "m", "--rerank-top-k", "50", "--top-k", "10"]
    assert GEN.check_rerank_args(P.parse_args(recipe)) == "--rerank-top-k 50: the search returns at most k <= 32 candidates per query"
    args = P.parse_args(recipe + ["--hybrid-on-device"])
    assert args.hybrid_on_device and GEN.check_rerank_args(args) is None and GEN.check_hybrid_device_args(args) is None
    emb_cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(emb_cfg)
    edir = tmp_path / "emb"
    save_hf_dir(edir, emb_cfg, seeded_state_dict(emb_cfg, seed=1, std=0.05))
    (edir / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n")
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    make_chunk_tree(tmp_path / "in", n_files=20, chunks_per_file=10, seed=1, words=words)
    qs = [" ".join(words[i:i + 5]) for i in range(0, 40, 5)]
    (tmp_path / "queries.txt").write_text("\n".join(qs) + "\n")
    monkeypatch.chdir(tmp_path)
    base = [str(tmp_path / "in"), "--model", str(edir), "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"),
            "--top-k", "8", "--hybrid-alpha", "0.7"]
    res = tmp_path / "embeddings_saved" / "search_results.json"

    def run(extra):
        GEN._model, GEN._model_name = None, None
        assert GEN.main(base + extra) == 0
        return json.loads(res.read_text())

    default, flagged = run([]), run(["--hybrid-on-device"])
    GEN._model, GEN._model_name = None, None
    assert flagged == default and all(len(q["results"]) == 8 and "hybrid_score" in q["results"][0] for q in flagged)
