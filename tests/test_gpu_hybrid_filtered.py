"""Hybrid search under row filters on the GPU: arx_bm25_search_filtered (csrc/bm25.hip), `KeywordIndex.search(allow=, filter_of=)`,
`HipCollection(hybrid_filters=True)` and the CLI's --hybrid-filters.

The expected answer is numpy's alone: the f32 sum of the STORED impacts in ascending term order (`ref_scores` of tests/test_gpu_hybrid.py),
`has &= allowed`, lexsort by (score desc, row asc).  The definition fixes the order of the additions, so every comparison of scores
and ids is BIT-EXACT; there is no tolerance anywhere in this file."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import config as C
from arxiv_rag_amd.where import pack_bitmap
from tests.helpers import synthetic_vocab
from tests.test_gpu_hybrid import EVERY, RARE, TILE, _RecordingReranker, docs_of, make_index, query_sets, ref_scores

pytestmark = pytest.mark.gpu

BASE = 1 << 33
ROWS = (1, 63, 64, 65, 1024, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, 3 * TILE + 777)
TILES, BLOCKS, NS = (0, 1024, 2048, 12288), (0, 1, 3), (1, 10, 32)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def masks_of(n_rows, seed=0):
    """name -> bool [n_rows]: the issue's mask families."""
    rs = np.random.RandomState(1000 + seed + n_rows)
    r = np.arange(n_rows)
    out = {"ones": np.ones(n_rows, bool), "zeros": np.zeros(n_rows, bool), "first": r == 0, "last": r == n_rows - 1, "alternating": r % 2 == 1}
    # whole tiles skipped at every tile size in use: rows [12288, 24576) (empty on shards of one tile: the all-skipped case again)
    out["tile_aligned"] = (r >= TILE) & (r < 2 * TILE)
    # starts and ends inside a word, and inside a 1024-row tile
    lo = n_rows // 4
    out["mid_word"] = (r >= lo) & (r < min(n_rows, lo + 1000 + 37))
    for name, p in (("half", 0.5), ("percent", 0.01), ("permille", 0.001)):
        out[name] = rs.rand(n_rows) < p
    return out


def pack(masks, garbage_seed=None):
    """bool [F, n_rows] -> uint64 [F, W]; with a seed the bits at and beyond n_rows of every last word are random."""
    words = np.stack([pack_bitmap(m) for m in masks])
    n_rows = masks[0].shape[0]
    if garbage_seed is not None and n_rows % 64:
        g = np.random.RandomState(garbage_seed).randint(0, 1 << 62, size=len(words)).astype(np.uint64) | np.uint64(1 << 63)
        words[:, -1] |= g << np.uint64(n_rows % 64)
    return words


def on_device(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


class Reference:
    """Per (query, mask): the definition's ranking, computed once and shared (never modified)."""

    def __init__(self, idx, queries):
        self.idx, self.queries = idx, queries
        self.scored = [ref_scores(idx, q) for q in queries]                 # (s64, has, s32) per query
        self._memo = {}

    def ranking(self, qi, mask, key):
        if (qi, key) not in self._memo:
            _, has, s32 = self.scored[qi]
            cand = np.flatnonzero(has & mask)
            order = cand[np.lexsort((cand, -s32[cand].astype(np.float64)))][:32]
            self._memo[(qi, key)] = (s32[order], order + self.idx.idx_base)
        return self._memo[(qi, key)]

    def expect(self, pairs, n):
        """pairs: [(query index, mask or None, key)] -> (scores f32 [len, n], ids int64 [len, n]); None = no such filter."""
        s = np.full((len(pairs), n), -np.inf, np.float32); i = np.full((len(pairs), n), -1, np.int64)
        for j, (qi, mask, key) in enumerate(pairs):
            if mask is None:
                continue
            rs_, ri = self.ranking(qi, mask, key)
            m = min(n, len(ri))
            s[j, :m], i[j, :m] = rs_[:m], ri[:m]
        return s, i


def assert_bits(got, want, what):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, want[1]), (what, np.argwhere(gi != want[1])[:3].tolist())
    assert np.array_equal(gs.view(np.uint32), want[0].view(np.uint32)), (what, np.argwhere(gs != want[0])[:3].tolist())


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", ROWS)
def test_every_mask_family_x_query_family_x_launch_shape_bit_exact(hip, n_rows):
    """All (query family, mask family) pairs in ONE call (a bitmap per mask, filter_of per pair), at every tile size, block cap and n,
    at idx_base = 1 << 33; the bits beyond n_rows are garbage in half of the calls."""
    idx = make_index(docs_of(n_rows), idx_base=BASE)
    qs = query_sets(idx)
    masks = masks_of(n_rows)
    names = list(masks)
    ref = Reference(idx, qs)
    pairs = [(qi, masks[nm], nm) for qi in range(len(qs)) for nm in names]
    queries = [qs[qi] for qi, _, _ in pairs]
    fo = torch.tensor([names.index(nm) for _, _, nm in pairs], dtype=torch.int32, device="cuda")
    clean, dirty = on_device(pack(list(masks.values()))), on_device(pack(list(masks.values()), garbage_seed=n_rows))
    want = {n: ref.expect(pairs, n) for n in NS}
    calls = 0
    for tile in TILES:
        for blocks in BLOCKS:
            for n in NS:
                allow = dirty if calls % 2 else clean
                assert_bits(idx.search(queries, n, tile_rows=tile, max_blocks=blocks, allow=allow, filter_of=fo), want[n],
                            f"rows={n_rows} tile={tile} blocks={blocks} n={n}")
                calls += 1
    # the all-ones mask reproduces arx_bm25_search bit for bit; the all-zeros mask and an empty tile-aligned range return nothing
    plain = idx.search(qs, 32)
    ones = [j for j, (_, _, nm) in enumerate(pairs) if nm == "ones"]
    s32, i32 = want[32]
    assert np.array_equal(plain[1].cpu().numpy(), i32[ones]) and np.array_equal(plain[0].cpu().numpy().view(np.uint32), s32[ones].view(np.uint32))
    zeros = [j for j, (_, _, nm) in enumerate(pairs) if nm == "zeros"]
    assert (i32[zeros] == -1).all() and np.isneginf(s32[zeros]).all()
    every = [qi for qi, q in enumerate(qs) if EVERY in q]
    assert every or n_rows < 4
    if every:                                                  # the term in every row: every allowed row is a candidate
        at = {nm: k for k, (qi, _, nm) in enumerate(pairs) if qi == every[0]}
        assert (i32[at["half"]] >= 0).sum() == min(32, int(masks["half"].sum()))
        assert i32[at["last"]][0] == BASE + n_rows - 1 and (i32[at["last"]][1:] == -1).all()


def test_all_ones_with_garbage_beyond_n_rows_and_a_poisoned_padding_word(hip):
    """One bitmap inside a larger buffer: the words before and after it are all ones (rows that do not exist), the bits of its last word
    beyond n_rows are garbage.  The result is arx_bm25_search's."""
    for n_rows in (65, 2049, TILE + 1):
        idx = make_index(docs_of(n_rows), idx_base=BASE)
        qs = query_sets(idx)
        W = (n_rows + 63) // 64
        buf = torch.full((W + 2,), -1, dtype=torch.int64, device="cuda")
        buf[1:W + 1] = on_device(pack([np.ones(n_rows, bool)], garbage_seed=3))[0]
        allow = buf[1:W + 1]
        assert allow.is_contiguous() and allow.data_ptr() == buf.data_ptr() + 8
        for tile in (0, 1024):
            got, want = idx.search(qs, 32, tile_rows=tile, allow=allow), idx.search(qs, 32)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n_rows, tile)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_to_the_lower_row_across_a_tile_edge(hip):
    """Sixty identical documents in rows [1000, 1060): equal scores on both sides of the 1024-row tile edge."""
    docs = [list(d) for d in docs_of(2049)]
    for r in range(1000, 1060):
        docs[r] = [RARE, 3, 9]
    idx = make_index(docs, idx_base=BASE)
    rows = np.arange(2049)
    masks = {"ones": np.ones(2049, bool), "odd": rows % 2 == 1, "upper": rows >= 1020, "edge": (rows >= 1023) & (rows <= 1024),
             "lower_tile": rows < 1024, "upper_tile": rows >= 1024}
    qs = [[RARE], [3, RARE], [RARE, EVERY]]
    ref = Reference(idx, qs)
    assert len(set(ref.scored[0][2][1000:1060].tolist())) == 1
    pairs = [(qi, m, nm) for qi in range(len(qs)) for nm, m in masks.items()]
    fo = torch.tensor([list(masks).index(nm) for _, _, nm in pairs], dtype=torch.int32, device="cuda")
    allow = on_device(pack(list(masks.values())))
    for tile, blocks in ((0, 0), (1024, 0), (1024, 1), (2048, 0)):
        for n in (32, 10):
            want = ref.expect(pairs, n)
            assert_bits(idx.search([qs[qi] for qi, _, _ in pairs], n, tile_rows=tile, max_blocks=blocks, allow=allow, filter_of=fo), want,
                        (tile, blocks, n))
    i = ref.expect(pairs, 32)[1] - BASE
    assert i[0].tolist() == list(range(1000, 1032)) and i[1].tolist() == list(range(1001, 1060, 2)) + [-1 - BASE] * 2
    assert i[2].tolist() == list(range(1020, 1052)) and i[3, :2].tolist() == [1023, 1024] and i[5, 0] == 1024


# 3 ---------------------------------------------------------------------------------------------------------------------------------
_BIG = {}


def big_case():
    if not _BIG:
        n_rows = 3 * TILE + 777
        idx = make_index(docs_of(n_rows), idx_base=BASE)
        qs = query_sets(idx, seed=1)
        rs = np.random.RandomState(9)
        dens = [1.0, 0.5, 0.01, 0.001, 0.0] + rs.rand(195).tolist()
        masks = [rs.rand(n_rows) < p for p in dens]
        masks[7] = (np.arange(n_rows) >= TILE) & (np.arange(n_rows) < 2 * TILE + 100)
        _BIG.update(idx=idx, qs=qs, masks=masks, words=pack(masks, garbage_seed=5), ref=Reference(idx, qs))
    return _BIG


@pytest.mark.parametrize("n_filters", (1, 2, 64, 200))
def test_a_filter_per_query(hip, n_filters):
    """1, 2, 64 and 200 bitmaps in one call, filter_of shuffled, the same query under different filters, filter_of = -1 and = n_filters."""
    c = big_case()
    idx, qs, ref = c["idx"], c["qs"], c["ref"]
    rs = np.random.RandomState(n_filters)
    nq = max(24, n_filters + 8)
    q_of = [j % len(qs) for j in range(nq)]
    f_of = rs.permutation(np.arange(nq) % n_filters)
    f_of[3], f_of[11] = -1, n_filters                                      # no such filter: no row
    if n_filters > 1:
        q_of[0] = q_of[1] = q_of[2] = 2                                    # one query under three filters
        f_of[0], f_of[1], f_of[2] = 0, 1, n_filters - 1
    allow = on_device(c["words"][:n_filters])
    pairs = [(q_of[j], c["masks"][f_of[j]] if 0 <= f_of[j] < n_filters else None, int(f_of[j])) for j in range(nq)]
    fo = torch.tensor(f_of.astype(np.int32), device="cuda")
    queries = [qs[q] for q in q_of]
    want = ref.expect(pairs, 32)
    got = idx.search(queries, 32, allow=allow, filter_of=fo)
    assert_bits(got, want, n_filters)
    assert (want[1][[3, 11]] == -1).all() and np.isneginf(want[0][[3, 11]]).all()
    if n_filters > 1:
        assert not np.array_equal(want[1][0], want[1][1])
    # the batch in another order, other launch shapes
    order = rs.permutation(nq)
    order_d = torch.from_numpy(order).cuda()
    for tile, blocks in ((1024, 0), (2048, 3), (12288, 1)):
        again = idx.search([queries[j] for j in order], 32, tile_rows=tile, max_blocks=blocks, allow=allow, filter_of=fo[order_d].contiguous())
        assert torch.equal(again[0], got[0][order_d]) and torch.equal(again[1], got[1][order_d]), (tile, blocks)
    # query by query: the single-query, single-bitmap call
    shapes = ((0, 0), (1024, 0), (2048, 3), (12288, 1), (4096, 2))
    for t, j in enumerate(rs.choice(nq, size=12, replace=False).tolist() + [0, 1, 2]):
        if not (0 <= f_of[j] < n_filters):
            continue
        tile, blocks = shapes[t % len(shapes)]
        alone = idx.search([queries[j]], 32, tile_rows=tile, max_blocks=blocks, allow=allow[int(f_of[j])])
        assert torch.equal(alone[0][0], got[0][j]) and torch.equal(alone[1][0], got[1][j]), (j, tile, blocks)
    # filter_of = NULL is an all-zero filter_of
    a, b = idx.search(queries, 10, allow=allow), idx.search(queries, 10, allow=allow, filter_of=torch.zeros(nq, dtype=torch.int32, device="cuda"))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert_bits(a, ref.expect([(q, c["masks"][0], 0) for q in q_of], 10), "filter_of=None")


def test_keyword_index_slices_filter_of_with_the_queries_and_refuses_wrong_tensors(hip, monkeypatch):
    from arxiv_rag_amd.keyword import KeywordIndex
    c = big_case()
    idx, qs = c["idx"], c["qs"]
    allow = on_device(c["words"][:5])
    queries = [qs[j % len(qs)] for j in range(20)]
    fo = torch.tensor([(3 * j) % 5 for j in range(20)], dtype=torch.int32, device="cuda")
    whole = idx.search(queries, 10, allow=allow, filter_of=fo)
    assert KeywordIndex.QUERY_STEP == 4096
    monkeypatch.setattr(KeywordIndex, "QUERY_STEP", 7)                    # 7 + 7 + 6 queries
    cut = idx.search(queries, 10, allow=allow, filter_of=fo)
    assert torch.equal(cut[0], whole[0]) and torch.equal(cut[1], whole[1])
    plain = idx.search(queries, 10)                                        # allow=None: the unfiltered call, sliced the same way
    monkeypatch.undo()
    again = idx.search(queries, 10)
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])
    for kw in (dict(allow=allow[:, :-1]), dict(allow=allow.to(torch.int32)), dict(allow=allow.cpu()), dict(allow=allow, filter_of=fo[:-1]),
               dict(allow=allow, filter_of=fo.long()), dict(allow=allow, filter_of=fo.cpu()), dict(filter_of=fo)):
        with pytest.raises(ValueError, match="allow|filter_of"):
            idx.search(queries, 10, **kw)


@pytest.mark.parametrize("n", (1, 32))
def test_the_stated_workspace_is_enough_and_one_byte_less_is_refused(hip, n):
    """arx_bm25_search_tuned and arx_bm25_search_filtered_tuned called directly with exactly arx_bm25_workspace_bytes(...) bytes of an
    0xA5-filled buffer: 4097 rows in 1024-row tiles are five blocks per query and a merge.  The 256 bytes behind the stated need stay
    untouched and the answer is the definition's, bit for bit; with one byte less the call is refused and nothing is launched."""
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    n_rows, tile, nq = 4097, 1024, 3
    idx = make_index(docs_of(n_rows), idx_base=BASE)
    qs = [query_sets(idx)[j] for j in (1, 2, 4)]                             # 2 and 17 terms, and the term in every row
    rows = np.arange(n_rows)
    masks = [np.random.RandomState(7).rand(n_rows) < 0.5, rows % 3 == 0]
    f_of = [0, 1, 0]
    ref = Reference(idx, qs)
    from arxiv_rag_amd.keyword import pack_query_terms
    qt, qn = pack_query_terms(qs, idx.vocab_size)
    qt_d, qn_d = torch.from_numpy(qt).cuda(), torch.from_numpy(qn).cuda()
    allow, fo = on_device(pack(masks, garbage_seed=1)), torch.tensor(f_of, dtype=torch.int32, device="cuda")
    need = lib.arx_bm25_workspace_bytes(n_rows, nq, n)
    assert need == -(-5 * nq * n * 8 // 256) * 256                          # five blocks of 8-byte keys
    head = (idx.term_ptr.data_ptr(), idx.post_row.data_ptr(), idx.post_w.data_ptr(), idx.vocab_size, n_rows)
    st = torch.cuda.current_stream().cuda_stream
    cases = (("arx_bm25_search_tuned", (), [(q, np.ones(n_rows, bool), "ones") for q in range(nq)]),
             ("arx_bm25_search_filtered_tuned", (allow.data_ptr(), len(masks), fo.data_ptr()), [(q, masks[f_of[q]], f_of[q]) for q in range(nq)]))
    for name, filters, pairs in cases:
        def call(ws, ws_bytes, out_s, out_i):
            rc = getattr(lib, name)(*head, *filters, qt_d.data_ptr(), qn_d.data_ptr(), nq, n, out_s.data_ptr(), out_i.data_ptr(), BASE,
                                    ws.data_ptr(), ws_bytes, tile, 0, st)
            torch.cuda.synchronize()
            return rc
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        out_s = torch.zeros((nq, n), dtype=torch.float32, device="cuda"); out_i = torch.zeros((nq, n), dtype=torch.int64, device="cuda")
        assert call(ws, need, out_s, out_i) == 0, lib.arx_last_error().decode()
        assert (ws[need:] == 0xA5).all() and not (ws[:need] == 0xA5).all(), name
        assert_bits((out_s, out_i), ref.expect(pairs, n), (name, n))
        ws.fill_(0xA5); out_s.fill_(7.0); out_i.fill_(7)
        assert call(ws, need - 1, out_s, out_i) == -1 and "workspace too small" in lib.arx_last_error().decode(), name
        assert (ws == 0xA5).all() and (out_s == 7.0).all() and (out_i == 7).all(), name       # nothing was launched


# 4 ---------------------------------------------------------------------------------------------------------------------------------
SECTIONS =("abstract", "Introduction", "Methods", "Results")


def _collections():
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from oracle import search_oracle as SO
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:120]
    rs = np.random.RandomState(4)
    N, D, NQ = 1500, 128, 72
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(N)]
    emb = SO.unit_rows_f16(N, D, 1).astype(np.float32)
    emb[700:730] = emb[40:70]                                            # near-duplicates: rows 700..729 are dropped by dedup_threshold
    meta = [{"chunk_id": f"c{j}", "text": t, "paper_id": f"p{j // 8:04d}", "section": SECTIONS[int(rs.randint(4))], "quality_score": float(rs.rand()),
             "year": int(1950 + rs.randint(75))} for j, t in enumerate(texts)]
    qs = [" ".join(rs.choice(words, size=4)) for _ in range(NQ)]
    Q = SO.unit_rows_f16(NQ, D, 2).astype(np.float32)
    kw = dict(device="cuda:0", keyword=True, tokenizer=tok, documents=True, dedup_threshold=0.999)
    return dict(col=HipCollection(emb, meta, hybrid_filters=True, **kw), dev=HipCollection(emb, meta, hybrid_filters=True, where_on_device=True, **kw),
                old=HipCollection(emb, meta, **kw), meta=meta, texts=texts, qs=qs, Q=Q, words=words, N=N)


def _padded(lists_s, lists_i, n):
    s = np.full((len(lists_s), n), -np.inf, np.float32); i = np.full((len(lists_s), n), -1, np.int64)
    for q, (a, b) in enumerate(zip(lists_s, lists_i)):
        s[q, :len(a)], i[q, :len(b)] = a, b
    return s, i


def test_collection_hybrid_query_under_every_kind_of_filter(hip):
    from arxiv_rag_amd.keyword import fuse
    from arxiv_rag_amd.where import compile_where, evaluate
    c = _collections()
    col, dev, old, meta, texts, qs, Q, N = c["col"], c["dev"], c["old"], c["meta"], c["texts"], c["qs"], c["Q"], c["N"]
    keep = col._keep_mask
    assert col.hybrid_filters and not old.hybrid_filters and not keep[700:730].any() and keep.sum() == N - 30
    word = c["words"][3]
    one = {"$and": [{"section": {"$in": ["abstract", "Methods"]}}, {"year": {"$gte": 1970}}]}
    doc = {"$contains": word}
    per_query = [None if j % 9 == 4 else {"year": {"$gte": 1950 + j}} for j in range(len(qs))]          # 64 distinct filters + None = 65 bitmaps
    per_doc = [doc if j % 3 == 0 else None for j in range(len(qs))]
    from arxiv_rag_amd.filter_sets import distinct_filters
    assert len(distinct_filters(per_query, [None] * len(qs))[0]) > 64

    def mask_of(w, d):
        m = keep.copy()
        if w is not None:
            m &= evaluate(compile_where(w), meta, 0, N)
        if d is not None:
            m &= np.array([d["$contains"] in t for t in texts])
        return m

    cases = (("where", dict(where=one), [mask_of(one, None)] * len(qs)),
             ("where_document", dict(where_document=doc), [mask_of(None, doc)] * len(qs)),
             ("both", dict(where=one, where_document=doc), [mask_of(one, doc)] * len(qs)),
             ("dedup only", dict(), [mask_of(None, None)] * len(qs)),
             ("per query", dict(where=per_query), [mask_of(w, None) for w in per_query]),
             ("per query x2", dict(where=per_query, where_document=per_doc), [mask_of(w, d) for w, d in zip(per_query, per_doc)]),
             ("nothing allowed", dict(where={"paper_id": "nope"}), [np.zeros(N, bool)] * len(qs)))
    n, K = 32, 12
    for name, kwargs, masks in cases:
        # the two filtered candidate lists, fetched separately: dense through the collection, keyword with bitmaps packed HERE
        dense = col.query(query_embeddings=Q, n_results=n, **kwargs)
        ds, di = _padded(dense["scores"], dense["indices"], n)
        ks, ki = [t.cpu().numpy() for t in col.keyword.search(qs, n, allow=on_device(pack(masks)), filter_of=torch.arange(len(qs), dtype=torch.int32, device="cuda"))]
        f, fi, fd, fk = fuse(ds, di, ks, ki, 0.7, K)
        for which in (col, dev):
            got = which.query(query_embeddings=Q, query_texts=qs, n_results=K, hybrid_alpha=0.7, **kwargs)
            for q in range(len(qs)):
                m = int((fi[q] >= 0).sum())
                assert got["indices"][q] == fi[q, :m].tolist() and got["hybrid_scores"][q] == f[q, :m].tolist(), (name, q)
                assert all(masks[q][r] for r in got["indices"][q]), (name, q)            # its filter holds, and it is no duplicate
                for r, sc, kw_ in zip(got["indices"][q], got["scores"][q], got["keyword_scores"][q]):
                    assert (np.isnan(sc) and r not in di[q]) or sc == ds[q][di[q].tolist().index(r)]
                    assert (np.isnan(kw_) and r not in ki[q]) or kw_ == ks[q][ki[q].tolist().index(r)]
        # alpha = 1: the filtered dense ranking; alpha = 0: the filtered BM25 ranking
        a1 = col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=1.0, **kwargs)
        assert a1["indices"] == [r[:10] for r in dense["indices"]], name
        a0 = col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=0.0, **kwargs)
        f0, fi0, _, _ = fuse(ds, di, ks, ki, 0.0, 10)
        for q in range(len(qs)):
            assert a0["indices"][q] == fi0[q][fi0[q] >= 0].tolist(), (name, q)
            live = ks[q][ki[q] >= 0]                                       # (the keyword list's lowest score normalises to 0: those rows tie
            m = min(10, int((live > live.min()).sum())) if len(live) else 0  #  with the rows of the dense list alone, by row)
            assert a0["indices"][q][:m] == ki[q, :m].tolist(), (name, q)
        if name == "nothing allowed":
            assert all(r == [] for r in got["indices"])
        elif name == "where":
            assert sum(len(r) for r in got["indices"]) == K * len(qs)
    # with a reranker the cross-encoder receives the fused FILTERED candidates
    rr = _RecordingReranker()
    masks = [mask_of(w, None) for w in per_query]
    b = col.query(query_embeddings=Q, query_texts=qs, n_results=3, hybrid_alpha=0.7, reranker=rr, n_candidates=K, where=per_query)
    dense = col.query(query_embeddings=Q, n_results=K, where=per_query)
    ds, di = _padded(dense["scores"], dense["indices"], K)
    ks, ki = [t.cpu().numpy() for t in col.keyword.search(qs, K, allow=on_device(pack(masks)), filter_of=torch.arange(len(qs), dtype=torch.int32, device="cuda"))]
    f, fi, _, _ = fuse(ds, di, ks, ki, 0.7, K)
    handed = {}
    for q_text, t in rr.pairs:
        handed.setdefault(q_text, []).append(t)
    for q in range(len(qs)):
        if qs.count(qs[q]) == 1:
            assert sorted(handed[qs[q]]) == sorted(texts[r] for r in fi[q] if r >= 0), q
        assert len(b["indices"][q]) == 3 and all(masks[q][r] for r in b["indices"][q]) and len(b["rerank_scores"][q]) == 3
    # the same collection without the flag: the exact old messages
    old_text = "the BM25 keyword search has no row filter"
    for kwargs, text in ((dict(), "a collection built with dedup_threshold cannot be queried with hybrid_alpha: " + old_text),
                         (dict(where=per_query), "where cannot be combined with hybrid_alpha: " + old_text)):
        with pytest.raises(ValueError) as e:
            old.query(query_embeddings=Q, query_texts=qs, hybrid_alpha=0.7, **kwargs)
        assert str(e.value) == text


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_hybrid_filters_on_gpu(hip, tmp_path, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import make_chunk_tree
    emb_cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(emb_cfg)
    edir = tmp_path / "emb"
    save_hf_dir(edir, emb_cfg, seeded_state_dict(emb_cfg, seed=1, std=0.05))
    (edir / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n")
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    chunks = make_chunk_tree(tmp_path / "in", n_files=20, chunks_per_file=10, seed=1, words=words)
    section = {c["chunk_id"]: c["metadata"]["section"] for c in chunks}
    qs = [" ".join(words[i:i + 5]) for i in range(0, 40, 5)]
    (tmp_path / "queries.txt").write_text("\n".join(qs) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = [str(tmp_path / "in"), "--model", str(edir), "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"),
            "--top-k", "8", "--hybrid-alpha", "0.7"]
    res = tmp_path / "embeddings_saved" / "search_results.json"

    def run(extra, rc=0):
        GEN._model, GEN._model_name = None, None
        assert GEN.main(base + extra) == rc
        return json.loads(res.read_text()) if rc == 0 else None

    where = ["--where", json.dumps({"section": "Methods"})]
    run(where, rc=2)                                                          # refused without the flag, as before
    got = run(where + ["--hybrid-filters"])
    free = run([])
    GEN._model, GEN._model_name = None, None
    assert [r["query"] for r in got] == qs and all(len(r["results"]) == 8 for r in got)
    assert all(section[h["chunk_id"]] == "Methods" for r in got for h in r["results"])
    assert all("hybrid_score" in h and "keyword_score" in h for r in got for h in r["results"])
    assert any(h["keyword_score"] is not None for r in got for h in r["results"])
    assert any(section[h["chunk_id"]] != "Methods" for r in free for h in r["results"])     # the filter was what made the difference
