"""Hybrid search on the GPU: arx_bm25_search / arx_bm25_scores (csrc/bm25.hip), keyword.KeywordIndex, HipCollection(hybrid_alpha=) and the
CLI's --hybrid-alpha, checked against float64 (tests/bm25_fp64.py).

Budget of a row's score: T * 2^-24 * ref, T = the query's term count, ref = the float64 sum of the STORED f32 impacts (only the kernel's
additions are under test; the impacts themselves are checked against the float64 formula in tests/test_keyword_host.py).  Derived, not
measured: T - 1 f32 additions of positive numbers in a fixed order have relative error below (T-1) u / (1 - (T-1) u), u = 2^-24.
The definition also fixes the ORDER of the additions (ascending term id, f32), so the exact bits are reproducible with numpy f32 and
are asserted as well."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import config as C
from tests import bm25_fp64 as R
from tests.helpers import synthetic_vocab

pytestmark = pytest.mark.gpu

V = 600
EVERY, ABSENT, RARE = V - 1, V - 2, V - 3          # a term in every row / in none / planted by hand where a test wants it
U = 2.0 ** -24
TILE = 12288                          # the default tile of a shard larger than one tile


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_DOCS = {}


def docs_of(n_rows, seed=5):
    if (n_rows, seed) not in _DOCS:
        d = R.zipf_corpus(n_rows, V - 3, 10, seed=seed)
        _DOCS[(n_rows, seed)] = [x + [EVERY] for x in d]
    return _DOCS[(n_rows, seed)]


def make_index(docs, **kw):
    from arxiv_rag_amd.keyword import KeywordIndex
    return KeywordIndex(pieces=docs, vocab_size=V, **kw)


def stored(idx):
    """(term_ptr, rows int64, w32) of the index as it sits in HBM."""
    P = idx.n_postings
    return idx.term_ptr.cpu().numpy(), idx.post_row.cpu().numpy().view(np.uint32)[:P].astype(np.int64), idx.post_w.cpu().numpy()[:P]


def ref_scores(idx, terms):
    """-> (float64 sum of the stored impacts [n_rows], candidate mask, the exact f32 sum in ascending term order)."""
    tp, rows, w = stored(idx)
    s64 = np.zeros(idx.n_rows, np.float64); s32 = np.zeros(idx.n_rows, np.float32); has = np.zeros(idx.n_rows, bool)
    for t in sorted(terms):
        a, b = tp[t], tp[t + 1]
        s64[rows[a:b]] += w[a:b].astype(np.float64)
        s32[rows[a:b]] += w[a:b]
        has[rows[a:b]] = True
    return s64, has, s32


def query_sets(idx, seed=0):
    """Term lists of 1, 2, 17 and 64 terms (frequent and rare ones mixed), one with the term in every row, one with the absent term,
    one with no term at all."""
    rs = np.random.RandomState(seed)
    df = idx.stats.df
    present = np.flatnonzero(df[:V - 3] > 0)
    top = present[np.argsort(-df[present])]
    pick = lambda n: sorted(set(top[:max(2, n // 3)].tolist()) | set(rs.choice(present, size=min(n, len(present)), replace=False).tolist()))[:n]
    qs = [pick(1), pick(2), pick(17), pick(64), sorted(pick(5) + [EVERY]), sorted(pick(3) + [ABSENT]), [ABSENT], []]
    return [q for q in qs if len(q) <= len(present) + 2]


def check_rows(idx, terms, got, what):
    s64, has, s32 = ref_scores(idx, terms)
    T = max(len(terms), 1)
    err = np.abs(got.astype(np.float64) - s64)
    bud = T * U * s64
    worst = float((err[has] / bud[has]).max()) if has.any() else 0.0
    print(f"{what}: T={len(terms)} rows={idx.n_rows} candidates={int(has.sum())} worst error {worst:.3f} of the budget")
    assert (err <= bud).all(), what
    assert (got[~has] == 0).all() and (got[has] > 0).all(), what
    assert np.array_equal(got, s32), what                         # the fixed order of the f32 additions: exact bits


def check_topn(idx, terms, s, i, n, what):
    """in the manner of helpers.check_topk_fp64: ids are candidates, scores within budget, order, nothing better left out."""
    s64, has, s32 = ref_scores(idx, terms)
    T = max(len(terms), 1)
    bud = T * U * s64
    m = min(n, int(has.sum()))
    assert (i[m:] == -1).all() and np.isneginf(s[m:]).all(), what
    rows = i[:m] - idx.idx_base
    assert ((rows >= 0) & (rows < idx.n_rows)).all() and len(set(rows.tolist())) == m and has[rows].all(), what
    assert (np.abs(s[:m].astype(np.float64) - s64[rows]) <= bud[rows]).all(), what
    for a in range(m - 1):
        assert s[a] > s[a + 1] or (s[a] == s[a + 1] and rows[a] < rows[a + 1]), (what, a)
    if m:
        out = has.copy(); out[rows] = False
        last = rows[m - 1]
        assert (s64[out] <= s64[last] + bud[out] + bud[last]).all(), what
    # and the exact answer of the definition (f32 sums in term order, (score desc, row asc))
    cand = np.flatnonzero(has)
    order = cand[np.lexsort((cand, -s32[cand].astype(np.float64)))][:n]
    assert rows.tolist() == order.tolist() and np.array_equal(s[:m], s32[order]), what


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 777])
def test_per_row_scores_and_topn_vs_fp64(hip, n_rows):
    """Every shard size x every query family: dense scores through the debug tap, then the top-n lists (n = 32, 10, 1), at
    idx_base = 1 << 33."""
    idx = make_index(docs_of(n_rows), idx_base=1 << 33)
    qs = query_sets(idx)
    assert [len(q) for q in qs[:4]] == [1, 2, 17, 64] or n_rows < 100
    for qi, terms in enumerate(qs):
        got = idx.scores(terms).cpu().numpy()
        check_rows(idx, terms, got, f"rows={n_rows} query {qi}")
    for n in (32, 10, 1):
        s, i = idx.search(qs, n)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        for qi, terms in enumerate(qs):
            check_topn(idx, terms, s[qi], i[qi], n, f"rows={n_rows} n={n} query {qi}")
        assert (i[-1] == -1).all() and np.isneginf(s[-1]).all()                  # the query with zero terms
        assert (i[-2] == -1).all()                                               # only the absent term
        assert (i[len(qs) - 4][:min(n, n_rows)] >= (1 << 33)).all()                # the term in every row: min(n, rows) hits, global ids


def test_scores_tap_sub_ranges_and_tiles(hip):
    idx = make_index(docs_of(3 * TILE + 777))
    terms = query_sets(idx)[2]
    full = idx.scores(terms).cpu().numpy()
    for lo, hi, tile in [(0, idx.n_rows, 1024), (5, 5000, 0), (TILE - 3, TILE + 2050, 2048), (idx.n_rows - 1, idx.n_rows, 0)]:
        assert np.array_equal(idx.scores(terms, lo, hi, tile).cpu().numpy(), full[lo:hi]), (lo, hi, tile)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_all_ties_and_fewer_candidates_than_n(hip):
    doc = [3, 9, 9, 27, EVERY]
    for n_rows in (40, 2 * TILE + 5):
        idx = make_index([list(doc) for _ in range(n_rows)], idx_base=7)
        s, i = idx.search([[3, 9], [EVERY], [ABSENT, EVERY]], 32)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        for q in range(3):
            assert i[q].tolist() == list(range(7, 7 + 32)) and len(set(s[q].tolist())) == 1 and s[q, 0] > 0, (n_rows, q)
    docs = [list(d) for d in docs_of(TILE + 1)]
    for r, times in ((0, 1), (4097, 3), (TILE - 1, 1), (TILE, 2)):                  # a planted term in 4 rows, across the tile boundary
        docs[r] = docs[r] + [RARE] * times
    idx = make_index(docs)
    rare = [RARE]
    s, i = idx.search([rare], 32)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert sorted(i[0, :4].tolist()) == [0, 4097, TILE - 1, TILE] and (i[0, 4:] == -1).all() and np.isneginf(s[0, 4:]).all()
    check_topn(idx, rare, s[0], i[0], 32, "fewer candidates than n")


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_independence_of_batch_and_launch_shape(hip):
    idx = make_index(docs_of(3 * TILE + 777))
    qs = query_sets(idx, seed=1)
    probe = qs[2]
    rs = np.random.RandomState(2)
    present = np.flatnonzero(idx.stats.df > 0)
    filler = [sorted(set(rs.choice(present, size=rs.randint(1, 40)).tolist())) for _ in range(62)]
    alone = [t.cpu().numpy() for t in idx.search([probe], 32)]
    batch = [t.cpu().numpy() for t in idx.search([probe] + filler + [probe], 32)]
    assert len(batch[0]) == 64
    for pos in (0, 63):
        assert np.array_equal(batch[0][pos], alone[0][0]) and np.array_equal(batch[1][pos], alone[1][0]), pos
    base = [t.cpu().numpy() for t in idx.search(qs, 32)]
    for tile, blocks in [(1024, 0), (4096, 0), (12288, 1), (2048, 3), (1024, 128)]:
        got = [t.cpu().numpy() for t in idx.search(qs, 32, tile_rows=tile, max_blocks=blocks)]
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (tile, blocks)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_budget_catches_injected_faults(hip):
    """Faults on the REFERENCE side (nothing is provoked on the GPU): one query term dropped, tf ignored, dl of the neighbouring row.
    Each must exceed the budget by a wide factor."""
    docs = docs_of(3000, seed=9)
    idx = make_index(docs)
    df = idx.stats.df
    terms = sorted(np.argsort(-df[:V - 3])[:17].tolist())
    got = idx.scores(terms).cpu().numpy().astype(np.float64)
    T = len(terms)

    def factor(imp, tl):
        s, has = R.scores(R.stored_f32(imp), tl, len(docs))
        bud = T * U * np.maximum(s, 1e-30)
        return float((np.abs(got - s) / bud).max())

    clean = factor(R.impacts(docs, V), terms)
    print(f"clean reference: worst {clean:.3f} of the budget (the reference's own f32 rounding of the impacts may differ in the last bit)")
    assert clean <= 2.0            # an independent float64 formula: at most one f32 ulp per impact beside the additions
    for name, f in [("term dropped", factor(R.impacts(docs, V), terms[:-1])), ("tf ignored", factor(R.impacts(docs, V, fault="no_tf"), terms)),
                    ("dl of the neighbour", factor(R.impacts(docs, V, fault="dl_neighbour"), terms))]:
        print(f"fault '{name}': {f:.1f} x the budget")
        assert f > 10, name


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_one_index(hip):
    from arxiv_rag_amd.index import merge_partials
    from arxiv_rag_amd.keyword import KeywordStats
    docs = docs_of(TILE + 1)
    whole = make_index(docs, idx_base=100)
    cut = 5000
    a, b = make_index(docs[:cut], stats=whole.stats, idx_base=100), make_index(docs[cut:], stats=whole.stats, idx_base=100 + cut)
    m = a.local_stats.merge(b.local_stats)
    assert (m.N, m.total_len) == (whole.stats.N, whole.stats.total_len) and np.array_equal(m.df, whole.stats.df)
    assert isinstance(m, KeywordStats)
    qs = query_sets(whole, seed=3)
    for n in (32, 7):
        ws, wi = whole.search(qs, n)
        sa, ia = a.search(qs, n); sb, ib = b.search(qs, n)
        ms, mi = merge_partials(torch.stack([sa, sb]).contiguous(), torch.stack([ia, ib]).contiguous(), n)
        assert torch.equal(ms, ws) and torch.equal(mi, wi), n


# 6 ---------------------------------------------------------------------------------------------------------------------------------
class _RecordingReranker:
    def __init__(self):
        self.pairs = []

    def predict(self, pairs, batch_size=32, convert_to_numpy=True, **kw):
        self.pairs.extend(pairs)
        return np.array([float(len(t)) for _, t in pairs], np.float32)


def test_collection_hybrid_query(hip):
    from arxiv_rag_amd.keyword import KeywordIndex, fuse
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from oracle import search_oracle as SO
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    rare, common = words[-1], words[:-1]
    rs = np.random.RandomState(4)
    N, D, PLANT = 400, 128, 77
    texts = [" ".join(rs.choice(common, size=rs.randint(5, 30))) for _ in range(N)]
    texts[PLANT] = f"{common[3]} {rare} {common[8]} {rare}"
    qs = [f"{rare} {common[3]} {common[5]}"] + [" ".join(rs.choice(common, size=4)) for _ in range(5)]
    emb = SO.unit_rows_f16(N, D, 1).astype(np.float32)
    Q = SO.unit_rows_f16(len(qs), D, 2).astype(np.float32)
    emb[PLANT] = -Q[0]                                               # far in cosine from the query that shares its rare word
    meta = [{"chunk_id": f"c{j}", "text": t, "paper_id": "p", "section": "s", "quality_score": 1.0} for j, t in enumerate(texts)]
    plain = HipCollection(emb, meta, device="cuda:0")
    col = HipCollection(emb, meta, device="cuda:0", keyword=True, tokenizer=tok)
    assert plain.keyword is None and col.keyword.n_rows == N
    base = plain.query(query_embeddings=Q, n_results=10)
    assert col.query(query_embeddings=Q, query_texts=qs, n_results=10) == base       # hybrid_alpha=None: today's path
    assert PLANT not in base["indices"][0]
    with pytest.raises(ValueError):
        plain.query(query_embeddings=Q, query_texts=qs, hybrid_alpha=0.5)
    with pytest.raises(ValueError):
        col.query(query_embeddings=Q, hybrid_alpha=0.5)
    with pytest.raises(ValueError):
        col.query(query_embeddings=Q, query_texts=qs, hybrid_alpha=1.5)
    n = 32
    ds, di = [t.cpu().numpy() for t in col.index.search(torch.from_numpy(Q.astype(np.float16)).cuda(), n)]
    ks, ki = [t.cpu().numpy() for t in col.keyword.search(qs, n)]
    # the keyword list is the float64 reference's
    pieces = tok._full_pieces(texts)
    imp = R.stored_f32(R.impacts(pieces, cfg.vocab_size))
    for qi, terms in enumerate(col.keyword.query_terms(qs)):
        assert terms == R.query_terms(tok._full_pieces([qs[qi]])[0])
        rs64, has = R.scores(imp, terms, N)
        ref_s, ref_i = R.topn(rs64, has, n)
        m = int((ref_i >= 0).sum())
        assert np.allclose(ks[qi, :m], ref_s[:m], rtol=len(terms) * U * 4, atol=0) and (ki[qi, m:] == -1).all()
        gap = np.abs(np.diff(ref_s[:m])) > 1e-5 * ref_s[0]             # order asserted where float64 separates neighbours
        same = ki[qi, :m] == ref_i[:m]
        assert same[np.r_[True, gap] & np.r_[gap, True]].all(), qi
    a1 = col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=1.0)
    assert a1["indices"] == base["indices"] and a1["scores"] == base["scores"]
    a0 = col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=0.0)
    assert a0["indices"] == [ki[qi, :10].tolist() for qi in range(len(qs))]
    assert a0["keyword_scores"] == [ks[qi, :10].tolist() for qi in range(len(qs))]
    K = 20
    a7 = col.query(query_embeddings=Q, query_texts=qs, n_results=K, hybrid_alpha=0.7)
    f, fi, fd, fk = fuse(ds, di, ks, ki, 0.7, K)
    for qi in range(len(qs)):
        ref = R.fuse(list(zip(ds[qi], di[qi].tolist())), [(s, r) for s, r in zip(ks[qi], ki[qi].tolist()) if r >= 0], 0.7, K)
        assert a7["indices"][qi] == [r for _, r in ref] == fi[qi].tolist()
        assert a7["hybrid_scores"][qi] == [x for x, _ in ref]
        assert a7["ids"][qi] == [f"c{r}" for r in a7["indices"][qi]] and a7["documents"][qi] == [texts[r] for r in a7["indices"][qi]]
        for r, sc, kw in zip(a7["indices"][qi], a7["scores"][qi], a7["keyword_scores"][qi]):
            assert (np.isnan(sc) and r not in di[qi]) or sc == ds[qi][di[qi].tolist().index(r)]
            assert (np.isnan(kw) and r not in ki[qi]) or kw == ks[qi][ki[qi].tolist().index(r)]
    assert PLANT in a7["indices"][0] and ki[0, 0] == PLANT
    assert np.isnan(a7["scores"][0][a7["indices"][0].index(PLANT)])                   # it came from the keyword list only
    # with a reranker the cross-encoder receives the FUSED candidates
    rr = _RecordingReranker()
    b = col.query(query_embeddings=Q, query_texts=qs, n_results=3, hybrid_alpha=0.7, reranker=rr, n_candidates=K)
    f, fi, fd, fk = fuse(ds[:, :K], di[:, :K], ks[:, :K], ki[:, :K], 0.7, K)           # K candidates from each side, the fused top K
    for qi in range(len(qs)):
        handed = [t for q, t in rr.pairs if q == qs[qi]]
        assert sorted(handed) == sorted(texts[r] for r in fi[qi]), qi
        best = sorted(fi[qi].tolist(), key=lambda r: (-len(texts[r]), fi[qi].tolist().index(r)))[:3]
        assert b["indices"][qi] == best and len(b["hybrid_scores"][qi]) == 3 and len(b["rerank_scores"][qi]) == 3
        assert b["hybrid_scores"][qi] == [f[qi, fi[qi].tolist().index(r)] for r in best]


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_hybrid_alpha_on_gpu(hip, tmp_path, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.hub import load_sentence_encoder
    from arxiv_rag_amd.keyword import KeywordIndex, fuse
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import make_chunk_tree
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
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = [str(tmp_path / "in"), "--model", str(edir), "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    res = tmp_path / "embeddings_saved" / "search_results.json"

    def run(extra):
        GEN._model, GEN._model_name = None, None
        assert GEN.main(base + extra) == 0
        return json.loads(res.read_text())

    dense32, dense8 = run(["--top-k", "32"]), run(["--top-k", "8"])
    hyb = run(["--top-k", "8", "--hybrid-alpha", "0.7"])
    one = run(["--top-k", "8", "--hybrid-alpha", "1.0"])
    GEN._model, GEN._model_name = None, None
    assert all("hybrid_score" not in h for q in dense8 for h in q["results"])
    kept = GEN.load_chunks_parallel(tmp_path / "in", 0.0, 4)
    tok = load_sentence_encoder(str(edir)).tokenizer
    kw = KeywordIndex(texts=[c["text"] for c in kept], tokenizer=tok)
    ks, ki = [t.cpu().numpy() for t in kw.search(qs, 32)]
    for qi in range(len(qs)):
        ds = np.array([h["score"] for h in dense32[qi]["results"]], np.float32)
        di = np.array([h["index"] for h in dense32[qi]["results"]], np.int64)
        f, fi, fd, fk = fuse(ds, di, ks[qi], ki[qi], 0.7, 8)
        got = hyb[qi]["results"]
        assert [h["index"] for h in got] == fi[0].tolist() and [h["rank"] for h in got] == list(range(1, 9))
        assert np.allclose([h["hybrid_score"] for h in got], f[0], rtol=0, atol=1e-12)
        for h, d_, k_ in zip(got, fd[0], fk[0]):
            assert (h["score"] is None and np.isnan(d_)) or h["score"] == float(d_)
            assert (h["keyword_score"] is None and np.isnan(k_)) or h["keyword_score"] == float(k_)
            assert h["chunk_id"] == kept[h["index"]]["chunk_id"]
        assert [h["index"] for h in one[qi]["results"]] == [h["index"] for h in dense8[qi]["results"]]
    assert any(h["score"] is None for q in hyb for h in q["results"]) or any(
        [h["index"] for h in a["results"]] != [h["index"] for h in b["results"]] for a, b in zip(hyb, dense8))
