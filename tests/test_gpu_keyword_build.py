"""The BM25 index built on the device (`arx_bm25_build_postings`, `arx_bm25_build_impacts`, csrc/bm25_build.hip) against the host build
(`keyword.build_postings`, `keyword.impacts_f64`), bit for bit: trivial corpora, vocabulary sizes around the radix passes' digit
boundaries, runs and posting lists that cross tiles and blocks, document counts around a wave, token counts around the tile, every
launch shape, ids outside the vocabulary, impacts under local and under global statistics, and the three front ends."""
import dataclasses

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd import keyword as KW

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _zipf_lists(rs, n_docs, lo, hi, vocab, empty_every=0):
    """`n_docs` lists of lo..hi ids with Zipf-like frequencies over [0, vocab); every `empty_every`-th one empty."""
    p = 1.0 / np.arange(1, vocab + 1)
    cdf = np.cumsum(p / p.sum())
    out = []
    for r in range(n_docs):
        n = 0 if (empty_every and r % empty_every == empty_every - 1) else int(rs.randint(lo, hi + 1))
        out.append(np.minimum(np.searchsorted(cdf, rs.rand(n)), vocab - 1).astype(np.int64).tolist())
    return out


def _check(lists, vocab, **shape):
    """The device build of `lists` equals `build_postings`; -> (reference arrays, the device build)."""
    term_ptr, rows, tf, dl = KW.build_postings(lists, vocab)
    flat, doc_ptr = KW.flatten_pieces(lists)
    built = KW.build_postings_device(flat, doc_ptr, vocab, DEV, **shape)
    P = built.n_postings
    assert P == len(rows), (P, len(rows), shape)
    assert np.array_equal(built.term_ptr.cpu().numpy(), term_ptr), shape
    assert np.array_equal(built.term_ptr_host, term_ptr) and built.term_ptr_host.dtype == np.int64
    assert np.array_equal(built.post_row.cpu().numpy().view(np.uint32)[:P], rows), shape
    assert np.array_equal(built.post_tf.cpu().numpy()[:P], tf), shape
    assert np.array_equal(built.dl, dl)
    assert P == 0 or all(np.all(np.diff(rows[term_ptr[t]:term_ptr[t + 1]].astype(np.int64)) > 0) for t in np.unique(flat)[:50])
    return (term_ptr, rows, tf, dl), built


@pytest.fixture(scope="module")
def corpus():
    """About 5 000 documents x 0-300 Zipf pieces over V = 30 522, its host build, and a second disjoint shard for global statistics."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rs = np.random.RandomState(7)
    V = 30522
    lists = _zipf_lists(rs, 5000, 0, 300, V, empty_every=97)
    for p in lists:
        if p:
            p[0] = 5                                             # a term present in every non-empty document ...
    lists = [p if p else [] for p in lists]
    lists[10] = [5]                                              # ... tf = 1 in a one-piece document between two empty ones
    lists[9], lists[11] = [], []
    lists[0][:2] = [0, V - 1]
    other = _zipf_lists(rs, 1500, 20, 60, V)
    return dict(V=V, lists=lists, other=other, ref=KW.build_postings(lists, V))


def test_trivial_corpora():
    for lists in ([], [[], [], []], [[3]]):
        for V in (1, 7):
            _check([[0] * len(p) for p in lists] if V == 1 else lists, V)


@pytest.mark.parametrize("V", [1, 256, 257, 30522, 65537])
def test_vocabulary_edges(V):
    rs = np.random.RandomState(V)
    lists = [rs.randint(0, V, size=rs.randint(0, 40)).tolist() for _ in range(300)]
    lists[0] = [V - 1, 0, V - 1] + lists[0]
    lists[-1] = lists[-1] + [0, V - 1]
    (term_ptr, _, _, _), _ = _check(lists, V)
    assert term_ptr[1] > 0 and term_ptr[V] > term_ptr[V - 1]     # ids 0 and V - 1 are present


def test_run_boundaries():
    tile = KW.BUILD_TILE_TOKENS
    assert 5000 > 2 * tile
    (_, rows, tf, _), _ = _check([[1], [7] * 5000, [2, 7]], 10)                           # tf = 5000: one run over tiles and blocks
    assert 5000 in tf.tolist()
    rs = np.random.RandomState(1)
    lists = [[3] + rs.randint(0, 50, size=rs.randint(0, 6)).tolist() for _ in range(5000)]
    (term_ptr, _, _, _), _ = _check(lists, 50)                                            # a term in each of 5 000 documents
    assert term_ptr[4] - term_ptr[3] == 5000
    _check(lists, 50, tile_tokens=KW.BUILD_ROUND_TOKENS, max_blocks=7)


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 5000])
def test_document_counts_with_empty_documents_scattered_in(n_docs):
    rs = np.random.RandomState(n_docs)
    lists = [rs.randint(0, 1000, size=rs.randint(1, 12)).tolist() if rs.rand() < 0.7 else [] for _ in range(n_docs)]
    if n_docs > 1:
        lists[0], lists[-1] = [], []                             # empty at both ends
    _check(lists, 1000)


@pytest.mark.parametrize("edge", ["tile", "round"])
def test_token_counts_around_the_tile(edge):
    size = KW.BUILD_TILE_TOKENS if edge == "tile" else KW.BUILD_ROUND_TOKENS
    rs = np.random.RandomState(2)
    for n_tokens in (size - 1, size, size + 1, 2 * size - 1, 2 * size, 2 * size + 1):
        flat = rs.randint(0, 300, size=n_tokens)
        cuts = np.sort(rs.randint(0, n_tokens + 1, size=40))
        lists = [a.tolist() for a in np.split(flat, cuts)]
        _check(lists, 300)
        _check(lists, 300, tile_tokens=KW.BUILD_ROUND_TOKENS)


def test_launch_shapes_give_the_same_bits(corpus):
    for shape in (dict(max_blocks=1), dict(max_blocks=3), dict(), dict(tile_tokens=256), dict(tile_tokens=256, max_blocks=5),
                  dict(tile_tokens=65536, max_blocks=2)):
        _check(corpus["lists"], corpus["V"], **shape)


def test_bad_ids_raise_and_write_nothing_out_of_range():
    V, G = 100, 4096
    rs = np.random.RandomState(4)
    good = [rs.randint(0, V, size=rs.randint(0, 30)).tolist() for _ in range(200)]
    for bad_id in (-1, V, -(1 << 31), (1 << 31) - 1):
        lists = [list(p) for p in good]
        lists[77].insert(3, bad_id)
        with pytest.raises(ValueError) as host:
            KW.build_postings(lists, V)
        flat, doc_ptr = KW.flatten_pieces(lists)
        with pytest.raises(ValueError) as dev:
            KW.build_postings_device(flat, doc_ptr, V, DEV)
        assert str(dev.value) == str(host.value) == f"term id outside [0, {V})"
        # the same call on buffers with guard regions: the flag is set and the guards stay untouched
        T, n = len(flat), len(lists)
        tp = torch.full((G + V + 1 + G,), -7, dtype=torch.int64, device=DEV)
        pr = torch.full((G + T + G,), -7, dtype=torch.int32, device=DEV)
        pt = torch.full((G + T + G,), -7, dtype=torch.int32, device=DEV)
        np_ = torch.full((G + 1 + G,), -7, dtype=torch.int64, device=DEV)
        fl = torch.full((G + 1 + G,), -7, dtype=torch.int32, device=DEV)
        KW.build_postings_raw(torch.from_numpy(flat).to(DEV), torch.from_numpy(doc_ptr).to(DEV), T, n, V, tp[G:], pr[G:], pt[G:], np_[G:], fl[G:])
        torch.cuda.synchronize()
        assert int(fl[G]) != 0 and 0 <= int(np_[G]) <= T
        for buf, used in ((tp, V + 1), (pr, T), (pt, T), (np_, 1), (fl, 1)):
            assert bool((buf[:G] == -7).all()) and bool((buf[G + used:] == -7).all())
        assert bool((pr[G + int(np_[G]):G + T] == -7).all())     # nothing beyond the P postings either
    # and a clean corpus through the same guarded call leaves the flag at zero
    flat, doc_ptr = KW.flatten_pieces(good)
    fl = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    T = len(flat)
    out = [torch.empty(V + 1, dtype=torch.int64, device=DEV), torch.empty(T, dtype=torch.int32, device=DEV), torch.empty(T, dtype=torch.int32, device=DEV),
           torch.empty(1, dtype=torch.int64, device=DEV)]
    KW.build_postings_raw(torch.from_numpy(flat).to(DEV), torch.from_numpy(doc_ptr).to(DEV), T, len(good), V, *out, fl)
    assert int(fl[0]) == 0 and int(out[3][0]) == len(KW.build_postings(good, V)[1])


def test_impacts_under_local_and_global_statistics(corpus):
    V, lists = corpus["V"], corpus["lists"]
    term_ptr, rows, tf, dl = corpus["ref"]
    flat, doc_ptr = KW.flatten_pieces(lists)
    built = KW.build_postings_device(flat, doc_ptr, V, DEV)
    local = KW.KeywordStats.from_postings(term_ptr, dl)
    merged = local.merge(KW.KeywordStats.from_pieces(corpus["other"], V))                # the multi-rank case at world size 1
    assert merged.N != local.N and merged.avgdl != local.avgdl and np.any(merged.df != local.df)
    full = KW.KeywordStats(local.N, np.where(np.arange(V) == 5, local.N, local.df), local.total_len)      # a term with df = N
    assert full.df[5] == full.N
    r10 = int(np.flatnonzero(rows[term_ptr[5]:term_ptr[6]] == 10)[0] + term_ptr[5])
    assert tf[r10] == 1 and dl[9] == 0 and dl[11] == 0 and dl[10] == 1                    # tf = 1 between two zero-length documents
    for stats in (local, merged, full):
        want = KW.impacts_f64(term_ptr, rows, tf, dl, stats).astype(np.float32)
        got = KW.build_impacts_device(built, stats).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_keyword_index_built_on_the_device_is_the_default_index(corpus):
    V, lists = corpus["V"], corpus["lists"]
    stats = KW.KeywordStats.from_postings(corpus["ref"][0], corpus["ref"][3]).merge(KW.KeywordStats.from_pieces(corpus["other"], V))
    rs = np.random.RandomState(9)
    queries = [sorted(set([5] + rs.choice(lists[int(rs.randint(len(lists)))] or [1], size=6).tolist())) for _ in range(8)]
    for kw in (dict(), dict(stats=stats, idx_base=1000)):
        host = KW.KeywordIndex(pieces=lists, vocab_size=V, device=DEV, **kw)
        flat_pair = KW.flatten_pieces(lists)
        for pieces in (lists, flat_pair):
            dev = KW.KeywordIndex(pieces=pieces, vocab_size=V, device=DEV, build_on_device=True, **kw)
            for name in ("term_ptr", "post_row", "post_w"):
                a, b = getattr(host, name), getattr(dev, name)
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if name == "post_w" else a,
                                                                                b.view(torch.int32) if name == "post_w" else b), name
            assert (dev.n_rows, dev.n_postings, dev.vocab_size, dev.idx_base) == (host.n_rows, host.n_postings, host.vocab_size, host.idx_base)
            assert np.array_equal(dev.term_ptr_host, host.term_ptr_host) and np.array_equal(dev.posting_bytes(queries), host.posting_bytes(queries))
            for s in ("stats", "local_stats"):
                a, b = getattr(host, s), getattr(dev, s)
                assert (a.N, a.total_len) == (b.N, b.total_len) and np.array_equal(a.df, b.df)
            for fn in (lambda ix: ix.search(queries), lambda ix: ix.search_wide(queries, n=100)):
                (hs, hi), (ds, di) = fn(host), fn(dev)
                assert torch.equal(hs.view(torch.int32), ds.view(torch.int32)) and torch.equal(hi, di)
            assert torch.equal(host.scores(queries[0]).view(torch.int32), dev.scores(queries[0]).view(torch.int32))
    empty = KW.KeywordIndex(pieces=[[], []], vocab_size=V, device=DEV, build_on_device=True)
    assert empty.n_postings == 0 and empty.n_rows == 2 and int(empty.search([[5]])[1].max()) == -1


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """About 300 short texts behind a tiny in-process encoder, as tests/test_gpu_retrieval_front_ends.py builds them."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.hub import load_sentence_encoder
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import synthetic_vocab
    root = tmp_path_factory.mktemp("keyword_build")
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    save_hf_dir(root / "emb", cfg, seeded_state_dict(cfg, seed=1, std=0.05))
    (root / "emb" / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n", encoding="utf-8")
    model = load_sentence_encoder(str(root / "emb"))
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:120]
    rs = np.random.RandomState(11)
    texts = [" ".join(rs.choice(words, size=rs.randint(5, 30))) for _ in range(300)]
    texts[17], texts[40] = "", "naïve " + words[3]               # an empty chunk and one the native feeder hands to HF tokenizers
    chunks = [{"chunk_id": f"c{j}", "text": t, "metadata": {"year": int(1950 + rs.randint(75))}} for j, t in enumerate(texts)]
    sink = GEN.ShardSink(model, 0, len(texts))
    model.encode(texts, batch_size=64, normalize_embeddings=True, device_f16_out=sink.rows)
    torch.cuda.synchronize()
    qs = [" ".join(rs.choice(words, size=5)) for _ in range(4)]
    qd = torch.empty((4, 128), dtype=torch.float16, device="cuda")
    model.encode(qs, batch_size=256, normalize_embeddings=True, device_f16_out=qd, low_latency=True)      # as search_queries encodes them
    yield dict(GEN=GEN, model=model, chunks=chunks, sink=sink, qs=qs, Q=qd.cpu().numpy(), root=root, emb=sink.rows.cpu().numpy())
    model.encoder.close()


def test_collection_and_search_queries_answer_the_same_with_the_flag(world):
    from arxiv_rag_amd.store import HipCollection
    w = world
    meta = [{"chunk_id": c["chunk_id"], "text": c["text"], **c["metadata"]} for c in w["chunks"]]
    kw = dict(device=DEV, keyword=True, tokenizer=w["model"].tokenizer)
    default, flagged = HipCollection(w["emb"], meta, **kw), HipCollection(w["emb"], meta, keyword_build_on_device=True, **kw)
    assert torch.equal(default.keyword.post_w.view(torch.int32), flagged.keyword.post_w.view(torch.int32))
    a = default.query(query_embeddings=w["Q"], query_texts=w["qs"], n_results=10, hybrid_alpha=0.7)
    b = flagged.query(query_embeddings=w["Q"], query_texts=w["qs"], n_results=10, hybrid_alpha=0.7)
    assert a.keys() == b.keys() and repr(a) == repr(b)          # (repr: nan == nan, and the floats' every digit)
    assert len(a["indices"]) == 4 and all(len(r) == 10 for r in a["indices"])
    both = HipCollection(w["emb"], meta, keyword_build_on_device=True, hybrid_on_device=True, hybrid_filters=True, **kw)
    plain = HipCollection(w["emb"], meta, hybrid_on_device=True, hybrid_filters=True, **kw)
    q = dict(query_embeddings=w["Q"], query_texts=w["qs"], n_results=10, hybrid_alpha=0.7, n_candidates=50, where={"year": {"$gte": 1980}})
    assert repr(both.query(**q)) == repr(plain.query(**q))
    common = dict(top_k=10, output_dir=str(w["root"]), hybrid_alpha=0.7)
    hits = w["GEN"].search_queries(w["model"], w["chunks"], w["sink"], w["qs"], **common)
    hits_dev = w["GEN"].search_queries(w["model"], w["chunks"], w["sink"], w["qs"], keyword_build_on_device=True, **common)
    assert repr(hits) == repr(hits_dev) and [h["index"] for h in hits[0]["results"]] == a["indices"][0]
