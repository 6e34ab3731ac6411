"""Cross-encoder reranking on the GPU (arx_encoder_score_pairs, arx_pair_head_forward, rerank.HipCrossEncoder) checked against the
float64 chain of tests/cross_encoder_fp64.py.  Every budget is shown tight: the same data under one of that module's faults breaks it."""
import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib, config as C
from arxiv_rag_amd.weights import seeded_pair_head, seeded_state_dict
from tests.cross_encoder_fp64 import (cls_rows, embed_ln_pairs_fp64, encoder_pairs_fp64, head_budget, logit_bar, pair_head_fp64,
                                      score_pairs_fp64)
from tests.helpers import U8, synthetic_vocab

pytestmark = pytest.mark.gpu

EMBED_K = 0.05          # layer 0: the embedding budget of tests/test_gpu_encoder_fp64.py (one bf16 rounding + fp32 terms)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _cross_cfg(base=C.MS_MARCO_MINILM_L6, **kw):
    enc = dataclasses.replace(base.encoder, **kw)
    return C.CrossEncoderConfig(enc, base.n_labels, base.activation)


def _model(cfg, n_labels=1, seed=3, std=0.05, low_latency=False, max_length=None):
    from arxiv_rag_amd.rerank import HipCrossEncoder
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    enc = cfg.encoder
    sd = seeded_state_dict(enc, seed=seed, std=std, bias_std=0.05, ln_jitter=0.1)
    sd["embeddings.token_type_embeddings.weight"] = (np.random.RandomState(seed + 1).standard_normal((2, enc.hidden)) * 0.5).astype(np.float32)
    head = seeded_pair_head(enc, n_labels, seed=seed + 2, std=0.1)
    cfg = C.CrossEncoderConfig(enc, n_labels, C.default_activation(n_labels))
    vocab = synthetic_vocab(dataclasses.replace(enc, vocab_size=min(enc.vocab_size, 2000)))
    tok = WordPieceTokenizer.from_vocab(vocab, enc, bert_pair=True)
    return HipCrossEncoder(cfg, {**sd, **head}, tok, device="cuda:0", max_length=max_length, low_latency=low_latency), sd, head


def _pairs(enc, lens_a, lens_b, seed, max_len=512):
    """Token-level pairs: ids [n, S], lens, seg_b with [CLS]=2 / [SEP]=3 (synthetic_vocab's ids), truncated to max_len."""
    rs = np.random.RandomState(seed)
    rows = []
    for la, lb in zip(lens_a, lens_b):
        a = rs.randint(4, enc.vocab_size, size=la).tolist()
        b = rs.randint(4, enc.vocab_size, size=lb).tolist()
        row = ([2] + a + [3] + b + [3])[:max_len]
        rows.append((row, min(la + 2, len(row))))
    S = max(len(r) for r, _ in rows)
    ids = np.zeros((len(rows), S), np.int32)
    for i, (r, _) in enumerate(rows):
        ids[i, :len(r)] = r
    return ids, np.array([len(r) for r, _ in rows], np.int32), np.array([s for _, s in rows], np.int32)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_dim", [32, 64])
def test_layer0_segments_vs_fp64_and_plain_forward_bits(hip, head_dim):
    cfg = _cross_cfg(layers=2, heads=384 // head_dim)
    m, sd, head = _model(cfg)
    enc = cfg.encoder
    ids, lens, seg = _pairs(enc, [5, 1, 30, 0, 200, 12], [7, 40, 0, 9, 300, 1], seed=1)
    got = torch.from_numpy(m.tap_hidden(ids, lens, seg, 0)).cuda().double()
    ref = embed_ln_pairs_fp64(sd, enc, ids, lens, seg, device="cuda")
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    bud = U8 * ref.abs() + EMBED_K * U8 * rms
    worst = ((got - ref).abs() / bud).max().item()
    assert worst <= 1, worst
    for f in ("type0", "seg_late"):
        bad = embed_ln_pairs_fp64(sd, enc, ids, lens, seg, device="cuda", fault=f)
        assert ((bad - ref).abs() / bud).max().item() > 1, f
    # seg_b = NULL and seg_b >= lens: the plain forward's bits (layer 0 and logits)
    plain = m.encoder.tap_hidden(ids, lens, 0)
    assert np.array_equal(m.tap_hidden(ids, lens, None, 0), plain)
    assert np.array_equal(m.tap_hidden(ids, lens, lens + 3, 0), plain)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    T, S = int(lens.sum()), int(lens.max())
    l_null = m.score_device(d(ids), d(lens), None, S, T).cpu().numpy()
    l_big = m.score_device(d(ids), d(lens), d(lens), S, T).cpu().numpy()
    assert np.array_equal(l_null, l_big)
    # ... and the plain forward's CLS rows (normalize = 0) through the head alone give the same logits
    cls = m.encoder.forward_tokens(d(ids), d(lens), S, T, normalize=False)
    assert np.array_equal(_head_forward(cls, m._head_c, 1), l_null)


def _head_forward(cls, head_c, n_labels):
    out = torch.full((cls.shape[0], n_labels), float("nan"), dtype=torch.float32, device=cls.device)
    lib = _lib.load()
    _lib.check(lib.arx_pair_head_forward(cls.data_ptr(), cls.stride(0), cls.shape[0], cls.shape[1], ctypes.byref(head_c),
                                         out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream), "arx_pair_head_forward")
    return out.cpu().numpy()


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [384, 1024])
@pytest.mark.parametrize("n_labels", [1, 3])
def test_pair_head_forward_vs_fp64(hip, H, n_labels):
    """The head alone on random CLS rows within cross_encoder_fp64.head_budget (fp32 dots of length H: H 2^-23 sum |w||x| per stage,
    tanh within 4 ulp, the first stage carried through |W_c|); the pooler without tanh breaks it."""
    rs = np.random.RandomState(H + n_labels)
    enc = dataclasses.replace(C.MS_MARCO_MINILM_L6.encoder, hidden=H)
    head = seeded_pair_head(enc, n_labels, seed=H, std=1.0 / np.sqrt(H) * 2)
    n = 37
    x = torch.from_numpy((rs.standard_normal((n, H)) * 0.8).astype(np.float32)).cuda()
    tens = {k: torch.from_numpy(v).cuda() for k, v in head.items()}
    hc = _lib.PairHeadC(n_labels=n_labels)
    hc.pooler_w, hc.pooler_b = tens["pooler.dense.weight"].data_ptr(), tens["pooler.dense.bias"].data_ptr()
    hc.cls_w, hc.cls_b = tens["classifier.weight"].data_ptr(), tens["classifier.bias"].data_ptr()
    got = _head_forward(x, hc, n_labels)
    ref, _ = pair_head_fp64(x, head)
    bud = head_budget(x, head)
    worst = ((torch.from_numpy(got).cuda().double() - ref).abs() / bud).max().item()
    assert worst <= 1, worst
    bad, _ = pair_head_fp64(x, head, fault="no_tanh")
    assert ((bad - ref).abs() / bud).max().item() > 1
    # bitwise independent of the other rows of the launch and of n
    for r in (0, 17, 36):
        assert np.array_equal(_head_forward(x[r:r + 1].contiguous(), hc, n_labels)[0], got[r])
    assert _lib.load().arx_pair_head_forward(None, H, 0, H, ctypes.byref(hc), None, n_labels, None) == 0


# 3 / 4 --------------------------------------------------------------------------------------------------------------------------
def _cls_of(m, ids, lens, seg):
    """The f32 CLS rows the head reads for these pairs (one scoring call, arx_encoder_debug_cls)."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    ml = int(lens.max())
    m.score_device(d(ids[:, :ml]), d(lens), d(seg), ml, int(lens.sum()))
    return m.last_cls_rows(len(lens)).double()


def _check_logits(m, sd, head, cfg, ids, lens, seg, n_labels, what):
    """Logits within cross_encoder_fp64.logit_bar of the fp64 chain, the CLS rows they came from within the encoders' cosine bar;
    the faults (segment B as type 0, no tanh, pooler on the mean row) break the logit bar."""
    got = m.score_tokens(ids, lens, seg, batch_size=64).astype(np.float64)
    x = encoder_pairs_fp64(sd, cfg.encoder, ids, lens, seg, device="cuda")
    h_ref = cls_rows(x, lens)
    ref = pair_head_fp64(h_ref, head)[0].cpu().numpy()
    h = torch.cat([_cls_of(m, ids[s:s + 64], lens[s:s + 64], seg[s:s + 64]) for s in range(0, len(lens), 64)])
    cos = (h * h_ref).sum(1) / (h.norm(dim=1) * h_ref.norm(dim=1))
    assert cos.min().item() >= 1 - 1e-3, (what, cos.min().item())
    bar = logit_bar(h, h_ref, head).cpu().numpy()
    worst = (np.abs(got - ref) / bar).max()
    assert worst <= 1, (what, worst)
    faults = {"type0": score_pairs_fp64(sd, head, cfg.encoder, ids, lens, seg, device="cuda", fault="type0")[0],
              "no_tanh": pair_head_fp64(h_ref, head, fault="no_tanh")[0],
              "mean_pool": pair_head_fp64(cls_rows(x, lens, fault="mean_pool"), head)[0]}
    for f, bad in faults.items():
        assert (np.abs(bad.cpu().numpy() - ref) / bar).max() > 1, (what, f)
    return got, ref, bar, worst


@pytest.mark.parametrize("head_dim,n_labels", [(32, 1), (64, 3)])
def test_tiny_cross_encoder_end_to_end(hip, head_dim, n_labels):
    cfg = _cross_cfg(layers=2, hidden=128, heads=128 // head_dim, ffn=256, vocab_size=2000)
    m, sd, head = _model(cfg, n_labels=n_labels)
    ids, lens, seg = _pairs(cfg.encoder, [3, 9, 16, 1, 40, 5, 60], [20, 2, 16, 70, 0, 5, 100], seed=2, max_len=128)
    _check_logits(m, sd, head, cfg, ids, lens, seg, n_labels, f"tiny dh{head_dim} L{n_labels}")


def test_minilm_shape_64_queries_x_32_candidates(hip):
    cfg = C.MS_MARCO_MINILM_L6
    m, sd, head = _model(cfg, std=0.05)
    rs = np.random.RandomState(5)
    n_q, n_c = 64, 32
    la = np.repeat(rs.randint(4, 24, size=n_q), n_c)
    lb = np.where(rs.rand(n_q * n_c) < 0.1, rs.randint(300, 600, size=n_q * n_c), rs.randint(0, 260, size=n_q * n_c))
    ids, lens, seg = _pairs(cfg.encoder, la, lb, seed=6, max_len=512)
    got, ref, bar, worst = _check_logits(m, sd, head, cfg, ids, lens, seg, 1, "minilm")
    g, r, b = got[:, 0].reshape(n_q, n_c), ref[:, 0].reshape(n_q, n_c), bar[:, 0].reshape(n_q, n_c)
    for q in range(n_q):
        far = (r[q][:, None] - r[q][None, :]) > 2 * np.maximum(b[q][:, None], b[q][None, :])
        assert (g[q][:, None] > g[q][None, :])[far].all(), q
    print(f"minilm 64x32: worst/bar {worst:.3f}, median bar {np.median(b):.4g}, logit std {r.std():.4g}")


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_batch_composition_independence(hip):
    cfg = _cross_cfg(layers=2)
    m, _, _ = _model(cfg)
    rs = np.random.RandomState(9)
    n_q, n_c = 4, 32
    ids, lens, seg = _pairs(cfg.encoder, np.repeat(rs.randint(4, 20, size=n_q), n_c), rs.randint(0, 300, size=n_q * n_c), seed=10)
    all_ = m.score_tokens(ids, lens, seg, batch_size=n_q * n_c)
    perm = rs.permutation(n_q * n_c)
    shuffled = np.empty_like(all_)
    shuffled[perm] = m.score_tokens(ids[perm], lens[perm], seg[perm], batch_size=48)
    assert np.array_equal(all_, shuffled)
    for q in range(n_q):
        sl = slice(q * n_c, (q + 1) * n_c)
        assert np.array_equal(m.score_tokens(ids[sl], lens[sl], seg[sl], batch_size=n_c), all_[sl])
    for r in (0, 37, 127):
        assert np.array_equal(m.score_tokens(ids[r:r + 1], lens[r:r + 1], seg[r:r + 1]), all_[r:r + 1])


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_predict_and_rank_semantics(hip):
    cfg = _cross_cfg(layers=2, hidden=128, heads=4, ffn=256, vocab_size=2000)
    m, _, _ = _model(cfg, max_length=64)
    q = "abc de fgh"
    docs = ["abc de", "", "xyz " * 200, "abc de", "fgh ij kl"]
    s = m.predict([(q, d) for d in docs])
    assert s.shape == (5,) and ((s > 0) & (s < 1)).all()
    logits = m.predict([(q, d) for d in docs], activation_fct=lambda t: t)
    assert np.allclose(1 / (1 + np.exp(-logits)), s, atol=1e-6)
    assert s[0] == s[3]                                           # identical pairs, identical bits
    assert np.isscalar(m.predict((q, docs[0])).item()) and m.predict((q, docs[0])).item() == s[0]
    ids, lens, seg = m.tokenize_pairs([(q, docs[2])])
    assert lens[0] == 64                                          # longer than max_length: truncated
    hits = m.rank(q, docs, return_documents=True)
    assert [h["corpus_id"] for h in hits] == sorted(range(5), key=lambda j: (-s[j], j))
    assert hits[0]["text"] == docs[hits[0]["corpus_id"]]
    assert [h["corpus_id"] for h in hits].index(0) < [h["corpus_id"] for h in hits].index(3)      # tie: lower corpus_id first
    assert len(m.rank(q, docs, top_k=2)) == 2 and m.rank(q, []) == []
    m3, _, _ = _model(cfg, n_labels=3, max_length=64)
    p3 = m3.predict([(q, d) for d in docs])
    assert p3.shape == (5, 3)                                     # identity activation for 3 labels
    sm = m3.predict([(q, d) for d in docs], apply_softmax=True)
    assert np.allclose(sm.sum(1), 1, atol=1e-6)
    with pytest.raises(ValueError):
        m3.rank(q, docs)
    # opt-in low-latency schedule: same scores to rounding
    ml, _, _ = _model(cfg, max_length=64, low_latency=True)
    assert np.allclose(ml.predict([(q, d) for d in docs]), s, atol=2e-3)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_cli_rerank_and_collection_on_gpu(hip, tmp_path, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.rerank import HipCrossEncoder
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.weights import save_cross_encoder_dir, save_hf_dir
    from tests.helpers import make_chunk_tree
    emb_cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(emb_cfg)
    toks = "\n".join(sorted(vocab, key=vocab.get)) + "\n"
    edir = tmp_path / "emb"
    save_hf_dir(edir, emb_cfg, seeded_state_dict(emb_cfg, seed=1, std=0.05))
    (edir / "vocab.txt").write_text(toks)
    ccfg = dataclasses.replace(emb_cfg, max_pos=128, max_seq_length=128)
    csd = seeded_state_dict(ccfg, seed=2, std=0.08, bias_std=0.05, ln_jitter=0.1)
    head = seeded_pair_head(ccfg, 1, seed=3, std=0.2)
    rdir = tmp_path / "rr"
    save_cross_encoder_dir(rdir, ccfg, csd, head)
    (rdir / "vocab.txt").write_text(toks)
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    make_chunk_tree(tmp_path / "in", n_files=20, chunks_per_file=10, seed=1, words=words)
    qs = [" ".join(words[i:i + 5]) for i in range(0, 40, 5)]
    (tmp_path / "queries.txt").write_text("\n".join(qs) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = [str(tmp_path / "in"), "--model", str(edir), "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    GEN._model, GEN._model_name = None, None
    assert GEN.main(base + ["--top-k", "8"]) == 0
    plain = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
    GEN._model, GEN._model_name = None, None
    assert GEN.main(base + ["--rerank-model", str(rdir), "--rerank-top-k", "8", "--top-k", "3"]) == 0
    rer = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
    GEN._model, GEN._model_name = None, None
    kept = GEN.load_chunks_parallel(tmp_path / "in", 0.0, 4)
    rm = HipCrossEncoder.from_dir(str(rdir))
    n_checked = 0
    for p, r in zip(plain, rer):
        cands = {h["index"]: h["score"] for h in p["results"]}
        got = [h["index"] for h in r["results"]]
        assert len(got) == 3 and set(got) <= set(cands)                     # the candidates are the search's own
        assert all(h["score"] == cands[h["index"]] for h in r["results"])    # cosine score kept
        # fp64 reference order over the 8 candidates
        cl = list(cands)
        ids, lens, seg = rm.tokenize_pairs([(p["query"], kept[j]["text"]) for j in cl])
        ref = score_pairs_fp64({k: v for k, v in csd.items()}, head, rm.cfg.encoder, ids, lens, seg, device="cuda")[0][:, 0].cpu().numpy()
        gap = 1e-2 * (np.abs(ref).max() + 1e-3)             # order asserted where the reference separates the top 4 by 1 %
        order = sorted(range(len(cl)), key=lambda a: -ref[a])
        top = [cl[a] for a in order[:3]]
        if all(ref[order[a]] - ref[order[a + 1]] > gap for a in range(3)):
            assert got == top, (p["query"], got, top)
            n_checked += 1
        rs_ = [h["rerank_score"] for h in r["results"]]
        assert rs_ == sorted(rs_, reverse=True)
    assert n_checked >= 1
    # the collection path
    arr = np.load(tmp_path / "embeddings_saved" / "embeddings.npy").astype(np.float32)
    meta = json.loads((tmp_path / "embeddings_saved" / "metadata.json").read_text())
    col = HipCollection(arr, meta, device="cuda:0")
    from arxiv_rag_amd.hub import load_sentence_encoder
    se = load_sentence_encoder(str(edir))
    qv = se.encode(qs, normalize_embeddings=True, low_latency=True)
    a = col.query(query_embeddings=qv, n_results=8)
    b = col.query(query_embeddings=qv, query_texts=qs, n_results=3, reranker=rm, n_candidates=8)
    for qi in range(len(qs)):
        assert set(b["indices"][qi]) <= set(a["indices"][qi]) and len(b["indices"][qi]) == 3
        sc = rm.predict([(qs[qi], meta[j]["text"]) for j in a["indices"][qi]])
        best = [a["indices"][qi][t] for t in np.lexsort((np.arange(8), -sc))[:3]]
        assert b["indices"][qi] == best
        assert np.allclose(b["rerank_scores"][qi], np.sort(sc)[::-1][:3])


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_set_pair_head_refuses_mpnet_and_mean_pool(hip):
    from arxiv_rag_amd.encoder import HipEncoder
    for cfg in (C.TINY_MPNET, C.TINY_BERT):
        e = HipEncoder(cfg, seeded_state_dict(cfg, seed=0), device="cuda:0")
        w = torch.zeros(cfg.hidden * cfg.hidden + 4 * cfg.hidden, device="cuda")
        hc = _lib.PairHeadC(n_labels=1)
        hc.type_emb = hc.pooler_w = hc.pooler_b = hc.cls_w = hc.cls_b = w.data_ptr()
        assert e.lib.arx_encoder_set_pair_head(e._handle, ctypes.byref(hc)) == -1
        e.close()
