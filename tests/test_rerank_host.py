"""Cross-encoder reranking, host side (no GPU): BERT pair tokenisation vs HF tokenizers, the float64 reference vs transformers,
config / activation / weight parsing, the CLI flags, and the multi-rank rerank exchange over gloo."""
import copy
import dataclasses
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd.tokenizer import WordPieceTokenizer
from arxiv_rag_amd.weights import load_cross_encoder_dir, save_cross_encoder_dir, seeded_pair_head, seeded_state_dict
from tests.helpers import synthetic_vocab

ROOT = Path(__file__).resolve().parents[1]
TINY = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=400, max_pos=512, max_seq_length=512)


def _tok():
    return WordPieceTokenizer.from_vocab(synthetic_vocab(TINY), TINY, bert_pair=True)


def _hf_pairs(tok, pairs, max_len):
    t = copy.deepcopy(tok._tok)
    t.enable_truncation(max_length=max_len, strategy="longest_first")
    return t.encode_batch(list(pairs))


def _random_text(rs, words, n, unicode=False):
    out = list(rs.choice(words, size=n))
    if unicode and n:
        for _ in range(max(1, n // 4)):
            out[rs.randint(0, n)] = rs.choice(["héllo", "naïve", "日本語", "ü", "Ωmega", "café!"])
    return " ".join(out)


@pytest.mark.parametrize("max_len", [10, 11, 16, 32, 512])
@pytest.mark.parametrize("native", [True, False])
def test_pair_encoding_equals_hf_tokenizers(max_len, native, monkeypatch):
    monkeypatch.setenv("ARX_NATIVE_TOKENIZER", "1" if native else "0")
    tok = _tok()
    assert (tok._native is not None) == native
    vocab = synthetic_vocab(TINY)
    words = [w for w in vocab if w.isalpha()]
    rs = np.random.RandomState(max_len)
    pairs = []
    for i in range(300):
        hi = 700 if i % 10 == 0 else 25
        pairs.append((_random_text(rs, words, rs.randint(0, hi), unicode=i % 3 == 0),
                      _random_text(rs, words, rs.randint(0, hi), unicode=i % 5 == 0)))
    q = pairs[0][0]
    pairs += [(q, _random_text(rs, words, k)) for k in (0, 3, 40, 600)]         # one query, many candidates
    ids, lens, seg = tok.encode_pairs_packed(pairs, max_len)
    for r, e in enumerate(_hf_pairs(tok, pairs, max_len)):
        assert ids[r, :lens[r]].tolist() == e.ids, r
        assert (ids[r, lens[r]:] == TINY.pad_id).all()
        assert [0] * seg[r] + [1] * (lens[r] - seg[r]) == e.type_ids, r


@pytest.mark.parametrize("max_len,la,lb,ka,kb", [(10, 8, 8, 3, 4), (10, 12, 2, 5, 2), (10, 2, 12, 2, 5), (11, 5, 7, 4, 4)])
def test_longest_first_table(max_len, la, lb, ka, kb):
    """The truncation table of the issue, pinned against the library itself."""
    tok = _tok()
    a, b = " ".join(["a"] * la), " ".join(["b"] * lb)        # one word piece per word
    e = _hf_pairs(tok, [(a, b)], max_len)[0]
    assert e.type_ids.count(0) - 2 == ka and e.type_ids.count(1) - 1 == kb
    assert WordPieceTokenizer.pair_keep(la, lb, max_len - 3) == (ka, kb)
    ids, lens, seg = tok.encode_pairs_packed([(a, b)], max_len)
    assert seg[0] == ka + 2 and lens[0] == ka + kb + 3


def test_single_sentence_template_unchanged():
    v = synthetic_vocab(C.TINY_BERT)
    a = WordPieceTokenizer.from_vocab(v, C.TINY_BERT)
    b = WordPieceTokenizer.from_vocab(v, C.TINY_BERT, bert_pair=True)
    texts = ["abc de fgh", "x", ""]
    assert a.encode_batch(texts, 16) == b.encode_batch(texts, 16)
    pa = a._tok.encode("abc", "de").type_ids
    pb = b._tok.encode("abc", "de").type_ids
    assert set(pa) == {0} and pb[-2:] == [1, 1]


# ---- fp64 reference vs transformers -------------------------------------------------------------------------------------------
def test_fp64_reference_matches_golden_logits():
    """tests/golden/tiny-cross-encoder.npz (tools/make_golden_cross.py: transformers BertForSequenceClassification, fp32, weights
    rounded to bf16 first) reproduced by tests/cross_encoder_fp64 to fp32 accuracy; every fault moves the logits far outside it."""
    from tests.cross_encoder_fp64 import FAULTS, golden_weights, score_pairs_fp64
    g = np.load(ROOT / "tests" / "golden" / "tiny-cross-encoder.npz")
    for name in [str(n) for n in g["names"]]:
        enc = C.EncoderConfig(**json.loads(str(g[f"{name}:cfg"])))
        n_labels = int(g[f"{name}:n_labels"])
        sd, head = golden_weights(g, name, enc, n_labels)
        ids, lens, tt = g[f"{name}:ids"], g[f"{name}:lens"], g[f"{name}:type_ids"]
        seg = np.array([int(np.argmax(r[:l])) if r[:l].any() else l for r, l in zip(tt, lens)], np.int32)
        logits, h, _ = score_pairs_fp64(sd, head, enc, ids, lens, seg)
        want, want_h = g[f"{name}:logits"].astype(np.float64), g[f"{name}:cls"].astype(np.float64)
        tol = 1e-4 * (1 + np.abs(want).max())
        assert np.abs(logits.numpy() - want).max() < tol, name
        assert np.abs(h.numpy() - want_h).max() < 1e-4 * (1 + np.abs(want_h).max()), name
        for f in FAULTS:
            bad = score_pairs_fp64(sd, head, enc, ids, lens, seg, fault=f)[0].numpy()
            assert np.abs(bad - want).max() > 100 * tol, (name, f)


# ---- config / weights -----------------------------------------------------------------------------------------------------------
def test_cross_config_parsing(tmp_path):
    assert C.CROSS_PRESETS["cross-encoder/ms-marco-MiniLM-L-6-v2"] == C.MS_MARCO_MINILM_L6
    e = C.MS_MARCO_MINILM_L6.encoder
    assert (e.arch, e.hidden, e.layers, e.heads, e.ffn, e.pool, e.max_seq_length, C.MS_MARCO_MINILM_L6.n_labels) == \
        (C.ARCH_BERT, 384, 6, 12, 1536, C.POOL_CLS, 512, 1)
    sd = seeded_state_dict(TINY, seed=0)
    save_cross_encoder_dir(tmp_path / "m1", TINY, sd, seeded_pair_head(TINY, 1), n_labels=1)
    c1 = C.cross_config_from_hf_dir(tmp_path / "m1")
    assert c1.n_labels == 1 and c1.activation == C.ACT_SIGMOID and c1.encoder.pool == C.POOL_CLS and c1.encoder.hidden == TINY.hidden
    save_cross_encoder_dir(tmp_path / "m3", TINY, sd, seeded_pair_head(TINY, 3), n_labels=3)
    assert C.cross_config_from_hf_dir(tmp_path / "m3").activation == C.ACT_IDENTITY
    j = json.loads((tmp_path / "m3" / "config.json").read_text())
    j["sbert_ce_default_activation_function"] = "torch.nn.modules.activation.Sigmoid"
    (tmp_path / "m3" / "config.json").write_text(json.dumps(j))
    assert C.cross_config_from_hf_dir(tmp_path / "m3").activation == C.ACT_SIGMOID
    del j["sbert_ce_default_activation_function"]
    j["sentence_transformers"] = {"activation_fn": "torch.nn.modules.linear.Identity"}
    j["id2label"] = {"0": "LABEL_0"}
    (tmp_path / "m3" / "config.json").write_text(json.dumps(j))
    c = C.cross_config_from_hf_dir(tmp_path / "m3")
    assert c.n_labels == 1 and c.activation == C.ACT_IDENTITY
    j["architectures"] = ["BertModel"]
    (tmp_path / "m3" / "config.json").write_text(json.dumps(j))
    with pytest.raises(ValueError):
        C.cross_config_from_hf_dir(tmp_path / "m3")
    with pytest.raises(ValueError):
        C.parse_activation("torch.nn.modules.activation.Tanh")


def test_head_weights_load_and_missing_key(tmp_path):
    from safetensors.numpy import load_file, save_file
    sd = seeded_state_dict(TINY, seed=0)
    head = seeded_pair_head(TINY, 1, seed=1)
    save_cross_encoder_dir(tmp_path / "m", TINY, sd, head)
    sd2, head2 = load_cross_encoder_dir(tmp_path / "m", TINY, 1)
    assert set(sd2) == set(sd) and all(np.array_equal(sd2[k], sd[k]) for k in sd)
    assert all(np.array_equal(head2[k], head[k]) for k in head)
    assert sd2["embeddings.token_type_embeddings.weight"].shape == (2, TINY.hidden)
    raw = load_file(str(tmp_path / "m" / "model.safetensors"))
    del raw["classifier.bias"]
    save_file(raw, str(tmp_path / "m" / "model.safetensors"))
    with pytest.raises(KeyError):
        load_cross_encoder_dir(tmp_path / "m", TINY, 1)


def test_product_never_imports_transformers():
    for f in (ROOT / "arxiv_rag_amd").glob("*.py"):
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|transformers)\b", f.read_text(), re.M), f


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_rerank_flags(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    p = GEN.build_parser()
    a = p.parse_args(["in"])
    assert a.rerank_model is None and a.rerank_top_k == 32 and a.top_k == 10 and a.queries is None and a.batch_size == 200
    assert GEN.check_rerank_args(a) is None
    a = p.parse_args(["in", "--rerank-model", "m", "--rerank-top-k", "33"])
    assert "k <= 32" in GEN.check_rerank_args(a)
    a = p.parse_args(["in", "--rerank-model", "m", "--rerank-top-k", "5", "--top-k", "6"])
    assert "--top-k" in GEN.check_rerank_args(a)
    assert GEN.check_rerank_args(p.parse_args(["in", "--rerank-model", "m", "--rerank-top-k", "8", "--top-k", "3"])) is None
    assert GEN.main([str(tmp_path), "--rerank-model", "m", "--rerank-top-k", "64"]) == 2
    assert "k <= 32" in capsys.readouterr().out


def test_rerank_merge_order():
    from arxiv_rag_amd.rerank import rerank_candidates, reorder_by_rerank
    cand = np.array([[5, 3, 9, -1], [1, 2, 3, 4]])
    texts = {j: f"t{j}" for j in range(10)}
    sc = rerank_candidates(lambda pairs: [float(t[1:]) % 3 for _, t in pairs], ["q0", "q1"], cand, texts)
    got = reorder_by_rerank(cand, sc, 3)
    assert [[j for _, j, _ in g] for g in got] == [[5, 3, 9], [2, 1, 4]]       # ties keep the cosine order


_WORKER = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, os.environ["ARX_ROOT"])
import torch.distributed as dist
from arxiv_rag_amd.rerank import rerank_candidates, reorder_by_rerank
from arxiv_rag_amd.index import shard_bounds
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rs = np.random.RandomState(0)
N, Q, K = 101, 7, 8
texts_all = {j: " ".join(str(x) for x in rs.randint(0, 50, size=rs.randint(1, 9))) for j in range(N)}
queries = [f"q{i} " + str(i * 7 % 5) for i in range(Q)]
cand = np.stack([rs.choice(N, size=K, replace=False) for _ in range(Q)])
cand[2, -2:] = -1
lo, hi = shard_bounds(N, world, rank)
score = lambda pairs: np.array([(len(q) * 31 + sum(map(int, t.split()))) % 11 / 7.0 for q, t in pairs], np.float32)
mine = {j: t for j, t in texts_all.items() if lo <= j < hi}
sc = rerank_candidates(score, queries, cand, mine, dist=dist if world > 1 else None)
got = reorder_by_rerank(cand, sc, 5)
if rank == 0:
    print("RESULT", json.dumps([[(p, j, round(s, 6)) for p, j, s in g] for g in got]))
dist.barrier()
dist.destroy_process_group()
'''


def _run_world(tmp_path, world):
    w = tmp_path / "worker.py"
    w.write_text(_WORKER)
    env = {**os.environ, "ARX_ROOT": str(ROOT), "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", f"--nproc-per-node={world}", "--master-port",
                        str(29700 + world), str(w)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0]


def test_rerank_exchange_world_size_2_gloo_equals_world_1(tmp_path):
    assert _run_world(tmp_path, 2) == _run_world(tmp_path, 1)
