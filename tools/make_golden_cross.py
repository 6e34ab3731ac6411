"""Write tests/golden/tiny-cross-encoder.npz: tiny BertForSequenceClassification cross-encoders run by `transformers` (fp32, eval mode)
on sentence pairs tokenised by HF `tokenizers` with BERT's pair template ("[CLS] $A [SEP] $B:1 [SEP]:1", longest_first truncation).

Weights are not stored: each entry keeps its seed and the sha256 of the weights tests/cross_encoder_fp64.seeded_cross_weights
regenerates from it (encoder matrices rounded to bf16 BEFORE the model is built, so that transformers, the float64 reference and the GPU
all start from the same numbers).  Stored per entry: config, n_labels, seed, weight digest, ids, lens, type_ids, CLS hidden, logits.

    python tools/make_golden_cross.py
"""
import dataclasses
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import config as C  # noqa: E402
from arxiv_rag_amd.tokenizer import WordPieceTokenizer  # noqa: E402
from tests.cross_encoder_fp64 import seeded_cross_weights, weights_digest  # noqa: E402
from tests.helpers import synthetic_vocab  # noqa: E402

BASE = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=400, max_pos=64, max_seq_length=32)
ENTRIES = {            # name: (config, n_labels, seed)
    "dh32_l1": (dataclasses.replace(BASE, hidden=64, heads=2, ffn=128), 1, 11),
    "dh64_l3": (dataclasses.replace(BASE, hidden=128, heads=2, ffn=256), 3, 12),
}
MAX_LEN = 32


def pairs(vocab, seed):
    rs = np.random.RandomState(seed)
    words = [w for w in vocab if w.isalpha()]
    t = lambda n: " ".join(rs.choice(words, size=n))
    out = [(t(rs.randint(1, 8)), t(rs.randint(0, 20))) for _ in range(10)]
    out += [(t(40), t(3)), (t(2), t(50)), (t(30), t(35)), (t(5), ""), (t(14), t(15))]     # A cut, B cut, both cut, empty B, at the limit
    return out


def model(cfg, n_labels, sd, head):
    import torch
    from transformers import BertConfig, BertForSequenceClassification
    bc = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                    intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos, layer_norm_eps=cfg.ln_eps, type_vocab_size=2,
                    hidden_act="gelu", num_labels=n_labels, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    pad_token_id=cfg.pad_id)
    m = BertForSequenceClassification(bc).eval()
    state = {"bert." + k: torch.from_numpy(v) for k, v in sd.items()}
    state.update({("bert." + k if k.startswith("pooler.") else k): torch.from_numpy(v) for k, v in head.items()})
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    return m


def main():
    import torch
    out = {"names": np.array(list(ENTRIES))}
    for name, (cfg, n_labels, seed) in ENTRIES.items():
        vocab = synthetic_vocab(cfg)
        tok = WordPieceTokenizer.from_vocab(vocab, cfg, bert_pair=True)._tok
        tok.enable_truncation(max_length=MAX_LEN, strategy="longest_first")
        enc = tok.encode_batch(pairs(vocab, seed))
        n = len(enc)
        ids = np.zeros((n, MAX_LEN), np.int32); tt = np.zeros((n, MAX_LEN), np.int32); lens = np.zeros(n, np.int32)
        for i, e in enumerate(enc):
            ids[i, :len(e.ids)] = e.ids; tt[i, :len(e.ids)] = e.type_ids; lens[i] = len(e.ids)
        sd, head = seeded_cross_weights(cfg, n_labels, seed)
        m = model(cfg, n_labels, sd, head)
        with torch.no_grad():
            mask = torch.from_numpy((np.arange(MAX_LEN)[None] < lens[:, None]).astype(np.int64))
            o = m(input_ids=torch.from_numpy(ids.astype(np.int64)), token_type_ids=torch.from_numpy(tt.astype(np.int64)),
                  attention_mask=mask, output_hidden_states=True)
        out.update({f"{name}:cfg": np.array(cfg.to_json()), f"{name}:n_labels": np.int32(n_labels), f"{name}:seed": np.int64(seed),
                    f"{name}:wdigest": np.frombuffer(weights_digest(sd, head), np.uint8), f"{name}:ids": ids, f"{name}:lens": lens,
                    f"{name}:type_ids": tt, f"{name}:cls": o.hidden_states[-1][:, 0].numpy().astype(np.float32),
                    f"{name}:logits": o.logits.numpy().astype(np.float32)})
    dst = ROOT / "tests" / "golden" / "tiny-cross-encoder.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
