"""Cross-encoder reranking throughput and latency at the cross-encoder/ms-marco-MiniLM-L-6-v2 shape (seeded weights, token-level
pairs; no tokenisation in the timed region):
  * pairs/s for 1 024 pairs of a 16-token query + a 240-token passage (259 tokens per pair with [CLS] / [SEP]), 256 pairs per call;
  * latency of reranking ONE query's 32 candidates (one arx_encoder_score_pairs call), default and low-latency schedules.
Device time from hipEvents around the calls (median of --reps, after warm-up).  Prints one JSON line.

    python tools/rerank_bench.py [--reps 20] [--out profiles/rerank_bench.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import config as C  # noqa: E402
from arxiv_rag_amd.rerank import HipCrossEncoder  # noqa: E402
from arxiv_rag_amd.weights import seeded_pair_head, seeded_state_dict  # noqa: E402


def pairs(n, la, lb, vocab, seed):
    rs = np.random.RandomState(seed)
    L = la + lb + 3
    ids = np.concatenate([np.full((n, 1), 101), rs.randint(1000, vocab, (n, la)), np.full((n, 1), 102),
                          rs.randint(1000, vocab, (n, lb)), np.full((n, 1), 102)], 1).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    return dev(ids), dev(np.full(n, L)), dev(np.full(n, la + 2)), L


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rerank_bench needs a GPU"
    cfg = C.MS_MARCO_MINILM_L6
    enc = cfg.encoder
    sd = seeded_state_dict(enc, seed=0, std=0.05)
    head = seeded_pair_head(enc, cfg.n_labels, seed=1)
    res = {"shape": "ms-marco-MiniLM-L-6-v2 (6L/384, 12 heads of 32, 1 label), seeded weights", "device": torch.cuda.get_device_name(0)}
    m = HipCrossEncoder(cfg, {**sd, **head}, tokenizer=None, device="cuda:0")
    n, bs = 1024, 256
    ids, lens, seg, L = pairs(n, 16, 240, enc.vocab_size, 2)
    out = torch.empty((n, 1), dtype=torch.float32, device="cuda")

    def thr():
        for s0 in range(0, n, bs):
            m.score_device(ids[s0:s0 + bs], lens[s0:s0 + bs], seg[s0:s0 + bs], L, bs * L, out=out[s0:s0 + bs])
    ms = timed(thr, args.reps)
    res["throughput"] = {"pairs": n, "tokens_per_pair": L, "pairs_per_call": bs, "ms": ms, "pairs_per_s": n / ms * 1e3}
    m.close()
    q_ids, q_lens, q_seg, Lq = pairs(32, 16, 240, enc.vocab_size, 3)
    lat = {}
    for ll in (False, True):
        mq = HipCrossEncoder(cfg, {**sd, **head}, tokenizer=None, device="cuda:0", low_latency=ll)
        o = torch.empty((32, 1), dtype=torch.float32, device="cuda")
        lat["low_latency" if ll else "default"] = timed(lambda: mq.score_device(q_ids, q_lens, q_seg, Lq, 32 * Lq, out=o), args.reps)
        mq.close()
    res["query_32_candidates_ms"] = lat
    res["minilm_encode_seq_per_s_for_comparison"] = 118000      # profiles/r04/bench_minilm.json (single sentences, 256 tokens)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
