#!/usr/bin/env python
"""Product-quantised search against the exact and the binary-code searches -> profiles/pq_bench.json (README, "product-quantised
search").

The shards of tools/binary_bench.py (`fill_clustered_rows`, dim 768, and the same rows plus a shared component) with a `pq.PqIndex`
(dsub 8, centre = the column mean, codebooks trained here) and a `binary.BinaryIndex` beside it.  Per arm Q x R: the median of 20 calls
of `PqIndex.search` (look-up tables and exact rescore included), the event spans of the `arx_pq_candidates` call alone, beside its floor
(the code array's n M bytes at the 6.29 TB/s copy rate, once per call), and of `arx_pq_lut` alone, recall@10 against
`ShardIndex.search` on the same queries, and, timed in turn in the same process, the exact search on the fp16 rows and with the int8
first pass and `BinaryIndex.search` at the same R with its recall.  Train and encode time per shard.  `loses` names the arms where the
PQ search is not faster than the better exact search, `slower_than_binary` those where it is not faster than the binary-code search.
No time or recall is a pass / fail gate.

    python tools/pq_bench.py --rows 1000000 10000000
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binary_bench import COPY_RATE, DIM, K, event_ms, median_ms, recall, shifted      # noqa: E402
from arxiv_rag_amd import pq as P                                                      # noqa: E402
from arxiv_rag_amd.binary import BinaryIndex                                           # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows                        # noqa: E402

DSUB = 8


def timed_build(index, train_rows, iters):
    """-> (PqIndex, train seconds, encode seconds): what `PqIndex.build(centre="mean")` does, its two steps timed apart."""
    n = int(index.n_rows)
    rows = index.corpus[:n]
    centre = rows.mean(dim=0, dtype=torch.float32).contiguous()
    pick = torch.randperm(n, device=rows.device, generator=torch.Generator(rows.device).manual_seed(0))[:train_rows].sort().values
    sample = rows[pick].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cb = P.train(sample, DSUB, centre, iters=iters, seed=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    codes = P.encode_device(rows, DSUB, centre, cb)
    torch.cuda.synchronize()
    return P.PqIndex(index, codes, cb, centre, DSUB), t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--candidates", type=int, nargs="+", default=[40, 128, 256])
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "pq_bench.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    report = {"dim": DIM, "dsub": DSUB, "k": K, "copy_rate_bytes_per_s": COPY_RATE, "train_rows": args.train_rows, "train_iters": args.iters,
              "shards": []}
    for n in args.rows:
        X = fill_clustered_rows(n, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev)
        exact16, exact8 = ShardIndex(X, prefilter=None), ShardIndex(X, prefilter="int8")
        pi, train_s, encode_s = timed_build(exact16, args.train_rows, args.iters)
        bi = BinaryIndex.build(exact16, centre="mean")
        shard = {"rows": n, "train_seconds": train_s, "encode_seconds": encode_s, "code_bytes": int(pi.codes.numel()),
                 "scan_floor_ms": pi.codes.numel() / COPY_RATE * 1e3, "arms": [], "loses": [], "slower_than_binary": []}
        print(f"rows {n}: train {train_s:.2f} s, encode {encode_s:.2f} s", flush=True)
        for nq in args.queries:
            q = fill_clustered_rows(nq, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=n + 12345)
            fp16_ms = median_ms(lambda: exact16.search(q, K))
            int8_ms = median_ms(lambda: exact8.search(q, K))
            truth = exact16.search(q, K)[1]
            lut = pi.lut(q)
            lut_ms = event_ms(lambda: pi.lut(q))
            for R in args.candidates:
                ms = median_ms(lambda: pi.search(q, K, R))
                scan_ms = event_ms(lambda: P.candidates_device(pi.codes, lut, DSUB, R, ws=pi._workspace(nq, R), want_sum=False))
                bin_ms = median_ms(lambda: bi.search(q, K, R))
                arm = {"queries": nq, "candidates": R, "pq_ms": ms, "scan_event_ms": scan_ms, "lut_event_ms": lut_ms, "exact_fp16_ms": fp16_ms,
                       "exact_int8_ms": int8_ms, "binary_ms": bin_ms, "recall_at_10": recall(pi.search(q, K, R)[1], truth),
                       "binary_recall_at_10": recall(bi.search(q, K, R)[1], truth)}
                shard["arms"].append(arm)
                print(json.dumps(arm), flush=True)
                if ms >= min(fp16_ms, int8_ms):
                    shard["loses"].append({"queries": nq, "candidates": R})
                if ms >= bin_ms:
                    shard["slower_than_binary"].append({"queries": nq, "candidates": R})
        # rows with a strong shared component: what the sign bits tell apart badly
        Y = shifted(X)
        del exact8, bi, pi
        ey = ShardIndex(Y, prefilter=None)
        q = shifted(fill_clustered_rows(64, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=n + 12345))
        truth = ey.search(q, K)[1]
        shard["shared_component"] = {"mean_pairwise_cosine": float((Y[:4096].float() @ Y[4096:8192].float().T).mean()), "arms": []}
        py, by = timed_build(ey, args.train_rows, args.iters)[0], BinaryIndex.build(ey, centre="mean")
        for R in args.candidates:
            arm = {"centre": "mean", "candidates": R, "recall_at_10": recall(py.search(q, K, R)[1], truth),
                   "binary_recall_at_10": recall(by.search(q, K, R)[1], truth)}
            shard["shared_component"]["arms"].append(arm)
            print(json.dumps(arm), flush=True)
        report["shards"].append(shard)
        Path(args.out).write_text(json.dumps(report, indent=2) + "\n")      # (kept after every shard)
        del X, Y, exact16, ey, py, by
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
