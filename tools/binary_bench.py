#!/usr/bin/env python
"""Binary-code search against the exact searches -> profiles/binary_bench.json (README, "binary-code search").

Shards of `fill_clustered_rows` (dim 768) with a `binary.BinaryIndex` (centre = the column mean); per arm Q x R: the median of 20
calls of `BinaryIndex.search` (query pack and exact rescore included), the event span of the `arx_binary_candidates` call alone beside
its floor (the code array's bytes at the 6.29 TB/s copy rate, once per call), recall@10 against `ShardIndex.search` on the same
queries, and, timed in turn in the same process, the exact search on the fp16 rows and with the int8 first pass.  The same recall on
rows with a strong shared component (every row plus a constant vector, renormalised), with centre = mean and with none.  `loses`
names the arms where the binary search is not faster than the better exact search.  No time is a pass / fail gate.

    python tools/binary_bench.py --rows 1000000 10000000
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from arxiv_rag_amd.binary import BinaryIndex, candidates_device      # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows      # noqa: E402

DIM, K, COPY_RATE = 768, 10, 6.29e12


def median_ms(fn, calls=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def event_ms(fn, calls=20, warmup=3):
    for _ in range(warmup):
        fn()
    spans = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        spans.append(a.elapsed_time(b))
    return statistics.median(spans)


def recall(ids, exact):
    hit = (ids[:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)
    return float(hit.any(1).float().sum() / (exact >= 0).sum().clamp(min=1))


def shifted(X, shift=1.5):
    """Rows with a strong shared component: every row plus a constant vector, renormalised, in slices."""
    out = torch.empty_like(X)
    for a in range(0, X.shape[0], 1 << 20):
        y = X[a:a + (1 << 20)].float() + shift / DIM ** 0.5 * 4.0
        out[a:a + (1 << 20)] = (y / y.norm(dim=1, keepdim=True)).half()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--candidates", type=int, nargs="+", default=[40, 128, 256])
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "binary_bench.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    report = {"dim": DIM, "k": K, "copy_rate_bytes_per_s": COPY_RATE, "shards": []}
    for n in args.rows:
        X = fill_clustered_rows(n, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev)
        exact16, exact8 = ShardIndex(X, prefilter=None), ShardIndex(X, prefilter="int8")
        t0 = time.perf_counter()
        bi = BinaryIndex.build(exact16, centre="mean")
        torch.cuda.synchronize()
        shard = {"rows": n, "build_seconds": time.perf_counter() - t0, "code_bytes": int(bi.codes.numel() * 8),
                 "scan_floor_ms": bi.codes.numel() * 8 / COPY_RATE * 1e3, "arms": [], "loses": []}
        for nq in args.queries:
            q = fill_clustered_rows(nq, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=n + 12345)
            fp16_ms = median_ms(lambda: exact16.search(q, K))
            int8_ms = median_ms(lambda: exact8.search(q, K))
            truth = exact16.search(q, K)[1]
            qcodes = bi.pack(q)
            for R in args.candidates:
                ms = median_ms(lambda: bi.search(q, K, R))
                scan_ms = event_ms(lambda: candidates_device(bi.codes, qcodes, R, ws=bi._workspace(nq, R), want_dist=False))
                arm = {"queries": nq, "candidates": R, "binary_ms": ms, "scan_event_ms": scan_ms, "exact_fp16_ms": fp16_ms, "exact_int8_ms": int8_ms,
                       "recall_at_10": recall(bi.search(q, K, R)[1], truth)}
                shard["arms"].append(arm)
                if ms >= min(fp16_ms, int8_ms):
                    shard["loses"].append({"queries": nq, "candidates": R})
        # rows with a strong shared component: the centre decides what the bits can tell apart
        Y = shifted(X)
        del exact8
        ey = ShardIndex(Y, prefilter=None)
        q = shifted(fill_clustered_rows(64, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=n + 12345))
        truth = ey.search(q, K)[1]
        shard["shared_component"] = {"mean_pairwise_cosine": float((Y[:4096].float() @ Y[4096:8192].float().T).mean()), "arms": []}
        for centre in ("mean", None):
            by = BinaryIndex.build(ey, centre=centre)
            for R in args.candidates:
                shard["shared_component"]["arms"].append({"centre": centre or "none", "candidates": R, "recall_at_10": recall(by.search(q, K, R)[1], truth)})
            del by
        report["shards"].append(shard)
        del X, Y, exact16, ey, bi
        torch.cuda.empty_cache()
    Path(args.out).write_text(json.dumps(report, indent=2) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
