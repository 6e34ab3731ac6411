#!/usr/bin/env python
"""IVF probe search against the exact searches -> profiles/ivf_bench.json (README, "IVF probe search").

Shards of `fill_clustered_rows` (dim 768), an `ivf.IvfIndex` per n_lists; per arm nprobe x Q: the median of 20 calls of
`IvfIndex.search` (probe included), the rows scanned, row bytes per second against the 6.29 TB/s copy rate, recall@10 against
`ShardIndex.search` on the same queries, and, timed in turn in the same process, the exact search (fp16 and with the int8 first pass)
and `search_filtered_many(path=2)` over the same probe bitmaps (Q <= 64).  No time is a pass / fail gate.

    python tools/ivf_bench.py --rows 1000000 10000000 --lists 1024 4096
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows      # noqa: E402
from arxiv_rag_amd.ivf import IvfIndex                               # noqa: E402

DIM, K, COPY_RATE = 768, 10, 6.29e12
BIT = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64)


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


def probe_bitmaps(labels, probes, n_rows):
    """int64 device [nq, ceil(n_rows / 64)]: the rows of every query's probed lists, packed on the device."""
    words = (n_rows + 63) // 64
    out = torch.empty((probes.shape[0], words), dtype=torch.int64, device=labels.device)
    bit = BIT.to(labels.device)
    for q in range(probes.shape[0]):
        m = torch.zeros(words * 64, dtype=torch.int64, device=labels.device)
        m[:n_rows] = torch.isin(labels, probes[q]).to(torch.int64)
        out[q] = (m.reshape(words, 64) * bit).sum(1)
    return out


def recall(ids, exact):
    hit = (ids[:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)
    return float(hit.any(1).float().sum() / (exact >= 0).sum().clamp(min=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default="profiles/ivf_bench.json")
    args = ap.parse_args()
    dev = "cuda:0"
    out_path = Path(args.out)
    results = json.loads(out_path.read_text()) if out_path.exists() else {"dim": DIM, "k": K, "copy_rate_bytes_per_s": COPY_RATE, "shards": {}}
    for n in args.rows:
        X = fill_clustered_rows(n, DIM, seed=11, n_clusters=max(64, n // 500), device=dev)
        Qall = fill_clustered_rows(max(args.queries), DIM, seed=11, n_clusters=max(64, n // 500), device=dev, row_base=1 << 40)
        fp16, i8 = ShardIndex(X, prefilter=None), ShardIndex(X, prefilter="int8")
        shard = results["shards"].setdefault(str(n), {"exact": {}, "lists": {}})
        exact_ids = {}
        for nq in args.queries:
            Q = Qall[:nq].contiguous()
            exact_ids[nq] = fp16.search(Q, K)[1]
            shard["exact"][str(nq)] = {"fp16_ms": median_ms(lambda: fp16.search(Q, K)), "int8_ms": median_ms(lambda: i8.search(Q, K))}
            print(n, "exact", nq, shard["exact"][str(nq)], flush=True)
        for n_lists in args.lists:
            ivf = IvfIndex.build(fp16, n_lists, iters=10, seed=0)
            entry = shard["lists"].setdefault(str(n_lists), {})
            entry["build"] = ivf.summary()
            print(n, n_lists, entry["build"], flush=True)
            arms = entry["arms"] = []
            for nprobe in args.nprobe:
                for nq in args.queries:
                    Q = Qall[:nq].contiguous()
                    s, i, scanned = ivf.search(Q, K, nprobe)
                    rows = float(scanned.float().mean())
                    ms = median_ms(lambda: ivf.search(Q, K, nprobe))
                    probes = ivf.probe(Q, nprobe)
                    maps = probe_bitmaps(ivf.labels, probes, n)
                    fo = torch.arange(nq, dtype=torch.int32, device=dev)
                    fs, fi = fp16.search_filtered_many(Q, maps, fo, K, path=2)
                    assert torch.equal(fi, i) and torch.equal(fs.view(torch.int32), s.view(torch.int32)), "IVF and the filtered search disagree"
                    arm = {"nprobe": nprobe, "queries": nq, "ivf_ms": ms, "rows_scanned_per_query": rows, "fraction_of_shard": rows / n,
                           "row_bytes_per_s": rows * nq * DIM * 2 / (ms * 1e-3), "recall_at_10": recall(i, exact_ids[nq]),
                           "filtered_many_path2_ms": median_ms(lambda: fp16.search_filtered_many(Q, maps, fo, K, path=2)),
                           "exact_fp16_ms": shard["exact"][str(nq)]["fp16_ms"], "exact_int8_ms": shard["exact"][str(nq)]["int8_ms"]}
                    arm["fraction_of_copy_rate"] = arm["row_bytes_per_s"] / COPY_RATE
                    arms.append(arm)
                    print(arm, flush=True)
                    del maps
            del ivf
            out_path.parent.mkdir(parents=True, exist_ok=True)
            out_path.write_text(json.dumps(results, indent=1))
        del X, fp16, i8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
