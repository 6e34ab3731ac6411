#!/usr/bin/env python
"""IVF probe search with a filter and a threshold per query -> profiles/ivf_multi_bench.json (README, "IVF probe search").

One shard of `fill_clustered_rows` (dim 768), one `ivf.IvfIndex` (4096 lists), k = 10; all arms run in turn in one process, every time
the median of 20 calls (host clock around a call that ends in a device synchronise; probe included), with the spread of the 20 kept.
  filters     Q = 1 / 8 / 64 queries with as many distinct random-10 % filters: `IvfIndex.search_many` (one call) against one
              `IvfIndex.search(allow=)` call per distinct filter and against `ShardIndex.search_filtered_many` over the full shard.
  min_score   `search_many` with every query's own 5th-best score as its threshold against the same call without a threshold.
  single      one filter, no threshold: `search_many` against `IvfIndex.search(allow=)` (`arx_ivf_search`, the entry point that was
              there before), the calls of the two alternating, and the ratio of the medians next to the spread of either.
No time is a pass / fail gate.

    python tools/ivf_multi_bench.py --rows 10000000
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

DIM, K, CALLS = 768, 10, 20
BIT = torch.tensor([1 << i for i in range(63)] + [-(1 << 63)], dtype=torch.int64)


def timed(fns, calls=CALLS, warmup=3):
    """[{median_ms, min_ms, max_ms, p10_ms, p90_ms}] per function: `calls` timed calls each, the functions taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(calls):
        for fn, ts in zip(fns, times):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    out = []
    for ts in times:
        ts = sorted(ts)
        out.append({"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1], "p10_ms": ts[len(ts) // 10], "p90_ms": ts[-1 - len(ts) // 10]})
    return out


def random_filters(n_filters, n_rows, share, device, seed):
    """int64 device [n_filters, ceil(n_rows / 64)]: bitmaps that allow a random `share` of the rows."""
    words = (n_rows + 63) // 64
    gen = torch.Generator(device=device).manual_seed(seed)
    bit = BIT.to(device)
    out = torch.empty((n_filters, words), dtype=torch.int64, device=device)
    for f in range(n_filters):
        m = (torch.rand(words * 64, generator=gen, device=device) < share).to(torch.int64)
        m[n_rows:] = 0
        out[f] = (m.reshape(words, 64) * bit).sum(1)
    return out


def same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default="profiles/ivf_multi_bench.json")
    args = ap.parse_args()
    assert max(args.queries) <= 64, "search_filtered_many takes at most 64 filters per call"
    dev, n, nprobe = "cuda:0", args.rows, args.nprobe
    X = fill_clustered_rows(n, DIM, seed=11, n_clusters=max(64, n // 500), device=dev)
    Qall = fill_clustered_rows(max(args.queries), DIM, seed=11, n_clusters=max(64, n // 500), device=dev, row_base=1 << 40)
    fp16 = ShardIndex(X, prefilter=None)
    ivf = IvfIndex.build(fp16, args.lists, iters=10, seed=0)
    allows = random_filters(max(args.queries), n, 0.1, dev, seed=5)
    res = {"dim": DIM, "k": K, "rows": n, "nprobe": nprobe, "calls": CALLS, "build": ivf.summary(), "filters": [], "min_score": [], "single": []}
    print(res["build"], flush=True)
    for nq in args.queries:
        Q = Qall[:nq].contiguous()
        A = allows[:nq].contiguous()
        fo = torch.arange(nq, dtype=torch.int32, device=dev)
        singles = [Qall[q:q + 1].contiguous() for q in range(nq)]

        def per_filter():
            return [ivf.search(singles[q], K, nprobe, allow=A[q]) for q in range(nq)]

        many = ivf.search_many(Q, K, nprobe, allows=A, filter_of=fo)
        each = per_filter()
        assert all(same([t[q:q + 1] for t in many[:3]], each[q]) for q in range(nq)), "search_many and the per-filter calls disagree"
        t_many, t_each = timed([lambda: ivf.search_many(Q, K, nprobe, allows=A, filter_of=fo), per_filter])      # the two IVF routes take turns
        t_full, = timed([lambda: fp16.search_filtered_many(Q, A, fo, K)])       # on its own: a pass over the whole shard leaves other cache contents
        arm = {"queries": nq, "distinct_filters": nq, "rows_scanned_per_query": float(many[2].float().mean()), "search_many": t_many,
               "search_per_filter": t_each, "filtered_many_full_shard": t_full,
               "per_filter_over_many": t_each["median_ms"] / t_many["median_ms"], "full_shard_over_many": t_full["median_ms"] / t_many["median_ms"]}
        res["filters"].append(arm)
        print(arm, flush=True)

        thr = many[0][:, 4].contiguous()                        # every query's own 5th-best score (-inf where it has fewer rows)
        hit = ivf.search_many(Q, K, nprobe, allows=A, filter_of=fo, min_score=thr)
        assert same([t[:, :5] for t in hit[:2]], [t[:, :5] for t in many[:2]]) and torch.equal(hit[2], many[2])
        t_thr, t_plain = timed([lambda: ivf.search_many(Q, K, nprobe, allows=A, filter_of=fo, min_score=thr),
                                lambda: ivf.search_many(Q, K, nprobe, allows=A, filter_of=fo)])
        arm = {"queries": nq, "hits_per_query": float(hit[3].float().mean()), "with_min_score": t_thr, "without": t_plain,
               "with_over_without": t_thr["median_ms"] / t_plain["median_ms"]}
        res["min_score"].append(arm)
        print(arm, flush=True)

        one, zero = allows[:1].contiguous(), torch.zeros(nq, dtype=torch.int32, device=dev)
        assert same(ivf.search_many(Q, K, nprobe, allows=one, filter_of=zero)[:3], ivf.search(Q, K, nprobe, allow=one[0]))
        t_new, t_old = timed([lambda: ivf.search_many(Q, K, nprobe, allows=one, filter_of=zero), lambda: ivf.search(Q, K, nprobe, allow=one[0])])
        ratio = t_new["median_ms"] / t_old["median_ms"]
        spread = max(t_old["p90_ms"] / t_old["median_ms"], t_new["p90_ms"] / t_new["median_ms"])
        arm = {"queries": nq, "search_many": t_new, "search": t_old, "many_over_search": ratio, "p90_over_median": spread,
               "inside_the_spread": bool(ratio <= spread)}
        res["single"].append(arm)
        print(arm, flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
