#!/usr/bin/env python
"""Graph search against the exact and the IVF probe searches -> profiles/graph_bench.json (README, "graph search").

Shards: the IVF benchmark's clustered rows (`fill_clustered_rows`, dim 768) and unclustered unit rows (`fill_unit_rows`), where IVF
has no cluster structure to lean on.  Per shard a `graph.GraphIndex` of degree 32 is built twice, timed: from the exact self-join
(skipped above `--exact-build-max-rows`: it is n^2 work) and through an `IvfIndex` of 4096 lists at `--build-nprobe` probes; the arms
run on the exact graph where there is one.  Per arm Q x ef, all in one process and timed in turn, median of 20 calls:
`GraphIndex.search` (its entry step, a centroid search, included), the exact search on the fp16 rows and with the int8 first pass, and
`IvfIndex.search` at nprobe 4 and 16; recall@10 of each approximate search against the exact search of the same run, and the rows
scored and iterations run per query (means).  `loses` names the arms where the graph search is not faster than the better exact
search, `slower_than_ivf` those where an IVF arm of at least its recall is faster.  No time or recall is a pass / fail gate.

    python tools/graph_bench.py --rows 1000000 10000000 --unit-rows 1000000
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binary_bench import DIM, K, median_ms, recall                                     # noqa: E402
from arxiv_rag_amd.graph import GraphIndex                                             # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows, fill_unit_rows        # noqa: E402
from arxiv_rag_amd.ivf import IvfIndex                                                 # noqa: E402

DEGREE, IVF_LISTS, IVF_PROBES = 32, 4096, (4, 16)


def rows_of(kind, n, dev, row_base=0):
    if kind == "clustered":
        return fill_clustered_rows(n, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=row_base)
    return fill_unit_rows(n, DIM, seed=1, device=dev, row_base=row_base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000], help="clustered shards")
    ap.add_argument("--unit-rows", type=int, nargs="*", default=[1_000_000], help="unclustered unit-row shards")
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--ef", type=int, nargs="+", default=[32, 64, 128, 256])
    ap.add_argument("--entries", type=int, default=8)
    ap.add_argument("--build-nprobe", type=int, default=16)
    ap.add_argument("--exact-build-max-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "graph_bench.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    report = {"dim": DIM, "k": K, "degree": DEGREE, "entries": args.entries, "ivf_lists": IVF_LISTS, "build_nprobe": args.build_nprobe, "shards": []}
    for kind, n in [("clustered", n) for n in args.rows] + [("unit", n) for n in args.unit_rows]:
        X = rows_of(kind, n, dev)
        exact16, exact8 = ShardIndex(X, prefilter=None), ShardIndex(X, prefilter="int8")
        ivf = IvfIndex.build(exact16, min(IVF_LISTS, n))
        via_ivf = GraphIndex.build(exact16, degree=DEGREE, ivf=ivf, nprobe=min(args.build_nprobe, ivf.n_lists))
        shard = {"kind": kind, "rows": n, "ivf_build_seconds": ivf.info["seconds"], "graph_build_seconds_through_ivf": via_ivf.info["seconds"],
                 "graph_build_seconds_exact": None, "arms": [], "loses": [], "slower_than_ivf": []}
        g = via_ivf
        if n <= args.exact_build_max_rows:
            g = GraphIndex.build(exact16, degree=DEGREE)
            shard["graph_build_seconds_exact"] = g.info["seconds"]
            shard["edges_shared_with_ivf_build"] = float((g.neighbors == via_ivf.neighbors).float().mean())
        shard["graph"] = {k: v for k, v in g.summary().items() if k != "seconds"}
        print(json.dumps({k: v for k, v in shard.items() if not isinstance(v, list)}), flush=True)
        for nq in args.queries:
            q = rows_of(kind, nq, dev, row_base=n + 12345)
            fp16_ms = median_ms(lambda: exact16.search(q, K))
            int8_ms = median_ms(lambda: exact8.search(q, K))
            truth = exact16.search(q, K)[1]
            ivf_arms = {p: {"ms": median_ms(lambda: ivf.search(q, K, p)), "recall_at_10": recall(ivf.search(q, K, p)[1], truth)}
                        for p in IVF_PROBES if p <= ivf.n_lists}
            for ef in args.ef:
                ms = median_ms(lambda: g.search(q, K, ef, n_entries=args.entries))
                ids, scored, expanded = g.search(q, K, ef, n_entries=args.entries, counters=True)[1:]
                arm = {"queries": nq, "ef": ef, "graph_ms": ms, "recall_at_10": recall(ids, truth), "rows_scored": float(scored.float().mean()),
                       "iterations": float(expanded.float().mean()), "exact_fp16_ms": fp16_ms, "exact_int8_ms": int8_ms,
                       **{f"ivf_nprobe{p}_ms": a["ms"] for p, a in ivf_arms.items()},
                       **{f"ivf_nprobe{p}_recall_at_10": a["recall_at_10"] for p, a in ivf_arms.items()}}
                shard["arms"].append(arm)
                print(json.dumps(arm), flush=True)
                if ms >= min(fp16_ms, int8_ms):
                    shard["loses"].append({"queries": nq, "ef": ef})
                if any(a["ms"] <= ms and a["recall_at_10"] >= arm["recall_at_10"] for a in ivf_arms.values()):
                    shard["slower_than_ivf"].append({"queries": nq, "ef": ef})
        report["shards"].append(shard)
        Path(args.out).write_text(json.dumps(report, indent=2) + "\n")      # (kept after every shard)
        del X, exact16, exact8, ivf, via_ivf, g
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
