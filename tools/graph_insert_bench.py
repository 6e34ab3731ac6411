#!/usr/bin/env python
"""Inserting rows into a built graph against rebuilding it -> profiles/graph_insert_bench.json (README, "graph search").

Workload: the graph benchmark's clustered rows (`fill_clustered_rows`, dim 768), degree 32.  The graph over all rows is built once, timed
(`GraphIndex.build`, the exact self-join).  Per arm the last m rows (1 000, 10 000, 100 000) are inserted into a graph built over the
rest (`GraphIndex.insert`), timed in turn in the same process.  Recorded per arm: the insert's seconds against the rebuild's; recall@10
against the exact search at ef 64 and 128, of the maintained and of the rebuilt graph, for 64 fresh queries and for 64 queries that are
inserted rows themselves; for the latter also the recall over the (query, true neighbour) pairs whose neighbour is an inserted row;
offers and orphans.  `loses` names the arms where the insert is not faster than the rebuild or the maintained graph recalls less than
the rebuilt one.  `quality_test` repeats the measurement of tests/test_gpu_graph_insert.py's last test.  Nothing is a pass / fail gate.

    python tools/graph_insert_bench.py --rows 1000000 --insert 1000 10000 100000
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binary_bench import DIM, K, recall                                                # noqa: E402
from arxiv_rag_amd.graph import GraphIndex                                             # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows                        # noqa: E402

DEGREE, EFS, NQ = 32, (64, 128), 64


def pair_recall(ids, truth, lo):
    """the share of the (query, true neighbour >= lo) pairs whose neighbour is among `ids`; the number of such pairs"""
    want = truth >= lo
    hit = (ids[:, :, None] == truth[:, None, :]).any(1) & want
    return (float(hit.sum() / want.sum().clamp(min=1)), int(want.sum()))


def quality_test(dev):
    n, lo, dim = 4096, 3072, 128
    X = fill_clustered_rows(n, dim, 11, 16, device=dev)
    q = fill_clustered_rows(NQ, dim, 11, 16, device=dev, row_base=n + 12345)
    idx = ShardIndex(X)
    truth = idx.search(q, K)[1]
    rebuilt = [recall(GraphIndex.build(idx, degree=DEGREE, iters=3, seed=seed).search(q, K, 64)[1], truth) for seed in range(5)]
    g = GraphIndex.build(ShardIndex(X[:lo].contiguous()), degree=DEGREE, iters=3, seed=0)
    g.index = idx
    info = g.insert(lo, n, insert_ef=64)
    return {"rows": n, "inserted": n - lo, "dim": dim, "ef": 64, "queries": NQ, "rebuilt_recall_at_10_by_entry_seed": rebuilt,
            "margin": 2 * (max(rebuilt) - min(rebuilt)), "maintained_recall_at_10": recall(g.search(q, K, 64)[1], truth), "orphans": info["orphans"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--insert", type=int, nargs="+", default=[1000, 10_000, 100_000])
    ap.add_argument("--insert-ef", type=int, default=64)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "graph_insert_bench.json"))
    args = ap.parse_args()
    dev, n = "cuda:0", args.rows
    report = {"dim": DIM, "k": K, "degree": DEGREE, "rows": n, "insert_ef": args.insert_ef, "quality_test": quality_test(dev), "arms": [], "loses": []}
    print(json.dumps(report["quality_test"]), flush=True)
    X = fill_clustered_rows(n, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev)
    exact = ShardIndex(X, prefilter=None)
    rebuilt = GraphIndex.build(exact, degree=DEGREE)
    report["rebuild_seconds"] = rebuilt.info["seconds"]
    q_fresh = fill_clustered_rows(NQ, DIM, seed=1, n_clusters=max(n // 2000, 8), device=dev, row_base=n + 12345)
    for m in args.insert:
        lo = n - m
        base = GraphIndex.build(ShardIndex(X[:lo], prefilter=None), degree=DEGREE)
        base.index = exact
        info = base.insert(lo, n, insert_ef=args.insert_ef)
        q_new = X[lo + torch.arange(NQ, device=dev) * (m // NQ)].contiguous()
        arm = {"inserted": m, "base_build_seconds": base.info["seconds"], "insert_seconds": info["seconds"],
               "rebuild_over_insert": rebuilt.info["seconds"] / info["seconds"], "offers": info["offers"], "orphans": info["orphans"]}
        for name, q in (("fresh", q_fresh), ("inserted_rows", q_new)):
            truth = exact.search(q, K)[1]
            for ef in EFS:
                for kind, g in (("maintained", base), ("rebuilt", rebuilt)):
                    ids = g.search(q, K, ef)[1]
                    arm[f"{name}_ef{ef}_{kind}_recall_at_10"] = recall(ids, truth)
                    if name == "inserted_rows":
                        arm[f"{name}_ef{ef}_{kind}_recall_of_inserted_neighbours"], arm["inserted_neighbour_pairs"] = pair_recall(ids, truth, lo)
        report["arms"].append(arm)
        print(json.dumps(arm), flush=True)
        worse = [key for key in arm if "_maintained_" in key and arm[key] < arm[key.replace("_maintained_", "_rebuilt_")]]
        if arm["insert_seconds"] >= rebuilt.info["seconds"] or worse:
            report["loses"].append({"inserted": m, "slower_than_rebuild": arm["insert_seconds"] >= rebuilt.info["seconds"], "recalls_less": worse})
        Path(args.out).write_text(json.dumps(report, indent=2) + "\n")      # (kept after every arm)
        del base
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
