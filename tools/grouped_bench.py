#!/usr/bin/env python
"""Times the grouped search (ShardIndex.search_grouped: the exact top papers with their best chunks) against the plain search of the
same rows.

One process, one GPU: 1 M x 768 unit rows in topic order (`fill_clustered_rows` with a negative `n_clusters`: every run of rows shares
a centre, as a paper's chunks do), papers = runs of 64 rows, and a second arm with runs of 200 rows; P = 10 papers, m = 3 chunks each; 1
and 64 queries (rows of the shard at scattered positions, perturbed).  Per arm the grouped call, `search` at k = 10 and `search` at
k = 32 (what a caller who collapses on the host over-fetches: the search's k limit) are timed in turn, call by call (5 warm-up rounds,
then `--calls` rounds, each call between two events), so all three see the same clocks; the median and the minimum over the calls, in
ms per batch, and the grouped search's counters go to profiles/grouped_bench.json.  Before timing, the grouped answer of the scan is
compared bit for bit with the exhaustive path's.  Run it under a time limit (e.g. `timeout -k 10 500 python tools/grouped_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.grouping import select_count                       # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows      # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--papers", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "grouped_bench.json"))
    args = ap.parse_args()
    n, d, P, m = args.rows, args.dim, args.papers, args.chunks
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "papers": P, "chunks_per_paper": m, "calls": args.calls,
           "unit": "ms per batch of all queries", "results": []}
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    for run in (64, 200):
        C_ = fill_clustered_rows(n, d, 1, -run)
        idx = ShardIndex(C_, prefilter=None).set_groups(torch.arange(n, device="cuda", dtype=torch.int32) // run)
        for nq in (1, 64):
            pos = torch.randint(n, (nq,), generator=g, device="cuda")
            Q_ = torch.nn.functional.normalize(C_[pos].float() + 0.02 * torch.randn((nq, d), generator=g, device="cuda"), dim=1).half().contiguous()

            def grouped():
                return idx.search_grouped(Q_, P, m)
            a, b = grouped(), idx.search_grouped(Q_, P, m, path=2)       # the same answers, bit for bit, before any timing
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (run, nq)
            grouped()
            over, groups = idx.grouped_stats()
            s10, i10 = idx.search(Q_, 10)
            s32, i32 = idx.search(Q_, 32)
            papers10 = float(np.mean([len(set((r // run).tolist())) for r in i10.cpu().numpy()]))
            papers32 = float(np.mean([len(set((r // run).tolist())) for r in i32.cpu().numpy()]))
            for _ in range(5):
                grouped(); idx.search(Q_, 10); idx.search(Q_, 32)
            torch.cuda.synchronize()
            t_g, t_10, t_32 = [], [], []
            for _ in range(args.calls):
                t_g.append(event_ms(grouped))
                t_10.append(event_ms(lambda: idx.search(Q_, 10)))
                t_32.append(event_ms(lambda: idx.search(Q_, 32)))
            row = {"run_rows": run, "queries": nq, "selected_group_maxima_K": select_count(P, idx.max_run_rows),
                   "grouped_ms_median": float(np.median(t_g)), "grouped_ms_min": float(min(t_g)),
                   "search_k10_ms_median": float(np.median(t_10)), "search_k10_ms_min": float(min(t_10)),
                   "search_k32_ms_median": float(np.median(t_32)), "search_k32_ms_min": float(min(t_32)),
                   "overflowed_queries": over, "candidate_groups": groups,
                   "distinct_papers_in_plain_top10": papers10, "distinct_papers_in_plain_top32": papers32}
            out["results"].append(row)
            print(json.dumps(row), flush=True)
        del idx, C_
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
