#!/usr/bin/env python
"""Times the score-threshold search (ShardIndex.search_range: up to 1 024 exact rows per query at or above a cosine) against the plain
search at k = 32 of the same rows.

One process, one GPU: 1 M x 768 unit rows (`fill_unit_rows`), batches of 1 and 64 queries, M = 32, 50, 256 and 1024, and two thresholds
per M: -inf (the list is the exact top M), and the score of each query's own M/2-th row (the list is complete and half full).  Per arm
the range call and `search` at k = 32 (fp16 rows, no int8 pre-filter: pass A is then the same work on both sides, and the difference is
what the long tail costs) are timed in turn, call by call (5 warm-up rounds, then `--calls` rounds, each call between two events), so
both see the same clocks; the median and the minimum over the calls, in ms per batch, and the range search's counters (candidate groups
rescored, queries that overflowed to the exhaustive path) go to profiles/range_bench.json.  Before timing, the scan's answer is compared
bit for bit with the exhaustive path's.  Run it under a time limit (e.g. `timeout -k 10 500 python tools/range_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.index import ShardIndex, fill_unit_rows      # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "range_bench.json"))
    args = ap.parse_args()
    n, d = args.rows, args.dim
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "calls": args.calls, "unit": "ms per batch of all queries",
           "results": []}
    C_ = fill_unit_rows(n, d, 1)
    idx = ShardIndex(C_, prefilter=None)
    for nq in (1, 64):
        Q_ = fill_unit_rows(nq, d, 2, row_base=n)
        for M in (32, 50, 256, 1024):
            top = idx.search_range(Q_, float("-inf"), M)
            for kind, ms in (("-inf", torch.full((nq,), float("-inf"), device="cuda")), ("own M/2-th score", top[0][:, M // 2 - 1].contiguous())):
                def ranged():
                    return idx.search_range(Q_, ms, M)
                a, b = ranged(), idx.search_range(Q_, ms, M, path=2)      # the same answers, bit for bit, before any timing
                assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (nq, M, kind)
                ranged()
                over, groups = idx.range_stats()
                for _ in range(5):
                    ranged(); idx.search(Q_, 32)
                torch.cuda.synchronize()
                t_r, t_32 = [], []
                for _ in range(args.calls):
                    t_r.append(event_ms(ranged))
                    t_32.append(event_ms(lambda: idx.search(Q_, 32)))
                row = {"queries": nq, "max_results": M, "min_score": kind, "rows_returned_mean": float((a[1] >= 0).sum(dim=1).float().mean()),
                       "truncated_queries": int((a[2] > M).sum()), "range_ms_median": float(np.median(t_r)), "range_ms_min": float(min(t_r)),
                       "search_k32_ms_median": float(np.median(t_32)), "search_k32_ms_min": float(min(t_32)),
                       "overflowed_queries": over, "candidate_groups": groups}
                out["results"].append(row)
                print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
