#!/usr/bin/env python
"""Times the near-duplicate self-join (`ShardIndex.nearest_earlier` over all rows, k = 1) on one GPU, beside the only route the code
had to a nearest neighbour of every row before it: `ShardIndex.search` of all rows as queries at k = 2 in 1 024-query batches on the
fp16 pass (the full square, not earlier-only: a row's best match is itself, the second its nearest neighbour on EITHER side).

One process: unit rows at D = 768 from `fill_unit_rows` and `fill_clustered_rows`, N = 200 000 by default (`--rows 1000000` where the
visit allows).  Per corpus: one warm-up slice, then the join timed between two events on the stream, `--repeats` times; the achieved
FLOP/s are counted over the N^2 D lower triangle (N (N - 1) / 2 pairs x 2 D), and the overflow counters of `prefix_stats` are read after
the last run.  The full-square search is timed the same way (its FLOP/s over N^2 pairs).  Results -> profiles/dedup_bench.json.
Run it under a time limit (e.g. `timeout -k 10 500 python tools/dedup_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows, fill_unit_rows      # noqa: E402


def timed(fn, repeats):
    runs = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(runs)), "ms_min": float(min(runs)), "runs": len(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--skip-square", action="store_true", help="time the join only")
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "dedup_bench.json"))
    args = ap.parse_args()
    d = args.dim
    out = {"device": torch.cuda.get_device_name(0), "dim": d, "k": 1, "results": []}
    for n in args.rows:
        for name, make in (("unit", lambda: fill_unit_rows(n, d, 1)), ("clustered", lambda: fill_clustered_rows(n, d, 1, args.clusters))):
            C_ = make()
            idx = ShardIndex(C_, prefilter=None)
            idx.nearest_earlier(0, min(n, 2048), 1)              # warm-up: kernels loaded, workspace allocated
            res = {}

            def join():
                res["s"], res["i"] = idx.nearest_earlier(0, n, 1)
            t = timed(join, args.repeats)
            over, groups = idx.prefix_stats()
            s = res["s"][1:, 0]
            row = {"rows": n, "corpus": name, "arm": "nearest_earlier (self-join, lower triangle)", **t,
                   "tflops_lower_triangle": n * (n - 1) * d / (t["ms_median"] * 1e-3) / 1e12,
                   "overflowed_queries": over, "candidate_groups": groups,
                   "rows_with_an_earlier_row_at_0.95": int((s >= 0.95).sum()), "nearest_score_median": float(s.median())}
            out["results"].append(row)
            print(json.dumps(row), flush=True)
            if args.skip_square:
                continue

            def square():
                for a in range(0, n, 1024):
                    idx.search(C_[a:a + 1024], 2)
            square()
            t2 = timed(square, args.repeats)
            row2 = {"rows": n, "corpus": name, "arm": "search of all rows, k = 2, 1 024-query batches (full square)", **t2,
                    "tflops_full_square": 2.0 * n * n * d / (t2["ms_median"] * 1e-3) / 1e12,
                    "join_time_over_square_time": t["ms_median"] / t2["ms_median"]}
            out["results"].append(row2)
            print(json.dumps(row2), flush=True)
            del idx, C_, res
            torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
