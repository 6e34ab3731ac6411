#!/usr/bin/env python
"""Times the filtered exact top-k search (ShardIndex.search(allow=...)) against the unfiltered fp16 search of the same run.

One process, one GPU: `fill_unit_rows(1 M, 768)`, 64 and 1 queries, k = 10.  Arms: the unfiltered `ShardIndex(prefilter=None).search`
(the yardstick: existing code) and the filtered search with masks that allow all rows, a random 50 % / 10 % / 1 % / 0.1 %, a contiguous
12.5 % and one row per 64-row group, each on the library's path (n_allowed given), the masked scan (path 1) and the exhaustive path
(path 2).  Per arm: 5 warm-up calls, then `--repeats` timed runs of `--iters` back-to-back calls between two events on the stream;
the median and the minimum of the runs, in ms per batch, go to profiles/filter_bench.json with the path the library chose and the
counters of `filtered_stats`.  Run it under a time limit (e.g. `timeout -k 10 500 python tools/filter_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.index import ShardIndex, fill_unit_rows      # noqa: E402
from arxiv_rag_amd.where import pack_bitmap                     # noqa: E402

def exhaustive_max_pairs(nq):         # csrc/filter.hip FILT_EXHAUSTIVE_MAX_PAIRS*: what path 0 compares n_allowed * n_queries with
    return (1 << 20) if nq >= 64 else (1 << 18)


def timed(fn, iters, repeats):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) / iters)
    return {"ms_median": float(np.median(runs)), "ms_min": float(min(runs)), "runs": len(runs), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "filter_bench.json"))
    args = ap.parse_args()
    n, d, k = args.rows, args.dim, args.k
    C_ = fill_unit_rows(n, d, 1)
    idx = ShardIndex(C_, prefilter=None)
    rs = np.random.RandomState(0)
    u = rs.rand(n)
    masks = {"all": np.ones(n, bool), "random 50%": u < 0.5, "random 10%": u < 0.1, "random 1%": u < 0.01, "random 0.1%": u < 0.001,
             "contiguous 12.5%": (np.arange(n) >= n // 3) & (np.arange(n) < n // 3 + n // 8), "one row per group": np.arange(n) % 64 == 17}
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "k": k, "exhaustive_max_pairs": {"queries >= 64": 1 << 20, "queries < 64": 1 << 18}, "results": []}
    for nq in (64, 1):
        Q_ = fill_unit_rows(nq, d, 2)
        base = timed(lambda: idx.search(Q_, k), args.iters, args.repeats)
        out["results"].append({"queries": nq, "arm": "unfiltered fp16 search", **base})
        print(json.dumps(out["results"][-1]), flush=True)
        for name, m in masks.items():
            allow = torch.from_numpy(pack_bitmap(m).view(np.int64)).cuda()
            n_allowed = int(m.sum())
            for arm, kw in (("library", dict(n_allowed=n_allowed)), ("masked scan", dict(path=1)), ("exhaustive", dict(path=2))):
                if arm == "exhaustive" and n_allowed * nq > (1 << 26):
                    continue                                     # (tens of milliseconds per batch: not a candidate, and GPU time is shared)
                t = timed(lambda: idx.search(Q_, k, allow=allow, **kw), args.iters, args.repeats)
                over, groups = idx.filtered_stats()
                chosen = arm if arm != "library" else ("exhaustive" if n_allowed * nq < exhaustive_max_pairs(nq) else "masked scan")
                out["results"].append({"queries": nq, "mask": name, "allowed_rows": n_allowed, "arm": arm, "path_run": chosen,
                                       "overflowed_queries": over, "candidate_groups": groups,
                                       "ratio_to_unfiltered": t["ms_median"] / base["ms_median"], **t})
                print(json.dumps(out["results"][-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
