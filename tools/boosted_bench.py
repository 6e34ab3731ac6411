#!/usr/bin/env python
"""Times the boosted exact top-k search (ShardIndex.search_boosted) against the all-rows filtered search and the plain search of the same run.

One process, one GPU: `fill_clustered_rows(1 M, 768)`, k = 10, 1 and 64 queries.  Arms, timed in turn in this one run: the boosted
search with a uniform-random prior in [0, 1) at weights 0, 0.05 and 0.5 (no bitmap); `search(allow=all-rows bitmap)`, the yardstick: the
boosted pass A does the same reads plus 4 bytes per row of prior; the plain fp16 `search`.  Per arm: 5 warm-up calls, then the median
of `--calls` single calls, each between two events on the stream, in ms per call; the boosted arms also record `boosted_stats()` of one
call (queries that overflowed to the exhaustive path, candidate groups rescored).  The largest |prior| is measured once, as
`set_boost` would, not in every call.  Writes profiles/boosted_bench.json.  No time is a pass or fail gate.  Run it under a time limit
(e.g. `timeout -k 10 500 python tools/boosted_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows      # noqa: E402
from arxiv_rag_amd.where import pack_bitmap                           # noqa: E402


def timed(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(runs)), "ms_min": float(min(runs)), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "boosted_bench.json"))
    args = ap.parse_args()
    n, d, k = args.rows, args.dim, args.k
    rows = fill_clustered_rows(n, d, 1, args.clusters)
    idx = ShardIndex(rows, prefilter=None)
    prior = torch.from_numpy(np.random.RandomState(0).rand(n).astype(np.float32)).to(rows.device)
    max_abs, bad = idx.prior_info(prior)
    allow = torch.from_numpy(pack_bitmap(np.ones(n, bool)).view(np.int64)).to(rows.device)
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "k": k, "clusters": args.clusters, "max_abs_prior": max_abs,
           "non_finite_priors": bad, "results": []}
    for nq in (1, 64):
        q = rows[torch.from_numpy(np.random.RandomState(nq).randint(0, n, nq)).to(rows.device)].contiguous()
        res = {"queries": nq, "arms": {}}
        for wt in (0.0, 0.05, 0.5):
            arm = timed(lambda: idx.search_boosted(q, k, prior, wt, max_abs_prior=max_abs), args.calls)
            idx.search_boosted(q, k, prior, wt, max_abs_prior=max_abs)
            arm["overflowed_queries"], arm["candidate_groups"] = idx.boosted_stats()
            res["arms"][f"boosted weight={wt}"] = arm
        res["arms"]["filtered, all rows"] = timed(lambda: idx.search(q, k, allow=allow), args.calls)
        res["arms"]["plain search"] = timed(lambda: idx.search(q, k), args.calls)
        ref = res["arms"]["filtered, all rows"]["ms_median"]
        res["boosted_over_filtered"] = {name: arm["ms_median"] / ref for name, arm in res["arms"].items() if name.startswith("boosted")}
        out["results"].append(res)
        print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
