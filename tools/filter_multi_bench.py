#!/usr/bin/env python
"""Times the search with a different filter per query in one call (ShardIndex.search_filtered_many) against the same queries answered by
one ShardIndex.search(allow=...) call per distinct filter (the existing single-filter search: the baseline).

One process, one GPU: `fill_unit_rows(1 M, 768)`, 64 queries, k = 10.  Arms: 1, 8 and 64 distinct filters, each with random 1 %, random
50 % and contiguous 12.5 % masks (a different random draw / a different offset per filter); query q uses filter q % F.  Per arm the two
ways are timed in turn, call by call (5 warm-up rounds, then `--calls` rounds: one multi call between two events, then the per-filter
loop between two events), so both see the same clocks; the median and the minimum over the calls, in ms per 64-query batch, go to
profiles/filter_multi_bench.json.  The one-filter arm is the price of the per-query machinery: there the loop IS the single-filter call of
all 64 queries.  `n_allowed` is not passed, so both ways take the masked scan.  Before timing, the two ways' answers are compared bit for
bit.  Run it under a time limit (e.g. `timeout -k 10 500 python tools/filter_multi_bench.py`)."""
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


def masks_of(kind, F, n, rs):
    if kind == "random 1%":
        return [rs.rand(n) < 0.01 for _ in range(F)]
    if kind == "random 50%":
        return [rs.rand(n) < 0.5 for _ in range(F)]
    out = []                                                     # contiguous 12.5 %, offsets spread over the shard, not aligned to 64
    for f in range(F):
        a = (n // 3 + f * (n - n // 8) // max(F, 1) + 37 * f) % (n - n // 8)
        m = np.zeros(n, bool); m[a:a + n // 8] = True
        out.append(m)
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "filter_multi_bench.json"))
    args = ap.parse_args()
    n, d, k, nq = args.rows, args.dim, args.k, args.queries
    idx = ShardIndex(fill_unit_rows(n, d, 1), prefilter=None)
    Q_ = fill_unit_rows(nq, d, 2)
    rs = np.random.RandomState(0)
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "k": k, "queries": nq, "calls": args.calls,
           "unit": "ms per batch of all queries", "results": []}
    for F in (1, 8, 64):
        for kind in ("random 1%", "random 50%", "contiguous 12.5%"):
            ms = masks_of(kind, F, n, rs)
            allows = torch.from_numpy(np.stack([pack_bitmap(m).view(np.int64) for m in ms])).cuda()
            fo = (torch.arange(nq, device="cuda") % F).to(torch.int32)
            subsets = [(f, torch.nonzero(fo == f).flatten()) for f in range(F)]
            subsets = [(f, Q_[qs].contiguous()) for f, qs in subsets if qs.numel()]
            s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            i = torch.empty((nq, k), dtype=torch.int64, device="cuda")

            def multi():
                return idx.search_filtered_many(Q_, allows, fo, k, out=(s, i))

            def loop():
                return [idx.search(q, k, allow=allows[f]) for f, q in subsets]
            multi()
            for (f, _), (ls, li) in zip(subsets, loop()):        # the same answers, bit for bit, before any timing
                qs = torch.nonzero(fo == f).flatten()
                assert torch.equal(li, i[qs]) and torch.equal(ls.view(torch.int32), s[qs].view(torch.int32)), (F, kind, f)
            over, groups = idx.filtered_many_stats()
            for _ in range(5):
                multi(); loop()
            torch.cuda.synchronize()
            t_multi, t_loop = [], []
            for _ in range(args.calls):
                t_multi.append(event_ms(multi))
                t_loop.append(event_ms(loop))
            row = {"filters": F, "mask": kind, "allowed_rows_per_filter": int(np.mean([m.sum() for m in ms])),
                   "multi_ms_median": float(np.median(t_multi)), "multi_ms_min": float(min(t_multi)),
                   "per_filter_loop_ms_median": float(np.median(t_loop)), "per_filter_loop_ms_min": float(min(t_loop)),
                   "loop_calls": len(subsets), "overflowed_queries": over, "candidate_groups": groups}
            row["loop_over_multi"] = row["per_filter_loop_ms_median"] / row["multi_ms_median"]
            out["results"].append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
