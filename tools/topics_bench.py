#!/usr/bin/env python
"""Times one Lloyd iteration of the topic clustering (`arxiv_rag_amd/topics.py`; csrc/cluster.hip) stage by stage, on one GPU.

One process, the arms in turn: `--rows` x `--dim` clustered fp16 rows (`fill_clustered_rows`) at C = 64, 256 and 1024, then two
filtered sets at C = 256 (a random 10 % and a contiguous 12.5 % of the rows, gathered once with `arx_gather_rows`).  Per arm the
stages of an iteration are timed apart, each between two events on the stream, median of `--repeats`:
  assign_kernel   `topics.assign(how="kernel")`: `arx_cluster_assign`, with its `stats` (rows flagged, slow-path scores) and beside its
                  floor: the larger of the bytes of X at the copy rate and 2 n C dim flop at the fp16 dense-MFMA rate (2.5 PF/s, the
                  specification figure, not a measurement of this repository)
  assign_search   `topics.assign(how="search")`: the exact k = 1 search of every row over the centroids, in batches of 65 536 (what
                  the assign was before the kernel), timed in the same process right after it
  sort     `topics.members`: the stable sort of the labels, `bincount` and the cumulative sum
  sums     `arx_cluster_sums`, beside its floor: the bytes of X at the 6.29 TB/s copy rate the other tools use
  finish   `arx_cluster_finish`
and, for comparison, the update a caller would otherwise write in torch: `index_add_` of the rows in f32 (float atomics: another
result on every run).  Results -> profiles/topics_bench.json.
Run it under a time limit (e.g. `timeout -k 10 600 python tools/topics_bench.py`)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import topics as T      # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows      # noqa: E402

COPY_RATE = 6.29e12
MFMA_F16_RATE = 2.5e15          # fp16 dense MFMA, flop/s: the MI355X specification figure
DEV = "cuda:0"


def timed(fn, repeats):
    fn()
    runs = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(runs)), "ms_min": float(min(runs)), "runs": len(runs)}


def arm(name, X, C, repeats, out):
    n, dim = int(X.shape[0]), int(X.shape[1])
    rows = torch.from_numpy(T.default_init_rows(n, C, 0)).to(DEV)
    c32 = X.index_select(0, rows).float()
    c16 = c32.half()
    assign_ws = T.assign_workspace(n, C, dim, DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    labels, scores = T.cluster_assign(X, c16, stats=stats, ws=assign_ws)     # the state after a first assign: what every later iteration looks like
    sl, ss = T.assign(X, c16, how="search")
    same_bits = bool(torch.equal(labels, sl) and torch.equal(scores.view(torch.int32), ss.contiguous().view(torch.int32)))
    order, start, sizes = T.members(labels, C)
    ws = torch.empty(((n + T.RUN - 1) // T.RUN + C) * dim, dtype=torch.float32, device=DEV)
    sums = torch.empty((C, dim), dtype=torch.float32, device=DEV)
    labels64 = labels.long()
    acc = torch.zeros((C, dim), dtype=torch.float32, device=DEV)

    def torch_update():
        acc.zero_()
        acc.index_add_(0, labels64, X.float())
    x_bytes = n * dim * 2
    floor_ms = x_bytes / COPY_RATE * 1e3
    row = {"arm": name, "rows": n, "dim": dim, "clusters": C, "largest_cluster": int(sizes.max().item()),
           "empty_clusters": int((sizes == 0).sum().item()),
           "assign_kernel": timed(lambda: T.assign(X, c16, how="kernel", ws=assign_ws), repeats),
           "assign_search": timed(lambda: T.assign(X, c16, how="search"), repeats),
           "sort": timed(lambda: T.members(labels, C), repeats),
           "sums": timed(lambda: T.cluster_sums(X, order, start, C, out=sums, ws=ws), repeats),
           "finish": timed(lambda: T.cluster_finish(sums, start, c32), repeats),
           "torch_index_add_f32": timed(torch_update, repeats)}
    row["sums"].update(bytes_of_X=x_bytes, floor_ms=floor_ms, times_floor=row["sums"]["ms_median"] / floor_ms,
                       achieved_TBps=x_bytes / (row["sums"]["ms_median"] * 1e-3) / 1e12)
    flagged, slow_scores = (int(v) for v in stats.cpu().tolist())
    assign_floor_ms = max(floor_ms, 2.0 * n * C * dim / MFMA_F16_RATE * 1e3)
    row["assign_kernel"].update(rows_flagged=flagged, slow_path_scores=slow_scores, same_bits_as_search=same_bits, floor_ms=assign_floor_ms,
                                floor_is="X bytes" if assign_floor_ms == floor_ms else "MFMA flop",
                                times_floor=row["assign_kernel"]["ms_median"] / assign_floor_ms)
    row["assign_search_over_kernel"] = row["assign_search"]["ms_median"] / row["assign_kernel"]["ms_median"]
    stages = ("assign_kernel", "sort", "sums", "finish")
    total = sum(row[k]["ms_median"] for k in stages)
    row["iteration_ms"] = total
    row["share_of_iteration"] = {k: row[k]["ms_median"] / total for k in stages}
    out["arms"].append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "topics_bench.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "mfma_f16_rate_PFps": MFMA_F16_RATE / 1e15,
           "mfma_f16_rate_source": "MI355X specification (dense fp16 MFMA), not measured here", "arms": []}
    X = fill_clustered_rows(args.rows, args.dim, 1, 256, device=DEV)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    for C in (64, 256, 1024):
        arm(f"all rows, C = {C}", X, C, args.repeats, out)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")      # (the arms so far are kept if a later one runs out of time)
    index = ShardIndex(X)
    n = args.rows
    rs = np.random.RandomState(0)
    a = n // 3
    for name, keep in (("random 10 % of the rows, C = 256", rs.rand(n) < 0.10),
                       ("contiguous 12.5 % of the rows, C = 256", (np.arange(n) >= a) & (np.arange(n) < a + n // 8))):
        rows = torch.from_numpy(np.nonzero(keep)[0]).to(DEV)
        gather = timed(lambda: T.gather(index, rows), 5)
        arm(name, T.gather(index, rows), 256, args.repeats, out)
        out["arms"][-1]["gather_once"] = gather
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
