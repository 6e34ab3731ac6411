#!/usr/bin/env python
"""Times MMR retrieval (arx_gather_rows, arx_mmr_select, HipCollection.query(mmr_lambda=...)) against the search it follows.

One process, one GPU: `fill_unit_rows(1 M, 768)`, n = 32 candidates, m = 10 picks, Q in {1, 64, 256}.  Per Q, the median of `--calls`
(20) calls of:
  gather kernel        arx_gather_rows on the [Q, 32] ids of a search          (one event pair per call)
  select kernel        arx_mmr_select on the gathered rows                      (one event pair per call)
  search k=10 / k=32   ShardIndex.search, what the two `query` arms run first   (one event pair per call)
  query                HipCollection.query(n_results=10)                        (wall clock: it ends with copies to the host)
  query k=32           HipCollection.query(n_results=32): the cost of fetching the candidates alone
  query mmr            HipCollection.query(n_results=10, n_candidates=32, mmr_lambda=0.5)
  host path            what a caller would otherwise run after query k=32: ids to the host, the candidates' rows fetched from the device,
                       `mmr_reference_f64(dtype=float32)` per query in numpy     (wall clock)
Writes profiles/mmr_bench.json.  Run it under a time limit (e.g. `timeout -k 10 500 python tools/mmr_bench.py`)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import _lib                                           # noqa: E402
from arxiv_rag_amd.index import fill_unit_rows                           # noqa: E402
from arxiv_rag_amd.mmr import gather_rows, mmr_reference_f64             # noqa: E402
from arxiv_rag_amd.store import HipCollection                            # noqa: E402


def device_ms(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "calls": calls, "clock": "device events"}


def wall_ms(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "calls": calls, "clock": "wall"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "mmr_bench.json"))
    args = ap.parse_args()
    n_rows, d, n, m = args.rows, args.dim, args.n, args.m
    lib = _lib.load()
    rows = fill_unit_rows(n_rows, d, 1)
    meta = [{"chunk_id": f"c{r}", "text": ""} for r in range(n_rows)]
    coll = HipCollection(rows.cpu().numpy(), meta)
    del rows
    idx = coll.index
    out = {"device": torch.cuda.get_device_name(0), "rows": n_rows, "dim": d, "candidates": n, "picks": m, "lambda": 0.5, "results": []}

    def add(nq, arm, t):
        out["results"].append({"queries": nq, "arm": arm, **t})
        print(json.dumps(out["results"][-1]), flush=True)
    for nq in (1, 64, 256):
        qd = fill_unit_rows(nq, d, 2)
        qh = qd.cpu().numpy()
        st = torch.cuda.current_stream().cuda_stream
        s, ids = idx.search(qd, n)
        cand = gather_rows(idx, ids)
        order = torch.empty((nq, m), dtype=torch.int32, device="cuda")
        val = torch.empty((nq, m), dtype=torch.float32, device="cuda")
        add(nq, "gather kernel", device_ms(lambda: lib.arx_gather_rows(idx.corpus.data_ptr(), idx.n_rows, d, idx.idx_base, ids.data_ptr(), ids.numel(),
                                                                        cand.data_ptr(), st), args.calls))
        add(nq, "select kernel", device_ms(lambda: lib.arx_mmr_select(qd.data_ptr(), cand.data_ptr(), ids.data_ptr(), nq, n, d, m, 0.5, order.data_ptr(),
                                                                       val.data_ptr(), st), args.calls))
        add(nq, "search k=10", device_ms(lambda: idx.search(qd, m), args.calls))
        add(nq, f"search k={n}", device_ms(lambda: idx.search(qd, n), args.calls))
        add(nq, "query", wall_ms(lambda: coll.query(query_embeddings=qh, n_results=m), args.calls))
        add(nq, f"query k={n}", wall_ms(lambda: coll.query(query_embeddings=qh, n_results=n), args.calls))
        add(nq, "query mmr", wall_ms(lambda: coll.query(query_embeddings=qh, n_results=m, n_candidates=n, mmr_lambda=0.5), args.calls))

        def host_path():
            ih = ids.cpu().numpy()
            ch = idx.corpus[(ids - idx.idx_base).clamp(min=0)].cpu().numpy().astype(np.float32)
            return mmr_reference_f64(qh.astype(np.float32), ch, ih, m, 0.5, dtype=np.float32)
        add(nq, "host path", wall_ms(host_path, args.calls))
        want = host_path()[0]
        agree = float((order.cpu().numpy() == want).mean())
        out["results"].append({"queries": nq, "arm": "picks equal to the host path's", "fraction": agree})
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
