#!/usr/bin/env python
"""Times Chroma `where` filters on the host path (`where.evaluate` on cached columns + `pack_bitmap` + the upload: the default of
`HipCollection`) against the device path (`where_device.MetadataColumns.allow_many`: lowering, one `arx_where_eval` launch, the count
read), in one process on one GPU, to profiles/where_device_bench.json.

Records: `--rows` (1 M) synthetic chunk records with `section` (5 values), `quality_score` (uniform), `year` (25 values) and
`paper_id = f"p{i // 64:06d}"`.  Arms:
* the five single filters of the table in README.md, host and device in turn, median of `--calls` (20) wall-clock runs each with a device
  synchronisation at the end (a host arm stops early once it has used `--host-budget` seconds; `calls` says how many ran); beside the
  device time the span of the launch between two stream events, and the floor: the bytes of the distinct columns the filter reads
  (9 per row and key) at the chip's measured 6.29 TB/s copy rate, with the multiple of it;
* 64 distinct filters in one `allow_many` against 64 host evaluations: the numeric filter with 64 thresholds, the `$in` filter with 64
  lists of 100 ids;
* a whole `HipCollection.query` of 64 queries (k = 10, dim 768) with a per-query filter list, on a default collection and on one with
  `where_on_device=True` over the same rows; the results are asserted equal.
Every device bitmap is asserted equal to the host one before it is timed.  Run it under a time limit
(e.g. `timeout -k 10 1100 python tools/where_device_bench.py`)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd.index import ShardIndex, fill_unit_rows                        # noqa: E402
from arxiv_rag_amd.store import HipCollection                                     # noqa: E402
from arxiv_rag_amd.where import compile_where, evaluate, keys_of, pack_bitmap     # noqa: E402
from arxiv_rag_amd.where_device import MetadataColumns                            # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured device-to-device copy rate
SECTIONS = ("abstract", "introduction", "methods", "results", "discussion")
# evaluate + pack_bitmap of the same filters, measured on the CPU-only build machine (best of 3, columns cached; the string $gte ran once)
CPU_BUILD_MACHINE_MS = {"quality_score $gte": 1.7, "section $eq": 9.6, "$and of section, quality_score, year": 13.3, "paper_id $gte": 139.0,
                        "paper_id $in 100 ids": 2322.0}


def make_records(n, seed=0):
    rs = np.random.RandomState(seed)
    sec, q, year = rs.randint(5, size=n), rs.rand(n), 2000 + rs.randint(25, size=n)
    return [{"chunk_id": f"c{i}", "section": SECTIONS[sec[i]], "quality_score": float(q[i]), "year": int(year[i]), "paper_id": f"p{i // 64:06d}"}
            for i in range(n)]


def wall_times(fn, calls, budget_s=None, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms, t_all = [], time.perf_counter()
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if budget_s is not None and time.perf_counter() - t_all > budget_s:
            break
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "calls": len(ms)}


def event_times(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds after which a host arm stops repeating")
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "where_device_bench.json"))
    args = ap.parse_args()
    n, dev = args.rows, "cuda:0"
    t0 = time.perf_counter()
    meta = make_records(n)
    print(f"records: {n} in {time.perf_counter() - t0:.1f} s", flush=True)
    cache = {}
    cols = MetadataColumns(meta, 0, n, dev)
    build = {}
    for key in ("section", "quality_score", "year", "paper_id"):
        t0 = time.perf_counter()
        evaluate(compile_where({key: {"$ne": 0}}), meta, cache=cache)
        build[key] = {"host_column_s": time.perf_counter() - t0}
        t0 = time.perf_counter()
        cols.device_column(key)
        torch.cuda.synchronize()
        build[key]["device_column_s"] = time.perf_counter() - t0
    print(json.dumps(build), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "column_bytes_per_row_and_key": 9, "column_build": build,
           "floor": "bytes of the distinct columns the filter reads / 6.29 TB/s (the chip's measured copy rate)",
           "cpu_build_machine_ms": {"what": "evaluate + pack_bitmap, measured on the CPU-only build machine", **CPU_BUILD_MACHINE_MS},
           "single": [], "batch64": [], "query": []}

    def host_allow(tree):
        mask = evaluate(tree, meta, 0, n, cache=cache)
        return torch.from_numpy(pack_bitmap(mask).view(np.int64)).to(dev), int(mask.sum())

    ids100 = [f"p{(37 * j) % (n // 64 + 1):06d}" for j in range(100)]
    singles = [("quality_score $gte", {"quality_score": {"$gte": 0.95}}), ("section $eq", {"section": "abstract"}),
               ("$and of section, quality_score, year", {"$and": [{"section": "abstract"}, {"quality_score": {"$gte": 0.95}}, {"year": {"$gte": 2015}}]}),
               ("paper_id $gte", {"paper_id": {"$gte": "p010000"}}), ("paper_id $in 100 ids", {"paper_id": {"$in": ids100}})]
    for name, f in singles:
        tree = compile_where(f)
        (hb, hc), (db, dc) = host_allow(tree), cols.allow_many([tree])
        assert torch.equal(hb, db[0]) and hc == dc[0], (name, "device and host disagree")
        host = wall_times(lambda: host_allow(tree), args.calls, args.host_budget, warm=0)
        device = wall_times(lambda: cols.allow_many([tree]), args.calls)
        prog = cols.lower([tree])
        ob, oc = torch.empty((1, cols.n_words), dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        span = event_times(lambda: cols.run_program(prog, ob, oc), args.calls)
        floor = cols.column_bytes(keys_of(tree)) / COPY_RATE * 1e3
        row = {"arm": name, "rows_allowed": hc, "host": host, "device": device, "device_launch_span_ms": span, "floor_ms": floor,
               "device_times_the_floor": device["ms_median"] / floor, "launch_span_times_the_floor": span / floor,
               "host_over_device": host["ms_median"] / device["ms_median"], "device_slower_than_host": device["ms_median"] > host["ms_median"],
               "cpu_build_machine_ms": CPU_BUILD_MACHINE_MS[name]}
        out["single"].append(row)
        print(json.dumps(row), flush=True)

    batches = [("quality_score $gte, 64 thresholds", [{"quality_score": {"$gte": 0.5 + j / 130.0}} for j in range(64)]),
               ("paper_id $in, 64 lists of 100 ids", [{"paper_id": {"$in": [f"p{(37 * i + 101 * j) % (n // 64 + 1):06d}" for i in range(100)]}} for j in range(64)])]
    for name, fs in batches:
        trees = [compile_where(f) for f in fs]
        bits, counts = cols.allow_many(trees)
        t0 = time.perf_counter()
        hosts = [host_allow(t) for t in trees]
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        assert all(torch.equal(hb, bits[j]) and hc == counts[j] for j, (hb, hc) in enumerate(hosts)), (name, "device and host disagree")
        host = {"ms_median": first_ms, "ms_min": first_ms, "calls": 1} if first_ms > 5e3 else \
            wall_times(lambda: [host_allow(t) for t in trees], args.calls, args.host_budget, warm=0)
        device = wall_times(lambda: cols.allow_many(trees), args.calls)
        floor = cols.column_bytes(set().union(*(keys_of(t) for t in trees))) / COPY_RATE * 1e3
        row = {"arm": name, "filters": 64, "host": host, "device": device, "floor_ms_one_pass_over_the_columns": floor,
               "device_times_the_floor": device["ms_median"] / floor, "device_times_64_floors": device["ms_median"] / (64 * floor),
               "host_over_device": host["ms_median"] / device["ms_median"], "device_slower_than_host": device["ms_median"] > host["ms_median"]}
        out["batch64"].append(row)
        print(json.dumps(row), flush=True)

    # ---- whole queries: two collections over the same device rows ----
    rows = fill_unit_rows(n, args.dim, 1)
    index = ShardIndex(rows, idx_base=0, prefilter="int8", adaptive=True)

    def collection(on_device):
        c = HipCollection.__new__(HipCollection)
        c.n_total, c.dim, c.lo, c.hi, c.world = n, args.dim, 0, n, 1
        c.metadata, c._where_columns, c.encoder, c.keyword, c.documents = meta, cache, None, None, None
        c.group_key = c.group_keys = c._keep = c._keep_mask = c.dedup_threshold = None
        c.duplicates, c.index = [], index
        c.where_on_device, c._device_columns = on_device, cols if on_device else None
        return c
    plain, on_dev = collection(False), collection(True)
    q = fill_unit_rows(64, args.dim, 2).cpu().numpy()
    for name, fs in batches:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = plain.query(query_embeddings=q, n_results=10, where=fs)
        first_ms = (time.perf_counter() - t0) * 1e3
        assert a == on_dev.query(query_embeddings=q, n_results=10, where=fs), (name, "the two collections disagree")
        host = {"ms_median": first_ms, "ms_min": first_ms, "calls": 1} if first_ms > 5e3 else \
            wall_times(lambda: plain.query(query_embeddings=q, n_results=10, where=fs), args.calls, args.host_budget, warm=0)
        device = wall_times(lambda: on_dev.query(query_embeddings=q, n_results=10, where=fs), args.calls)
        row = {"arm": f"query, 64 queries, k=10, dim {args.dim}, per-query where: {name}", "default_collection": host, "where_on_device": device,
               "default_over_device": host["ms_median"] / device["ms_median"], "device_slower_than_host": device["ms_median"] > host["ms_median"]}
        out["query"].append(row)
        print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
