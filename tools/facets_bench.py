#!/usr/bin/env python
"""Times facet counts on the device (`facets.count`: one `arx_facet_count` per call, the top bins taken with `torch.topk`, one read)
against two host arms in the same process, on one GPU, to profiles/facets_bench.json.

Records: `--rows` (1 M) synthetic chunk records with `section` (10 values), `paper_id` (about 20 000 values, 50 consecutive rows
each: the order a corpus is loaded in), `paper_shuffled` (the same ids in random row order) and `quality_score` (uniform, counted under
4 edges).  Arms, each the median of `--calls` (20) wall-clock runs with a device synchronisation at the end:
* 1 and 64 filters, every bitmap of a call of one kind: all rows, a random 1 %, a contiguous 12.5 % (its start moves with the filter);
  the keys `section`, `paper_id`, `paper_shuffled` and `quality_score` under the edges, one call each;
* `section`, `paper_id` and `quality_score` in one call against one call each (all rows, 1 filter);
* the kernel alone, between two stream events: `section` through the LDS histogram against the forced direct path, and `paper_id` /
  `paper_shuffled` (20 002 counters: direct by default) against an LDS histogram of 32 768 counters.
Beside each arm the floor (the bytes of the column, 9 per row, plus the bitmaps, at the chip's measured 6.29 TB/s copy rate) and the
two host arms: `np.bincount` over cached numpy columns under the mask (what a caller who rebuilt the columns would run) and the
`collections.Counter` loop over the metadata dicts (`facets.oracle`; run once, on 1 filter).  Every device result is asserted equal to
the `np.bincount` one before it is timed.  Run it under a time limit (e.g. `timeout -k 10 900 python tools/facets_bench.py`)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import facets as F                                              # noqa: E402
from arxiv_rag_amd.where import pack_bitmap                                        # noqa: E402
from arxiv_rag_amd.where_device import MetadataColumns                            # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured device-to-device copy rate
SECTIONS = ("abstract", "introduction", "related work", "background", "methods", "experiments", "results", "discussion", "conclusion",
            "appendix")
EDGES = [0.0, 0.5, 0.9, 0.95, 1.0]
ROWS_PER_PAPER = 50


def make_records(n, seed=0):
    rs = np.random.RandomState(seed)
    sec, q = np.minimum(rs.zipf(1.5, n) - 1, 9), rs.rand(n)
    paper = np.arange(n) // ROWS_PER_PAPER
    shuffled = paper[rs.permutation(n)]
    return [{"section": SECTIONS[sec[i]], "paper_id": f"p{paper[i]:06d}", "paper_shuffled": f"p{shuffled[i]:06d}", "quality_score": float(q[i])}
            for i in range(n)]


def wall_times(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
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


def host_bincount(f, kind, val, masks, top):
    """The host arm: np.bincount over cached numpy columns under each mask, the top list by the same rule."""
    out = []
    for m in masks:
        out.append(F._from_counters(f, F.bin_counts_host(f.mode, f.want_kind, f.n_bins, f.cuts, kind, val, m), top))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "facets_bench.json"))
    args = ap.parse_args()
    n, dev, top = args.rows, "cuda:0", args.top
    t0 = time.perf_counter()
    meta = make_records(n)
    print(f"records: {n} in {time.perf_counter() - t0:.1f} s", flush=True)
    cols = MetadataColumns(meta, 0, n, dev)
    specs = {"section": "section", "paper_id": "paper_id", "paper_shuffled": "paper_shuffled",
             "quality_score under 4 edges": {"key": "quality_score", "edges": EDGES}}
    build, host_cols, facets = {}, {}, {}
    for name, spec in specs.items():
        key = spec if isinstance(spec, str) else spec["key"]
        t0 = time.perf_counter()
        cols.device_column(key)
        facets[name] = F.resolve(cols, spec)
        torch.cuda.synchronize()
        build[name] = {"column_and_resolve_s": time.perf_counter() - t0, "bins": facets[name].n_bins}
        host_cols[name] = cols.host_column(key)
    print(json.dumps(build), flush=True)
    rs = np.random.RandomState(1)

    def masks_of(kind, nf):
        if kind == "all rows":
            return [np.ones(n, bool)] * nf
        if kind == "random 1 %":
            return [rs.rand(n) < 0.01 for _ in range(nf)]
        out = []
        for j in range(nf):
            m = np.zeros(n, bool)
            a = 37 + (j * (n - n // 8 - 64)) // max(1, nf)
            m[a:a + n // 8] = True
            out.append(m)
        return out

    out = {"device": torch.cuda.get_device_name(0), "rows": n, "top": top, "column_build": build,
           "floor": "(9 bytes per row of the key's column + the bitmap words of every filter) / 6.29 TB/s (the chip's measured copy rate)",
           "what": "ms per call: device = facets.count (launch, topk, one read); host_bincount = np.bincount over cached numpy columns "
                   "under the masks; host_counter = facets.oracle, the Counter loop over the dicts (one run, 1 filter)",
           "filters": [], "keys_in_one_call": None, "kernel_paths": []}
    counter_ms = {}
    for kind in ("all rows", "random 1 %", "contiguous 12.5 %"):
        for nf in (1, 64):
            masks = masks_of(kind, nf)
            bits = torch.from_numpy(np.stack([pack_bitmap(m) for m in masks]).view(np.int64)).to(dev)
            for name, spec in specs.items():
                f = facets[name]
                hk, hv = host_cols[name]
                got = F.count(cols, [spec], bits, top)
                want = host_bincount(f, hk, hv, masks, top)
                assert [g[0] for g in got] == want, (kind, nf, name, "device and host disagree")
                device = wall_times(lambda: F.count(cols, [spec], bits, top), args.calls)
                host = wall_times(lambda: host_bincount(f, hk, hv, masks, top), args.calls if nf == 1 else 3, warm=0)
                floor = (9 * n + 8 * cols.n_words * nf) / COPY_RATE * 1e3
                row = {"bitmaps": kind, "filters": nf, "key": name, "device": device, "host_bincount": host, "floor_ms": floor,
                       "device_times_the_floor": device["ms_median"] / floor, "bincount_over_device": host["ms_median"] / device["ms_median"],
                       "device_slower_than_bincount": device["ms_median"] > host["ms_median"]}
                if nf == 1:
                    if (kind, name) not in counter_ms:
                        t0 = time.perf_counter()
                        ref = F.oracle(meta, 0, n, [spec], masks, top)
                        counter_ms[(kind, name)] = (time.perf_counter() - t0) * 1e3
                        assert ref[0] == got[0], (kind, name, "device and Counter disagree")
                    row["host_counter_ms"] = counter_ms[(kind, name)]
                out["filters"].append(row)
                print(json.dumps(row), flush=True)

    three = [specs["section"], specs["paper_id"], specs["quality_score under 4 edges"]]
    together = wall_times(lambda: F.count(cols, three, None, top), args.calls)
    apart = wall_times(lambda: [F.count(cols, [s], None, top) for s in three], args.calls)
    assert F.count(cols, three, None, top)[0] == [F.count(cols, [s], None, top)[0][0] for s in three]
    out["keys_in_one_call"] = {"keys": ["section", "paper_id", "quality_score under 4 edges"], "bitmaps": "all rows (allow = NULL)", "filters": 1,
                               "one_call": together, "one_call_each": apart, "each_over_one": apart["ms_median"] / together["ms_median"],
                               "floor_ms": 3 * 9 * n / COPY_RATE * 1e3}
    print(json.dumps(out["keys_in_one_call"]), flush=True)

    bx = max(1, min(512, -(-cols.n_words // 64)))               # the default grid of a 256-thread block on this chip
    for name, shapes in (("section", (("LDS histogram (default)", (256, bx, 8192)), ("direct to out (lds_bins = 0)", (256, bx, 0)))),
                         ("paper_id", (("direct to out (default)", (256, bx, 8192)), ("LDS histogram of 32 768 counters", (256, bx, 32768)))),
                         ("paper_shuffled", (("direct to out (default)", (256, bx, 8192)), ("LDS histogram of 32 768 counters", (256, bx, 32768))))):
        f = facets[name]
        kd, vd = cols.device_column(f.key)
        buf = torch.empty(f.n_bins + 2, dtype=torch.int32, device=dev)
        keys = [(kd, vd, f.cuts_device(dev), f.mode, f.want_kind, f.n_bins, 0)]
        ref = None
        for label, tuned in shapes:
            F.launch(keys, n, None, 0, 1, buf, f.n_bins + 2, tuned=tuned)
            now = buf.cpu().numpy().copy()
            assert ref is None or np.array_equal(ref, now), (name, label, "the two paths disagree")
            ref = now
            span = event_times(lambda: F.launch(keys, n, None, 0, 1, buf, f.n_bins + 2, tuned=tuned), args.calls)
            row = {"key": name, "bins": f.n_bins, "path": label, "block_threads": tuned[0], "blocks_x": tuned[1], "lds_bins": tuned[2],
                   "bitmaps": "all rows (allow = NULL)", "kernel_span_ms": span, "floor_ms": 9 * n / COPY_RATE * 1e3,
                   "span_times_the_floor": span / (9 * n / COPY_RATE * 1e3)}
            out["kernel_paths"].append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
