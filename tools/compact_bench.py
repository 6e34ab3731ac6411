#!/usr/bin/env python
"""Times the device compaction (`arx_compact_plan`, `arx_compact_rows`, `arx_compact_text`; csrc/compact.hip) and the mutable
`HipCollection` built on it, on one GPU.

One process, the arms in turn.  Kernel arms: `--rows` x 768 fp16 rows and a text blob of about 1.1 KB a row, under three tombstone
patterns (random 10 %, random 50 %, a contiguous 12.5 %); each call is timed between two events on the stream, median of `--repeats`,
and stands beside its floor: the bytes it must read plus the bytes it must write at the 6.29 TB/s copy rate the other tools use.
Collection arms (`--collection-rows`, texts and `group_key` present, no keyword index: tokenising the texts is host work that the
mutation neither adds nor saves): whole `compact()` after a random 10 % delete and whole `add` of 10 000 rows, each including the int8
rebuild of the new `ShardIndex`, beside the only alternative an immutable collection offers: building a new `HipCollection` from the
surviving host arrays.  Wall-clock, median of `--collection-repeats`.  Results -> profiles/compact_bench.json.
Run it under a time limit (e.g. `timeout -k 10 900 python tools/compact_bench.py`)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import _lib      # noqa: E402
from arxiv_rag_amd.where import pack_bitmap      # noqa: E402

COPY_RATE = 6.29e12
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


def beside_floor(t, bytes_moved):
    floor_ms = bytes_moved / COPY_RATE * 1e3
    return {**t, "bytes_read_plus_written": int(bytes_moved), "floor_ms": floor_ms, "times_floor": t["ms_median"] / floor_ms,
            "achieved_TBps": bytes_moved / (t["ms_median"] * 1e-3) / 1e12}


def kernel_arms(n, dim, repeats, out):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(0)
    shard = torch.randn((n, dim), device=DEV).half()
    dst = torch.empty_like(shard)
    lens = rs.randint(900, 1300, size=n).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[-1])
    blob = torch.randint(0, 256, (total,), dtype=torch.uint8, device=DEV)
    new_blob = torch.empty_like(blob)
    off_d = torch.from_numpy(off).to(DEV)
    n_words = (n + 63) // 64
    a = n // 3
    masks = {"random 10 % deleted": rs.rand(n) >= 0.10, "random 50 % deleted": rs.rand(n) >= 0.50,
             "contiguous 12.5 % deleted": ~((np.arange(n) >= a) & (np.arange(n) < a + n // 8))}
    for name, keep in masks.items():
        words = torch.from_numpy(pack_bitmap(keep).view(np.int64).copy()).to(DEV)
        rank = torch.empty(n_words + 1, dtype=torch.int64, device=DEV)
        cnt = torch.empty(1, dtype=torch.int64, device=DEV)
        count, kept_bytes = int(keep.sum()), int(lens[keep].sum())
        new_off = torch.empty(count + 1, dtype=torch.int64, device=DEV)

        def plan():
            _lib.check(lib.arx_compact_plan(words.data_ptr(), n, rank.data_ptr(), cnt.data_ptr(), st), "arx_compact_plan")

        def rows():
            _lib.check(lib.arx_compact_rows(shard.data_ptr(), dst.data_ptr(), 2 * dim, n, words.data_ptr(), rank.data_ptr(), st), "arx_compact_rows")

        def text():
            _lib.check(lib.arx_compact_text(blob.data_ptr(), off_d.data_ptr(), n, words.data_ptr(), rank.data_ptr(), new_blob.data_ptr(),
                                            new_off.data_ptr(), st), "arx_compact_text")
        row = {"rows": n, "dim": dim, "text_bytes": total, "tombstones": name, "kept_rows": count,
               "plan": beside_floor(timed(plan, repeats), 8 * n_words + 8 * (n_words + 1)),
               "row_move": beside_floor(timed(rows, repeats), 2 * count * 2 * dim + 16 * n_words),
               "text_move": beside_floor(timed(text, repeats), 2 * kept_bytes + 8 * (n + 1) + 8 * (count + 1) + 16 * n_words)}
        assert int(cnt.item()) == count and int(new_off[-1].item()) == kept_bytes
        out["kernels"].append(row)
        print(json.dumps(row), flush=True)


def wall(fn, repeats, setup=None):
    runs = []
    for _ in range(repeats):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(runs)), "ms_min": float(min(runs)), "runs": len(runs)}


def collection_arms(n, dim, repeats, out):
    from arxiv_rag_amd.store import HipCollection
    rs = np.random.RandomState(1)
    emb = rs.standard_normal((n + 10000, dim)).astype(np.float16)
    word = "".join(chr(97 + i % 26) for i in range(1100))
    meta = [{"chunk_id": f"c{j}", "text": word[j % 50:] + str(j), "paper_id": f"p{j // 8}"} for j in range(n + 10000)]
    kw = dict(device=DEV, documents=True, group_key="paper_id")
    gone = rs.rand(n) < 0.10
    surv = np.nonzero(~gone)[0]
    ids = [f"c{j}" for j in np.nonzero(gone)[0]]

    def fresh_mutable():
        col = HipCollection(emb[:n], meta[:n], capacity=n + 10000, **kw)
        col.compact()                                            # (nothing to do; allocates nothing either)
        return col

    def deleted():
        col = fresh_mutable()
        col._buf_spare = torch.empty_like(col._buf)              # the second buffer exists from the first real compaction on
        col.delete(ids=ids)
        return col
    res = {"rows": n, "dim": dim, "text_bytes": int(sum(len(m["text"]) for m in meta[:n])),
           "compact() after a random 10 % delete": wall(lambda col: col.compact(), repeats, deleted),
           "rebuild from the survivors": wall(lambda _: HipCollection(emb[surv], [meta[r] for r in surv], **kw), repeats),
           "add of 10 000 rows": wall(lambda col: col.add(emb[n:], meta[n:]), repeats, fresh_mutable),
           "rebuild with the 10 000 rows": wall(lambda _: HipCollection(emb, meta, **kw), repeats)}
    out["collection"].append(res)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--collection-rows", type=int, default=1_000_000)
    ap.add_argument("--collection-repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "compact_bench.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "kernels": [], "collection": []}
    kernel_arms(args.rows, args.dim, args.repeats, out)
    torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")      # (the kernel arms are kept even if the collection arms run out of time)
    if args.collection_rows > 0:
        collection_arms(args.collection_rows, args.dim, args.collection_repeats, out)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
