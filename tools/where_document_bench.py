#!/usr/bin/env python
"""Times the `where_document` substring scan (`arx_text_contains`) and `HipCollection.query(where_document=...)`.

One process, one GPU.  Corpus: `--rows` (1 M) synthetic chunks of 200-2000 characters cut out of one seeded text of lower-case
pseudo-words (the range `text_processing.max_chunk_size` produces).  Into 0.1 % of the chunks a "rare" marker of 3, 8 and 64 bytes is
written, into 50 % a "common" one (upper-case letters, which the text itself never holds: the selectivity is exact, and the first
bytes of the pattern are as selective as they can be); the 8- and 32-pattern arms take real words of the text instead (3-12 bytes,
first bytes that occur everywhere).

Arms, all in one run, to profiles/where_document_bench.json:
* scan: one `arx_text_contains` launch per call with the patterns already on the device, 3 warm-up calls, then the median (and
  minimum) of `--calls` (20) calls, each between its own pair of events on the stream; blob GB, GB/s, rows matched; beside it the
  floor (blob bytes at the chip's measured 6.29 TB/s copy rate) and `evaluate_host` of the same filter in this process (wall clock, one
  run: the only alternative a caller has without the kernel) with the ratio;
* query: `HipCollection.query` at 64 queries and at 1 query (k = 10, dim 768 unit rows from `fill_unit_rows`), wall clock around the
  call with a device synchronisation (it ends in a host copy anyway), median of `--calls`: unfiltered, `where=` on a metadata flag
  with the same rows set (host-evaluated, its columns cached after the first call), and `where_document=`.  The collection is put
  together from a `ShardIndex` over device-generated rows and a `DocumentStore` (its constructor wants the embeddings on the host;
  `query` itself is the shipped code).
Run it under a time limit (e.g. `timeout -k 10 540 python tools/where_document_bench.py`)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import _lib                                                   # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_unit_rows                        # noqa: E402
from arxiv_rag_amd.store import HipCollection                                     # noqa: E402
from arxiv_rag_amd.where_document import DocumentStore, compile_where_document, evaluate_host, pack_patterns      # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, the chip's measured device-to-device copy rate


def make_corpus(n, seed):
    rs = np.random.RandomState(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    lens = rs.randint(2, 13, size=20000)
    flat = rs.choice(letters, size=int(lens.sum()), p=np.r_[[0.08] * 5, [0.6 / 21] * 21])
    words, at = [], 0
    for l in lens.tolist():
        words.append("".join(flat[at:at + l]))
        at += l
    zipf = np.minimum(rs.zipf(1.3, size=6_000_000) - 1, len(words) - 1)
    base = " ".join(words[i] for i in zipf.tolist())
    size = rs.randint(200, 2001, size=n)
    start = rs.randint(0, len(base) - 2001, size=n)
    upper = np.array(list("ABCDEFGHIJKLMNOPQRSTUVWXYZ"))
    marks = {(kind, L): "".join(rs.choice(upper, size=L)) for kind in ("rare", "common") for L in (3, 8, 64)}
    assert len(set(marks.values())) == len(marks) and not any(a in b for a in marks.values() for b in marks.values() if a != b)
    u = rs.rand(n)
    member = {"rare": u < 0.001, "common": (u >= 0.25) & (u < 0.75)}
    shift = rs.randint(0, 21, size=n)
    texts = []
    for r in range(n):
        t = base[start[r]:start[r] + size[r]]
        for kind in ("rare", "common"):
            if member[kind][r]:                               # (no row is in both sets; the three markers sit in slots that cannot overlap)
                for slot, L in ((0, 3), (30, 8), (60, 64)):
                    a = slot + int(shift[r])
                    t = t[:a] + marks[(kind, L)] + t[a + L:]
        texts.append(t)
    natural = [w for w in dict.fromkeys(words[i] for i in zipf[:200000].tolist()) if 3 <= len(w) <= 12]
    return texts, marks, member, natural


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
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "calls": calls}


def wall_times(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "where_document_bench.json"))
    args = ap.parse_args()
    n = args.rows
    t0 = time.perf_counter()
    texts, marks, member, natural = make_corpus(n, 0)
    print(f"corpus: {n} chunks in {time.perf_counter() - t0:.1f} s", flush=True)
    t0 = time.perf_counter()
    store = DocumentStore(texts, device="cuda:0")
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    gb = store.n_bytes / 1e9
    floor_ms = store.n_bytes / COPY_RATE * 1e3
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "blob_GB": gb, "document_store_load_s": load_s,
           "floor": {"what": "blob bytes / 6.29 TB/s (the chip's measured copy rate)", "ms": floor_ms}, "scan": [], "query": []}
    print(f"blob {gb:.3f} GB uploaded in {load_s:.1f} s; floor {floor_ms:.3f} ms", flush=True)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream

    arms = [(f"1 {kind} pattern, {L} bytes", [marks[(kind, L)]]) for kind in ("rare", "common") for L in (3, 8, 64)]
    arms += [("8 patterns (words of the text, 3-12 bytes)", natural[40:48]), ("32 patterns (words of the text, 3-12 bytes)", natural[40:72]),
             ("32 patterns (absent: upper-case, 8 bytes)", ["".join(chr(65 + (7 * i + j) % 26) for j in range(8)) + "Q" for i in range(32)])]
    for name, pats in arms:
        pb, po = pack_patterns(pats)
        d_pb, d_po = torch.from_numpy(pb.copy()).cuda(), torch.from_numpy(po).cuda()
        bits = torch.empty((len(pats), store.n_words), dtype=torch.int64, device="cuda")

        def scan():
            _lib.check(lib.arx_text_contains(store.blob.data_ptr(), store.row_off.data_ptr(), n, d_pb.data_ptr(), d_po.data_ptr(), len(pats),
                                             bits.data_ptr(), st), "arx_text_contains")
        t = event_times(scan, args.calls)
        matched = [store.count(bits[i].contiguous()) for i in range(len(pats))]
        tree = compile_where_document({"$or": [{"$contains": p} for p in pats]})
        h0 = time.perf_counter()
        per_pat = [evaluate_host(("contains", p), texts) for p in pats]
        host_ms = (time.perf_counter() - h0) * 1e3
        assert [int(m.sum()) for m in per_pat] == matched, (name, "device and host disagree")
        words, n_allowed = store.allow(tree)
        row = {"arm": name, "patterns": len(pats), "pattern_bytes": sorted({len(p) for p in pats}), "rows_matched": matched if len(pats) <= 8 else None,
               "rows_matched_any": n_allowed, **t, "GB_per_s": gb / (t["ms_median"] * 1e-3), "floor_ms": floor_ms,
               "times_the_floor": t["ms_median"] / floor_ms, "evaluate_host_ms": host_ms, "host_over_device": host_ms / t["ms_median"]}
        out["scan"].append(row)
        print(json.dumps(row), flush=True)

    # ---- whole queries ----
    coll = HipCollection.__new__(HipCollection)
    rows = fill_unit_rows(n, args.dim, 1)
    coll.n_total, coll.dim, coll.lo, coll.hi = n, args.dim, 0, n
    coll.metadata = [{"chunk_id": f"c{r}", "text": t, "rare": bool(member["rare"][r]), "common": bool(member["common"][r])} for r, t in enumerate(texts)]
    coll._where_columns, coll.encoder, coll.keyword, coll.documents = {}, None, None, store
    coll.index = ShardIndex(rows, idx_base=0, prefilter="int8", adaptive=True)
    for nq in (64, 1):
        q = fill_unit_rows(nq, args.dim, 2).cpu().numpy()
        base = wall_times(lambda: coll.query(query_embeddings=q, n_results=10), args.calls)
        out["query"].append({"queries": nq, "arm": "unfiltered", **base})
        print(json.dumps(out["query"][-1]), flush=True)
        for kind in ("common", "rare"):
            f = {"$contains": marks[(kind, 8)]}
            a = coll.query(query_embeddings=q, n_results=10, where={kind: True})
            b = coll.query(query_embeddings=q, n_results=10, where_document=f)
            assert a["indices"] == b["indices"] and a["scores"] == b["scores"], "where and where_document disagree on the same rows"
            tw = wall_times(lambda: coll.query(query_embeddings=q, n_results=10, where={kind: True}), args.calls)
            td = wall_times(lambda: coll.query(query_embeddings=q, n_results=10, where_document=f), args.calls)
            for arm, t in ((f"where={{'{kind}': True}} (host-evaluated mask, columns cached)", tw), (f"where_document $contains the {kind} 8-byte marker", td)):
                out["query"].append({"queries": nq, "arm": arm, "allowed_rows": int(member[kind].sum()), **t,
                                     "ratio_to_unfiltered": t["ms_median"] / base["ms_median"]})
                print(json.dumps(out["query"][-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
