"""Building the BM25 keyword index: the host build (the default) beside the device build (`build_on_device`), on one GPU.

Corpus: --docs documents of 100-220 word pieces each, Zipf-distributed over a 30 522-word vocabulary in a seeded random order (1 M
documents = about 160 M pieces).  Both builds run in turn in ONE process, one of each per round; the figure is the median of --reps
rounds after one warm-up round; before anything is timed the two indexes are compared bit for bit.

  host:    keyword.build_postings (word-piece lists -> one np.unique) + keyword.impacts_f64 + the three uploads        (host clock)
  device:  keyword.build_postings_device (upload of the flat pieces and doc_ptr, arx_bm25_build_postings, the reads of the flag, P and
           term_ptr) + keyword.build_impacts_device (idf on the host, arx_bm25_build_impacts)                             (host clock)
and, from events around the two library calls alone (inputs uploaded before): their device times, beside the floor: the bytes the
passes of csrc/bm25_build.hip must move at the 6.29 TB/s copy rate the other benches use.  `flatten_ms` is the part of the host build
that walks the Python lists (`np.fromiter` over a generator), measured alone, for a caller who already holds flat arrays.
With --texts FILE (one text per line) and --tokenizer DIR it also times `full_pieces_flat` against `_full_pieces` on up to 100 000 texts.
Prints one JSON line.

    python tools/keyword_build_bench.py [--docs 1000000] [--reps 5] [--out profiles/keyword_build_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import keyword as KW  # noqa: E402

VOCAB = 30522
COPY_RATE = 6.29e12            # bytes / s


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def corpus(n_docs, seed):
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(p / p.sum())
    perm = rs.permutation(VOCAB).astype(np.int32)
    dl = rs.randint(100, 221, size=n_docs).astype(np.int64)
    doc_ptr = np.zeros(n_docs + 1, np.int64)
    np.cumsum(dl, out=doc_ptr[1:])
    flat = np.empty(int(doc_ptr[-1]), np.int32)
    for a in range(0, len(flat), 1 << 24):
        b = min(len(flat), a + (1 << 24))
        flat[a:b] = perm[np.minimum(np.searchsorted(cdf, rs.rand(b - a)), VOCAB - 1)]
    return flat, doc_ptr


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(v):
    return [float(np.median(v)), float(np.min(v)), float(np.max(v))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--texts", type=str, default=None)
    ap.add_argument("--tokenizer", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "keyword_build_bench needs a GPU"
    dev = "cuda:0"
    flat, doc_ptr = corpus(args.docs, 0)
    T, n = len(flat), args.docs
    say(f"corpus: {n} documents, {T} pieces")
    lists = [a.tolist() for a in np.split(flat, doc_ptr[1:-1])]
    say("lists ready")

    def host_build():
        t = {}
        t0 = time.perf_counter()
        term_ptr, rows, tf, dl = KW.build_postings(lists, VOCAB)
        t["build_postings_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        w = KW.impacts_f64(term_ptr, rows, tf, dl, KW.KeywordStats.from_postings(term_ptr, dl)).astype(np.float32)
        t["impacts_f64_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        d = (torch.from_numpy(term_ptr).to(dev), torch.from_numpy(rows.view(np.int32)).to(dev), torch.from_numpy(w).to(dev))
        torch.cuda.synchronize()
        t["upload_ms"] = (time.perf_counter() - t0) * 1e3
        return t, d, (term_ptr, dl)

    def device_build():
        t = {}
        t["build_postings_device_ms"], built = clock(lambda: KW.build_postings_device(flat, doc_ptr, VOCAB, dev))
        stats = KW.KeywordStats.from_postings(built.term_ptr_host, built.dl)
        t["build_impacts_device_ms"], w = clock(lambda: KW.build_impacts_device(built, stats))
        return t, (built.term_ptr, built.post_row, w), built

    # the same index, bit for bit (this is the warm-up round too)
    _, hd, (term_ptr_h, dl_h) = host_build()
    say("host build done")
    _, dd, built = device_build()
    P = built.n_postings
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(hd, dd)), "the device build differs from the host build"
    say(f"device build equals the host build: {P} postings")
    del hd, dd
    torch.cuda.empty_cache()
    host, device = [], []
    for r in range(args.reps):
        t, d, _ = host_build()
        host.append(t)
        del d
        t, d, built = device_build()
        device.append(t)
        del d
        torch.cuda.empty_cache()
        say(f"round {r}: host {sum(host[-1].values()):.0f} ms, device {sum(device[-1].values()):.1f} ms")
    t0 = time.perf_counter()
    np.fromiter((t for p in lists for t in p), np.int64, T)
    flatten_ms = (time.perf_counter() - t0) * 1e3
    del lists

    # the two library calls alone, device time
    pieces_d, doc_ptr_d = torch.from_numpy(flat).to(dev), torch.from_numpy(doc_ptr).to(dev)
    out = [torch.empty(VOCAB + 1, dtype=torch.int64, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
           torch.empty(T, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)]
    stats = KW.KeywordStats.from_postings(term_ptr_h, dl_h)
    calls = {"arx_bm25_build_postings": lambda: KW.build_postings_raw(pieces_d, doc_ptr_d, T, n, VOCAB, *out),
             "arx_bm25_build_impacts": lambda: KW.build_impacts_device(built, stats)}
    dev_ms = {}
    for name, fn in calls.items():
        ts = []
        for r in range(args.reps + 1):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            if r:
                ts.append(a.elapsed_time(b))
        dev_ms[name] = stat(ts)
    passes = 2                                                   # ceil(bits(VOCAB - 1) / 8)
    post_bytes = (12 * T) + passes * (4 * T + 16 * T) + 8 * T + (8 * T + 4 * T + 4 * P) + (12 * P + 8 * P) + 8 * (VOCAB + 1)
    imp_bytes = 8 * P + 4 * P + 8 * (VOCAB + 1) + 8 * (n + 1) + 8 * VOCAB
    res = {"device": torch.cuda.get_device_name(0), "docs": n, "pieces": T, "vocab": VOCAB, "postings": P, "reps": args.reps,
           "timing": "one host build and one device build per round, in turn, one process; [median, min, max] ms of reps rounds after one warm-up "
                     "round; the two indexes compared bit for bit first",
           "host": {k: stat([t[k] for t in host]) for k in host[0]}, "host_total_ms": stat([sum(t.values()) for t in host]),
           "host_flatten_ms_once": flatten_ms,
           "device_path": {k: stat([t[k] for t in device]) for k in device[0]}, "device_path_total_ms": stat([sum(t.values()) for t in device]),
           "device_time_ms": dev_ms,
           "floor_ms": {"arx_bm25_build_postings": post_bytes / COPY_RATE * 1e3, "arx_bm25_build_impacts": imp_bytes / COPY_RATE * 1e3},
           "floor": "bytes the passes must move (init 12 T; each of 2 radix passes 4 T counted + 16 T scattered; heads 8 T counted, 12 T + 4 P "
                    "numbered; 20 P emitted; impacts 12 P and the tables) at 6.29 TB/s",
           "tokenizer": None}
    res["ratio_device_to_host"] = res["device_path_total_ms"][0] / res["host_total_ms"][0]
    if args.texts and args.tokenizer:
        from arxiv_rag_amd.hub import load_sentence_encoder
        tok = load_sentence_encoder(args.tokenizer).tokenizer
        texts = [l.rstrip("\n") for l in open(args.texts, encoding="utf-8")][:100000]
        a, b = [], []
        for r in range(args.reps):
            t0 = time.perf_counter(); ref = tok._full_pieces(texts); a.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); got = tok.full_pieces_flat(texts); b.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got[0], KW.flatten_pieces(ref)[0])
        res["tokenizer"] = {"texts": len(texts), "pieces": int(len(got[0])), "_full_pieces_ms": stat(a), "full_pieces_flat_ms": stat(b)}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
