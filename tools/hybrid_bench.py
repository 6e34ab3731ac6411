"""Cost of the keyword side of hybrid search beside the cosine search it accompanies, on one GPU.

Synthetic corpus, generated on the device from a seed (no file): --docs documents of --doc-len word pieces drawn from a Zipf
distribution over a 30 522-word vocabulary; 64-query batches of 8-16 distinct terms drawn from the same distribution.  Measured, in ONE
run: device time of `arx_bm25_search` (n = 32) per batch, the posting bytes its terms cover (8 bytes per posting, read once: the
kernel's streaming work) and the GB/s that gives; and `ShardIndex.search` (k = 32) for the same number of rows and the same batch at
D = 768 (fp16 rows and the int8 pre-filter).  Device time from events on the stream, median of --reps after warm-up; the timed region
holds no host work (the query terms are uploaded before).  Prints one JSON line.

    python tools/hybrid_bench.py [--docs 1000000] [--reps 20] [--out profiles/hybrid_bench.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from arxiv_rag_amd import _lib  # noqa: E402
from arxiv_rag_amd.index import ShardIndex, fill_unit_rows  # noqa: E402
from arxiv_rag_amd.keyword import KeywordIndex, pack_query_terms  # noqa: E402

VOCAB = 30522


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def zipf_postings(n_docs, doc_len, seed, chunk=200000):
    """(term_ptr, rows, tf, dl) of a seeded Zipf corpus; sampling, sorting and counting run on the device."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    p = 1.0 / torch.arange(1, VOCAB + 1, dtype=torch.float64, device="cuda") ** 1.07
    perm = torch.randperm(VOCAB, generator=g, device="cuda")
    cdf = torch.cumsum(p / p.sum(), 0)
    keys, cnts = [], []
    for lo in range(0, n_docs, chunk):
        m = min(chunk, n_docs - lo)
        u = torch.rand((m, doc_len), dtype=torch.float64, device="cuda", generator=g)
        t = perm[torch.searchsorted(cdf, u).clamp_(max=VOCAB - 1)]                                          # [m, doc_len], inverse-CDF sampling
        key = (t * n_docs + torch.arange(lo, lo + m, device="cuda")[:, None]).reshape(-1)
        k, c = torch.unique(key, return_counts=True)
        keys.append(k); cnts.append(c)
    key = torch.cat(keys); cnt = torch.cat(cnts)
    key, order = torch.sort(key)                                  # (term, row): chunks hold disjoint rows, so the keys are distinct
    cnt = cnt[order]
    term = key // n_docs
    term_ptr = torch.zeros(VOCAB + 1, dtype=torch.int64, device="cuda")
    term_ptr[1:] = torch.cumsum(torch.bincount(term, minlength=VOCAB), 0)
    return (term_ptr.cpu().numpy(), (key % n_docs).cpu().numpy().astype(np.uint32), cnt.cpu().numpy().astype(np.int32),
            np.full(n_docs, doc_len, np.int64), p.cpu().numpy(), perm.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--doc-len", type=int, default=160)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hybrid_bench needs a GPU"
    lib = _lib.load()
    term_ptr, rows, tf, dl, p, perm = zipf_postings(args.docs, args.doc_len, seed=0)
    kw = KeywordIndex.from_postings(term_ptr, rows, tf, dl)
    del rows, tf
    torch.cuda.empty_cache()
    rs = np.random.RandomState(1)
    pz = p / p.sum()
    nq, n = 64, 32
    res = {"device": torch.cuda.get_device_name(0), "docs": args.docs, "doc_len": args.doc_len, "vocab": VOCAB, "postings": int(kw.n_postings),
           "index_bytes": int(kw.n_postings) * 8 + (VOCAB + 1) * 8, "queries_per_batch": nq, "n": n, "reps": args.reps,
           "timing": "hipEvents on the stream, median of reps after 3 warm-up calls; clocks as the machine runs them (not pinned)"}
    out_s = torch.empty((nq, n), dtype=torch.float32, device="cuda"); out_i = torch.empty((nq, n), dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.arx_bm25_workspace_bytes(kw.n_rows, nq, n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    batches = []
    for b in range(args.batches):
        tl = [sorted(set(perm[rs.choice(VOCAB, size=rs.randint(8, 17), p=pz)].tolist())) for _ in range(nq)]
        qt, qn = pack_query_terms(tl, VOCAB)
        qt_d, qn_d = torch.from_numpy(qt).cuda(), torch.from_numpy(qn).cuda()
        nbytes = kw.posting_bytes(tl)

        def call():
            _lib.check(lib.arx_bm25_search(kw.term_ptr.data_ptr(), kw.post_row.data_ptr(), kw.post_w.data_ptr(), VOCAB, kw.n_rows,
                                           qt_d.data_ptr(), qn_d.data_ptr(), nq, n, out_s.data_ptr(), out_i.data_ptr(), 0, ws.data_ptr(),
                                           ws.numel(), st), "arx_bm25_search")
        med, lo, hi = timed(call, args.reps)
        batches.append({"terms_per_query_mean": float(np.mean([len(t) for t in tl])), "posting_bytes_per_query_mean": float(nbytes.mean()),
                        "posting_bytes_per_query_max": int(nbytes.max()), "posting_bytes_batch": int(nbytes.sum()),
                        "ms_per_batch": med, "ms_min": lo, "ms_max": hi, "gb_per_s": float(nbytes.sum()) / (med * 1e-3) / 1e9,
                        "hits_per_query_mean": float((out_i >= 0).sum().item()) / nq})
    res["bm25_batches"] = batches
    res["bm25_ms_per_batch"] = float(np.median([b["ms_per_batch"] for b in batches]))
    res["bm25_gb_per_s"] = float(np.median([b["gb_per_s"] for b in batches]))
    res["posting_bytes_per_query"] = float(np.mean([b["posting_bytes_per_query_mean"] for b in batches]))
    # the dense search the keyword side accompanies: same rows, same batch, D = 768, k = 32
    D = 768
    corpus = fill_unit_rows(args.docs, D, seed=3)
    Q = fill_unit_rows(nq, D, seed=4)
    for name, pre in (("dense_fp16", None), ("dense_int8_prefilter", "int8")):
        ix = ShardIndex(corpus, prefilter=pre)
        med, lo, hi = timed(lambda: ix.search(Q, n), args.reps)
        res[name + "_ms_per_batch"] = med
        res[name + "_ms_min_max"] = [lo, hi]
        del ix
    res["bm25_over_dense_fp16"] = res["bm25_ms_per_batch"] / res["dense_fp16_ms_per_batch"]
    res["bm25_over_dense_int8_prefilter"] = res["bm25_ms_per_batch"] / res["dense_int8_prefilter_ms_per_batch"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
