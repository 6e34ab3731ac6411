"""Cost of hybrid search on the device (`hybrid_on_device`) beside the default path, on one GPU.

The workload of tools/hybrid_bench.py: a seeded synthetic corpus of --docs documents of --doc-len word pieces (Zipf over a 30 522-word
vocabulary), queries of 8-16 distinct terms.  Every arm of a comparison runs once per round, in turn, in ONE process; the figure is the
median of --reps rounds after 3 warm-up rounds; before anything is timed the outputs of the two paths are compared bit for bit.

1. the default path against the new one, at Q = 1 and Q = 64, n = 32 per side, k = 32 (host clock around work that ends with the four
   result arrays on the host, as `retrieval.retrieve` leaves them; the dense list is given, on the device, in both arms):
     host:    KeywordIndex.search -> both lists .cpu() -> keyword.fuse
     device:  KeywordIndex.search_wide -> keyword.fuse_device -> four arrays .cpu()
2. the cost of width: arx_bm25_search_wide at n = 32 / 50 / 256 / 1024 against arx_bm25_search at n = 32 (device time from events,
   query terms uploaded before)
3. arx_hybrid_fuse alone at (n_dense, n_kw) = (32, 32), (50, 50), (1024, 1024), k = n_dense (device time from events)
Prints one JSON line.

    python tools/hybrid_device_bench.py [--docs 1000000] [--reps 20] [--out profiles/hybrid_device_bench.json]
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
sys.path.insert(0, str(ROOT / "tools"))

from arxiv_rag_amd import _lib  # noqa: E402
from arxiv_rag_amd.keyword import KeywordIndex, fuse, fuse_device, pack_query_terms  # noqa: E402
from hybrid_bench import VOCAB, zipf_postings  # noqa: E402


def rounds(arms, reps, device_time):
    """arms: {name: fn}.  Every arm once per round, in turn -> {name: [median, min, max] ms}."""
    ts = {k: [] for k in arms}
    for r in range(reps + 3):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            if device_time:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                b.synchronize()
                t = a.elapsed_time(b)
            else:
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
            if r >= 3:
                ts[name].append(t)
    return {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ts.items()}


def dense_lists(nq, n, n_rows, seed):
    """A dense candidate list per query as a cosine search leaves it: distinct rows, scores descending; on the device."""
    rs = np.random.RandomState(seed)
    s = -np.sort(-rs.uniform(0.2, 0.9, size=(nq, n)).astype(np.float32), axis=1)
    i = np.stack([rs.choice(n_rows, size=n, replace=False) for _ in range(nq)]).astype(np.int64)
    return torch.from_numpy(s).cuda(), torch.from_numpy(i).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--doc-len", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hybrid_device_bench needs a GPU"
    lib = _lib.load()
    term_ptr, rows, tf, dl, p, perm = zipf_postings(args.docs, args.doc_len, seed=0)
    kw = KeywordIndex.from_postings(term_ptr, rows, tf, dl)
    del rows, tf
    torch.cuda.empty_cache()
    rs = np.random.RandomState(1)
    pz = p / p.sum()
    queries = [sorted(set(perm[rs.choice(VOCAB, size=rs.randint(8, 17), p=pz)].tolist())) for _ in range(64)]
    res = {"device": torch.cuda.get_device_name(0), "docs": args.docs, "doc_len": args.doc_len, "vocab": VOCAB, "postings": int(kw.n_postings),
           "reps": args.reps, "timing": "every arm of a comparison once per round, in turn, one process; [median, min, max] ms of reps rounds "
           "after 3 warm-up rounds; clocks as the machine runs them (not pinned)"}
    st = torch.cuda.current_stream().cuda_stream
    # 1 ------------------------------------------------------------------------------------------------------------------------------
    alpha, n = 0.7, 32
    for nq in (1, 64):
        tl = queries[:nq]
        ds, di = dense_lists(nq, n, kw.n_rows, seed=nq)
        ki0 = kw.search(tl, n)[1].cpu().numpy()
        di_h = kw.n_rows + di.cpu().numpy()                      # ids beyond the keyword side's rows: distinct, no chance overlap ...
        third = np.arange(n) % 3 == 0                            # ... and every third slot a row of the keyword list, as a real query has
        di_h[:, third] = np.where(ki0[:, third] >= 0, ki0[:, third], di_h[:, third])
        di = torch.from_numpy(di_h).cuda()

        def host_path():
            ks, ki = kw.search(tl, n)
            return fuse(ds.cpu().numpy(), di.cpu().numpy(), ks.cpu().numpy(), ki.cpu().numpy(), alpha, n)

        def device_path():
            ks, ki = kw.search_wide(tl, n)
            return tuple(t.cpu().numpy() for t in fuse_device(ds, di, ks, ki, alpha, n))
        a, b = host_path(), device_path()
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and np.array_equal(a[0].view(np.int64), b[0].view(np.int64))
        res[f"pipeline_q{nq}_ms"] = rounds({"host_search_copy_fuse": host_path, "device_search_wide_fuse_device": device_path}, args.reps, False)
        r = res[f"pipeline_q{nq}_ms"]
        res[f"pipeline_q{nq}_device_over_host"] = r["device_search_wide_fuse_device"][0] / r["host_search_copy_fuse"][0]
    # 2 ------------------------------------------------------------------------------------------------------------------------------
    for nq in (1, 64):
        qt, qn = pack_query_terms(queries[:nq], VOCAB)
        qt_d, qn_d = torch.from_numpy(qt).cuda(), torch.from_numpy(qn).cuda()
        out_s = torch.empty((nq, 1024), dtype=torch.float32, device="cuda"); out_i = torch.empty((nq, 1024), dtype=torch.int64, device="cuda")
        ws = torch.empty(max(lib.arx_bm25_workspace_bytes(kw.n_rows, nq, 32), lib.arx_bm25_wide_workspace_bytes(kw.n_rows, nq, 1024),
                             lib.arx_bm25_wide_workspace_bytes(kw.n_rows, nq, 32)), dtype=torch.uint8, device="cuda")
        head = (kw.term_ptr.data_ptr(), kw.post_row.data_ptr(), kw.post_w.data_ptr(), VOCAB, kw.n_rows)

        def narrow():
            _lib.check(lib.arx_bm25_search(*head, qt_d.data_ptr(), qn_d.data_ptr(), nq, 32, out_s.data_ptr(), out_i.data_ptr(), 0, ws.data_ptr(),
                                           ws.numel(), st), "arx_bm25_search")

        def wide(n):
            return lambda: _lib.check(lib.arx_bm25_search_wide(*head, None, 0, None, qt_d.data_ptr(), qn_d.data_ptr(), nq, n, out_s.data_ptr(),
                                                               out_i.data_ptr(), 0, ws.data_ptr(), ws.numel(), 0, 0, st), "arx_bm25_search_wide")
        arms = {"arx_bm25_search_n32": narrow, **{f"arx_bm25_search_wide_n{n}": wide(n) for n in (32, 50, 256, 1024)}}
        r = res[f"width_q{nq}_ms"] = rounds(arms, args.reps, True)
        res[f"width_q{nq}_over_search_n32"] = {k: v[0] / r["arx_bm25_search_n32"][0] for k, v in r.items()}
    # 3 ------------------------------------------------------------------------------------------------------------------------------
    for nq in (1, 64):
        arms = {}
        for n in (32, 50, 1024):
            ds, di = dense_lists(nq, n, 4 * n, seed=n)
            ks, ki = dense_lists(nq, n, 4 * n, seed=n + 1)
            arms[f"arx_hybrid_fuse_{n}_{n}_k{n}"] = (lambda a: lambda: fuse_device(*a, alpha, a[0].shape[1]))((ds, di, ks, ki))
        res[f"fuse_q{nq}_ms"] = rounds(arms, args.reps, True)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
