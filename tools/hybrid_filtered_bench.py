"""Cost of the row filter in the BM25 keyword search (`arx_bm25_search_filtered`) beside the unfiltered `arx_bm25_search`, on one GPU.

Synthetic corpus of tools/hybrid_bench.py (--docs documents of --doc-len word pieces, Zipf over a 30 522-word vocabulary, generated on
the device from a seed); a 64-query batch and a single query of 8-16 distinct terms, n = 32.  Arms, all in ONE process and timed IN
TURN (every round runs each arm once, so drift of the clocks or of the shared machine falls on all of them alike): the unfiltered call
(the baseline), an all-rows mask, a contiguous 12.5 % mask, random 50 % / 1 % / 0.1 % masks, and 64 distinct random-1 % filters in one
call against the same 64 queries as 64 single-filter calls.  Device time from events on the stream, median of --reps rounds after 3
warm-up rounds; every arm is reported in ms and as a ratio to the unfiltered call of the same run.  No figure is fixed in advance.

Also recorded: a whole `HipCollection.query(where=..., hybrid_alpha=0.7)` (host clock, the call returns host lists) against the same
query without `where`, on a collection of --collection-docs short synthetic texts built with `hybrid_filters=True`.

    python tools/hybrid_filtered_bench.py [--docs 1000000] [--reps 20] [--out profiles/hybrid_filtered_bench.json]
"""
import argparse
import dataclasses
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
from arxiv_rag_amd.keyword import KeywordIndex, pack_query_terms  # noqa: E402
from arxiv_rag_amd.where import pack_bitmap  # noqa: E402
from hybrid_bench import VOCAB, zipf_postings  # noqa: E402


def timed_in_turn(arms, reps, warmup=3):
    """arms: {name: callable} -> {name: (median, min, max) ms}; one call of every arm per round."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (float(np.median(t)), float(np.min(t)), float(np.max(t))) for name, t in ts.items()}


def device_words(masks):
    return torch.from_numpy(np.stack([pack_bitmap(m) for m in masks]).view(np.int64)).cuda()


def kernel_arms(args, res):
    lib = _lib.load()
    term_ptr, rows, tf, dl, p, perm = zipf_postings(args.docs, args.doc_len, seed=0)
    kw = KeywordIndex.from_postings(term_ptr, rows, tf, dl)
    del rows, tf
    torch.cuda.empty_cache()
    N, n = kw.n_rows, 32
    rs = np.random.RandomState(1)
    pz = p / p.sum()
    res.update(postings=int(kw.n_postings), index_bytes=int(kw.n_postings) * 8 + (VOCAB + 1) * 8, bitmap_bytes=(N + 63) // 64 * 8)
    r = np.arange(N)
    masks = {"all_rows": np.ones(N, bool), "contiguous_12.5pct": (r >= N // 2) & (r < N // 2 + N // 8), "random_50pct": rs.rand(N) < 0.5,
             "random_1pct": rs.rand(N) < 0.01, "random_0.1pct": rs.rand(N) < 0.001}
    single = {name: device_words([m]) for name, m in masks.items()}
    many = device_words([rs.rand(N) < 0.01 for _ in range(64)])
    st = torch.cuda.current_stream().cuda_stream
    for nq in (64, 1):
        tl = [sorted(set(perm[rs.choice(VOCAB, size=rs.randint(8, 17), p=pz)].tolist())) for _ in range(nq)]
        qt, qn = pack_query_terms(tl, VOCAB)
        qt_d, qn_d = torch.from_numpy(qt).cuda(), torch.from_numpy(qn).cuda()
        out_s = torch.empty((nq, n), dtype=torch.float32, device="cuda"); out_i = torch.empty((nq, n), dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.arx_bm25_workspace_bytes(N, nq, n), dtype=torch.uint8, device="cuda")
        each = torch.arange(nq, dtype=torch.int32, device="cuda")
        head = (kw.term_ptr.data_ptr(), kw.post_row.data_ptr(), kw.post_w.data_ptr(), VOCAB, N)

        def unfiltered():
            _lib.check(lib.arx_bm25_search(*head, qt_d.data_ptr(), qn_d.data_ptr(), nq, n, out_s.data_ptr(), out_i.data_ptr(), 0, ws.data_ptr(),
                                           ws.numel(), st), "arx_bm25_search")

        def filtered(allow, n_filters, filter_of, first=0, count=nq):
            def call():
                _lib.check(lib.arx_bm25_search_filtered(*head, allow.data_ptr(), n_filters, None if filter_of is None else filter_of.data_ptr(),
                                                        qt_d[first:].data_ptr(), qn_d[first:].data_ptr(), count, n, out_s[first:].data_ptr(),
                                                        out_i[first:].data_ptr(), 0, ws.data_ptr(), ws.numel(), st), "arx_bm25_search_filtered")
            return call

        arms = {"unfiltered": unfiltered}
        for name in masks:
            arms[name] = filtered(single[name], 1, None)
        if nq == 64:
            arms["64_filters_one_call"] = filtered(many, 64, each)
            singles = [filtered(many[j], 1, None, first=j, count=1) for j in range(64)]
            arms["64_filters_64_calls"] = lambda: [fn() for fn in singles]
        t = timed_in_turn(arms, args.reps)
        base = t["unfiltered"][0]
        res[f"queries_{nq}"] = {"terms_per_query_mean": float(np.mean([len(x) for x in tl])),
                                "posting_bytes_batch": int(kw.posting_bytes(tl).sum()),
                                "arms": {name: {"ms": v[0], "ms_min": v[1], "ms_max": v[2], "ratio_to_unfiltered": v[0] / base} for name, v in t.items()}}
        # the timed calls computed what they should: the all-rows mask gives the unfiltered answer
        unfiltered(); a = (out_s.clone(), out_i.clone())
        arms["all_rows"](); torch.cuda.synchronize()
        assert torch.equal(a[0], out_s) and torch.equal(a[1], out_i), "the all-rows mask must reproduce the unfiltered search"
    del kw
    torch.cuda.empty_cache()


def collection_arm(args, res):
    from arxiv_rag_amd import config as C
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from arxiv_rag_amd.index import fill_unit_rows
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=VOCAB, max_seq_length=64)
    rs = np.random.RandomState(2)
    letters = "abcdefghijklmnopqrstuvwxyz"
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(letters)
    seen = set(toks)
    while len(toks) < VOCAB:
        w = "".join(rs.choice(list(letters), size=rs.randint(3, 8)))
        if w not in seen:
            seen.add(w); toks.append(w)
    tok = WordPieceTokenizer.from_vocab({t: i for i, t in enumerate(toks)}, cfg)
    words = np.array(toks[30:])
    N, D, nq = args.collection_docs, 384, 64
    pz = 1.0 / np.arange(1, len(words) + 1) ** 1.07
    pz /= pz.sum()
    draw = rs.choice(len(words), size=(N, 24), p=pz)
    texts = [" ".join(words[row]) for row in draw]
    meta = [{"chunk_id": f"c{j}", "text": t, "year": int(2000 + j % 25)} for j, t in enumerate(texts)]
    emb = fill_unit_rows(N, D, seed=3).cpu().numpy()
    Q = fill_unit_rows(nq, D, seed=4).cpu().numpy()
    qs = [" ".join(words[rs.choice(len(words), size=10, p=pz)]) for _ in range(nq)]
    col = HipCollection(emb, meta, keyword=True, tokenizer=tok, hybrid_filters=True)
    where = {"year": {"$gte": 2022}}                           # 12 % of the rows, scattered

    def wall(fn, reps):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    reps = max(3, args.reps // 4)
    calls = {"hybrid": lambda: col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=0.7),
             "hybrid_where": lambda: col.query(query_embeddings=Q, query_texts=qs, n_results=10, hybrid_alpha=0.7, where=where),
             "dense_where": lambda: col.query(query_embeddings=Q, n_results=10, where=where)}
    t = {name: wall(fn, reps) for name, fn in calls.items()}
    res["collection_query"] = {"docs": N, "dim": D, "queries": nq, "where": where, "reps": reps, "clock": "host, around the whole call",
                               "ms": t, "hybrid_where_over_hybrid": t["hybrid_where"] / t["hybrid"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--doc-len", type=int, default=160)
    ap.add_argument("--collection-docs", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hybrid_filtered_bench needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "docs": args.docs, "doc_len": args.doc_len, "vocab": VOCAB, "n": 32, "reps": args.reps,
           "timing": "hipEvents on the stream, median of reps rounds after 3 warm-up rounds, every arm once per round; clocks as the machine "
                     "runs them (not pinned)"}
    kernel_arms(args, res)
    if args.collection_docs > 0:
        collection_arm(args, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
