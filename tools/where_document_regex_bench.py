#!/usr/bin/env python
"""Times the `where_document` regular-expression scan (`arx_text_regex`) beside the substring scan (`arx_text_contains`).

One process, one GPU, the corpus of tools/where_document_bench.py (`--rows`, 1 M synthetic chunks of 200-2000 characters with its
upper-case markers).  Arms, timed in turn, to profiles/where_document_regex_bench.json; each is one launch per call with its tables or
patterns already on the device, 3 warm-up calls, then the median (and minimum) of `--calls` (20) calls, each between its own pair of
events on the stream:
* a literal regex (the common 8-byte marker) and `$contains` of the same string, with their ratio: whether the byte-at-a-time table
  walk or HBM paces the scan;
* `(?i)` of that marker in lower case;
* an alternation of 8 words of the text and the 8-substring `$or` (one `arx_text_contains` launch), with their ratio;
* `\\d{4}\\.\\d{4,5}` and `[A-Z][a-z]+ et al\\.` (neither occurs: every row is walked to its end);
* a 256-state pattern;
* the 8 regexes above and one more in one call.
Beside each arm: the floor (blob bytes at the chip's measured 6.29 TB/s copy rate), the rows matched, and a Python `re` loop over the
same texts in this process (wall clock, one run over the first `--re-rows` texts, all of them by default), whose count must agree.
Run it under a time limit (e.g. `timeout -k 10 840 python tools/where_document_regex_bench.py`)."""
import argparse
import json
import re
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from arxiv_rag_amd import _lib                                                   # noqa: E402
from arxiv_rag_amd.regex_dfa import pack_tables                                   # noqa: E402
from arxiv_rag_amd.where_document import DocumentStore, compiled_regex, pack_patterns      # noqa: E402
from where_document_bench import COPY_RATE, event_times, make_corpus              # noqa: E402

STATES_256 = "a[ab]{6}c|d[de]{6}f"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--re-rows", type=int, default=0, help="texts the Python re loop reads (0 = all)")
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "where_document_regex_bench.json"))
    args = ap.parse_args()
    n = args.rows
    re_rows = n if args.re_rows <= 0 else min(n, args.re_rows)
    t0 = time.perf_counter()
    texts, marks, member, natural = make_corpus(n, 0)
    print(f"corpus: {n} chunks in {time.perf_counter() - t0:.1f} s", flush=True)
    store = DocumentStore(texts, device="cuda:0")
    torch.cuda.synchronize()
    gb = store.n_bytes / 1e9
    floor_ms = store.n_bytes / COPY_RATE * 1e3
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "blob_GB": gb, "re_rows": re_rows,
           "floor": {"what": "blob bytes / 6.29 TB/s (the chip's measured copy rate)", "ms": floor_ms}, "arms": []}
    print(f"blob {gb:.3f} GB; floor {floor_ms:.3f} ms", flush=True)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    marker, words = marks[("common", 8)], natural[40:48]

    def time_regexes(patterns):
        dfas = [compiled_regex(p) for p in patterns]
        tb, to = pack_tables(dfas)
        d_tb, d_to = torch.from_numpy(tb).cuda(), torch.from_numpy(to).cuda()
        bits = torch.empty((len(patterns), store.n_words), dtype=torch.int64, device="cuda")

        def scan():
            _lib.check(lib.arx_text_regex(store.blob.data_ptr(), store.row_off.data_ptr(), n, d_tb.data_ptr(), d_to.data_ptr(), len(patterns),
                                          bits.data_ptr(), st), "arx_text_regex")
        t = event_times(scan, args.calls)
        return t, bits, [[d.n_states, d.n_classes] for d in dfas]

    def time_contains(pats):
        pb, po = pack_patterns(pats)
        d_pb, d_po = torch.from_numpy(pb.copy()).cuda(), torch.from_numpy(po).cuda()
        bits = torch.empty((len(pats), store.n_words), dtype=torch.int64, device="cuda")

        def scan():
            _lib.check(lib.arx_text_contains(store.blob.data_ptr(), store.row_off.data_ptr(), n, d_pb.data_ptr(), d_po.data_ptr(), len(pats),
                                             bits.data_ptr(), st), "arx_text_contains")
        return event_times(scan, args.calls), bits

    def python_re(patterns):
        """(wall ms of one loop per pattern over texts[:re_rows], rows matched by each); `^` / `$` do not occur in the arms."""
        head, counts = texts[:re_rows], []
        h0 = time.perf_counter()
        for p in patterns:
            flags = re.ASCII | (re.IGNORECASE if p.startswith("(?i)") else 0)
            search = re.compile(p[4:] if p.startswith("(?i)") else p, flags).search
            counts.append(sum(1 for t in head if search(t)))
        return (time.perf_counter() - h0) * 1e3, counts

    def record(name, patterns, t, bits, tables=None, contains=None):
        matched = [store.count(bits[i].contiguous()) for i in range(bits.shape[0])]
        row = {"arm": name, "patterns": patterns, "states_classes": tables, "rows_matched": matched, **t, "GB_per_s": gb / (t["ms_median"] * 1e-3),
               "floor_ms": floor_ms, "times_the_floor": t["ms_median"] / floor_ms}
        if tables is not None:
            re_ms, counts = python_re(patterns)
            if re_rows == n:
                assert counts == matched, (name, "device and Python re disagree", counts, matched)
            row.update(python_re_ms=re_ms, python_re_rows=re_rows, python_re_rows_matched=counts,
                       python_re_over_device=re_ms * (n / re_rows) / t["ms_median"])
        if contains is not None:
            row["ratio_to_contains"] = t["ms_median"] / contains["ms_median"]
        out["arms"].append(row)
        print(json.dumps(row), flush=True)

    literal = re.escape(marker)
    tc, bits_c = time_contains([marker])
    record("$contains, the common 8-byte marker", [marker], tc, bits_c)
    t, bits, tabs = time_regexes([literal])
    assert torch.equal(bits, bits_c), "the literal regex and $contains disagree"
    record("$regex, the same marker as a literal", [literal], t, bits, tabs, contains=tc)
    singles = [("(?i) of the marker in lower case", "(?i)" + literal.lower())]
    t8c, bits_8c = time_contains(words)
    any_c = bits_8c[0].clone()
    for i in range(1, 8):
        any_c |= bits_8c[i]
    record("$or of 8 $contains (words of the text, 3-12 bytes), one launch", words, t8c, bits_8c)
    alternation = "|".join(re.escape(w) for w in words)
    t, bits, tabs = time_regexes([alternation])
    assert torch.equal(bits[0], any_c), "the alternation and the $or of $contains disagree"
    record("$regex, an alternation of the same 8 words", [alternation], t, bits, tabs, contains=t8c)
    singles += [("arXiv id", "\\d{4}\\.\\d{4,5}"), ("citation", "[A-Z][a-z]+ et al\\."), ("256 states", STATES_256)]
    for name, p in singles:
        t, bits, tabs = time_regexes([p])
        record(f"$regex, {name}", [p], t, bits, tabs)
    eight = [literal, singles[0][1], alternation, singles[1][1], singles[2][1], STATES_256, "[aeiou]{5}", "(?i)" + re.escape(marks[("rare", 8)]).lower()]
    t, bits, tabs = time_regexes(eight)
    record("8 regexes in one call", eight, t, bits, tabs)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
