"""Chroma `where_document` on the device: the substring scan (`arx_text_contains`), the bitmap count, `DocumentStore.allow`,
`HipCollection.query(where_document=...)` and the CLI flag.  The expected bits always come from Python's `in` on the strs; every
comparison is exact (bits, ids, score bits)."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd.where import pack_bitmap
from arxiv_rag_amd.where_document import (DocumentStore, compile_where_document, encode_text, evaluate_host, pack_documents, pack_patterns)

pytestmark = pytest.mark.gpu

PATTERN_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256)


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _expect(texts, patterns):
    """uint64 [P, ceil(n / 64)] from Python `in`."""
    return np.stack([pack_bitmap(np.fromiter((p in t for t in texts), dtype=bool, count=len(texts))) for p in patterns])


def _scan(hip, texts, patterns, prefill=0xFF):
    """arx_text_contains through the C ABI -> uint64 [P, words] on the host; the output buffer holds `prefill` bytes before the call."""
    blob, off = pack_documents(texts)
    pb, po = pack_patterns(patterns)
    n, words = len(texts), (len(texts) + 63) // 64
    d_blob = torch.zeros(max(16, blob.shape[0]), dtype=torch.uint8, device="cuda")
    d_blob[:blob.shape[0]] = torch.from_numpy(blob.copy()).cuda()
    d_off, d_pb, d_po = torch.from_numpy(off).cuda(), torch.from_numpy(pb.copy()).cuda(), torch.from_numpy(po).cuda()
    out = torch.full((len(patterns), words), prefill, dtype=torch.uint8, device="cuda").repeat_interleave(8, dim=1).contiguous().view(torch.int64)
    assert out.shape == (len(patterns), words)
    rc = hip.load().arx_text_contains(d_blob.data_ptr(), d_off.data_ptr(), n, d_pb.data_ptr(), d_po.data_ptr(), len(patterns), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    hip.check(rc, "arx_text_contains")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _check(hip, texts, patterns, what, prefill=0xFF):
    got, want = _scan(hip, texts, patterns, prefill), _expect(texts, patterns)
    if not np.array_equal(got, want):
        p, w = np.argwhere(got != want)[0]
        diff = int(got[p, w] ^ want[p, w])
        r = int(w) * 64 + (diff & -diff).bit_length() - 1
        raise AssertionError(f"{what}: pattern {p} ({patterns[p][:40]!r}, {len(encode_text(patterns[p]))} B) row {r} "
                             f"({len(encode_text(texts[r])) if r < len(texts) else 'beyond n_rows'} B): device "
                             f"{bool(got[p, w] >> np.uint64(r % 64) & np.uint64(1))}, python {bool(want[p, w] >> np.uint64(r % 64) & np.uint64(1))}; "
                             f"{int((got != want).sum())} words differ")
    return want


# ---- seeded corpora ---------------------------------------------------------------------------------------------------------------------
VOCAB = ["ab", "ba", "aab", "abba", "b", "a", "bab", " "]          # a small alphabet: matches and near-matches everywhere


def _base(rs, n_bytes):
    return "".join(rs.choice(VOCAB, size=n_bytes // 2 + 16))[:n_bytes]


def _corpus(n, seed, typical, long_row=0):
    """n texts cut out of one seeded string: lengths 0, 1, m - 1, m, m + 1 for every pattern length m, 5000, and 0..`typical` otherwise;
    `long_row`: one row of that many bytes as well."""
    rs = np.random.RandomState(seed)
    base = _base(rs, 1 << 20)
    special = [0, 1, 5000] + [m + d for m in PATTERN_LENGTHS for d in (-1, 0, 1)]
    lens = rs.randint(0, typical + 1, size=n)
    if n == 1:
        lens[:] = 5000
    else:
        where = rs.permutation(n)[:len(special)]
        lens[where] = special[:where.shape[0]]
    starts = rs.randint(0, len(base) - 5001, size=n)
    texts = [base[s:s + l] for s, l in zip(starts.tolist(), lens.tolist())]
    if long_row:
        big = _base(rs, long_row - 3) + "Qz9"                  # the only "Qz9" of the corpus sits in the row's last bytes
        texts[int(rs.randint(n))] = big
    return texts, rs


def _patterns(texts, rs, count):
    """`count` patterns, cycling through PATTERN_LENGTHS: substrings of rows (at the start, at the end, inside), whole rows, and copies with
    one changed character (the near-matches).  ASCII corpus: characters are bytes."""
    by_len = sorted(range(len(texts)), key=lambda r: -len(texts[r]))
    out = []
    for i in range(count):
        m = PATTERN_LENGTHS[(i * 5 + i // 13) % len(PATTERN_LENGTHS)]
        fits = [r for r in by_len[:64] if len(texts[r]) >= m]
        exact = [r for r in range(min(len(texts), 4000)) if len(texts[r]) == m]
        if not fits:
            out.append("ab"[i % 2] * m)
            continue
        t = texts[fits[int(rs.randint(len(fits)))]]
        kind = i % 5
        if kind == 0 and exact:
            s = texts[exact[int(rs.randint(len(exact)))]]       # a pattern equal to a whole row
        elif kind == 1:
            s = t[:m]
        elif kind == 2:
            s = t[len(t) - m:]
        else:
            a = int(rs.randint(len(t) - m + 1))
            s = t[a:a + m]
        if kind == 4:                                           # near-match: every proper prefix (or suffix) still occurs
            s = (s[:-1] + "z") if i % 2 else ("z" + s[1:])
        assert len(s) == m
        out.append(s)
    return out


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 200001])
def test_text_contains_equals_python_in_on_seeded_corpora(hip, n_rows):
    """Rows of 0, 1, m - 1, m, m + 1 and 5000 bytes (and, at 1000 rows, one row of more than 4 MB); pattern lengths 1..256; 1, 2, 31 and 32
    patterns per call with duplicates among them."""
    texts, rs = _corpus(n_rows, seed=n_rows, typical=100 if n_rows > 1000 else 400, long_row=(4 << 20) + 77 if n_rows == 1000 else 0)
    if n_rows > 1:
        assert {0, 1, 5000} <= {len(t) for t in texts}
    if n_rows == 1000:
        assert max(len(t) for t in texts) > 4 << 20
    matched = set()
    for n_pat in (1, 2, 31, 32):
        pats = _patterns(texts, rs, n_pat)
        if n_pat >= 31:
            pats[7], pats[19] = pats[3], pats[3]                # duplicates
            pats[11] = "Qz9"
        want = _check(hip, texts, pats, f"n_rows={n_rows} n_pat={n_pat}", prefill=0xFF if n_pat % 2 else 0x00)
        matched |= {len(p) for p, w in zip(pats, want) if w.any()}
        if n_pat == 32:
            assert {len(p) for p in pats} == set(PATTERN_LENGTHS)
            if n_rows == 1000:
                assert int(sum(bin(int(x)).count("1") for x in want[11])) == 1       # found at the end of the 4 MB row only
    for m in PATTERN_LENGTHS:                                    # every length alone as well, so that its halo is the one in use
        longest = max(texts, key=len)
        pats = [p for p in _patterns(texts, rs, 26) if len(p) == m][:2] + [longest[len(longest) // 2:][:m]]      # the last one occurs for certain
        assert len(pats[-1]) == m
        want = _check(hip, texts, pats, f"n_rows={n_rows} length {m} alone")
        matched |= {m for w in want if w.any()}
    assert matched == set(PATTERN_LENGTHS), f"no pattern of length {sorted(set(PATTERN_LENGTHS) - matched)} matched any row: the corpus proves nothing for it"


def test_constructed_cases(hip):
    rs = np.random.RandomState(5)
    letters = np.array(list("cdefghijklmnopqrstuvw"))

    def rnd(n):
        return "".join(rs.choice(letters, size=n))

    def none_set(texts, pats, what):
        want = _check(hip, texts, pats, what)
        assert not want.any(), what

    # a pattern made of the tail of row r and the head of row r + 1 that occurs nowhere else: at every alignment of the boundary in a 16-byte chunk
    for k in range(0, 36):
        none_set(["x" * k + "abc", "defg" + "y" * 5, "zz"], ["cd", "bcde", "abcdefg", "cdefgy"], f"straddle at {k}")
        none_set(["x" * k + "abc", "", "defg" + "y" * 5], ["cd", "bcde", "abcdefg"], f"straddle over an empty row at {k}")
    for m in (5, 17, 64, 255, 256):                             # long patterns across a boundary, also far from the blob's start
        a, b = rnd(700), rnd(700)
        for cut in (1, m // 2, m - 1):
            none_set([rnd(1500), a, b, rnd(90)], [a[len(a) - cut:] + b[:m - cut]], f"straddle length {m} cut {cut}")
            none_set([a, "", "", b], [a[len(a) - cut:] + b[:m - cut]], f"straddle length {m} cut {cut} over two empty rows")
    # first and last bytes of the blob, first and last bytes of a row, a pattern equal to a whole row; blob sizes around a multiple of 16
    for pad in range(0, 18):
        texts = ["HEAD" + "z" * pad, "q" * 7, "LEFTmiddleRIGHT", "whole row", "", "z" * 11 + "TAIL"]
        pats = ["HEAD", "TAIL", "LEFT", "RIGHT", "whole row", "LEFTmiddleRIGHT", "D" + "z" * pad, "zTAIL", "HEAD" + "z" * pad + "q", "whole row "]
        want = _check(hip, texts, pats, f"ends, pad {pad}")
        assert [int(w[0]) for w in want] == [1, 32, 4, 4, 8, 4, 1, 32, 0, 0]
    want = _check(hip, ["T"], ["T", "TT", "t"], "one row of one byte")
    assert [int(w[0]) for w in want] == [1, 0, 0]
    want = _check(hip, ["", "", ""], ["a"], "only empty rows")
    assert not want.any()
    # self-overlapping patterns
    want = _check(hip, ["aaaa", "aa", "ababab", "abab", "aabaab", "abaabaa"], ["aaa", "abab", "aabaa", "ababab", "aaaaa"], "self-overlap")
    assert [int(w[0]) for w in want] == [0b000001, 0b001100, 0b110000, 0b000100, 0]
    # every proper prefix occurs, the pattern itself does not (short, and long enough to leave the 4-byte window)
    for pat in ("abcd", "abcdefgh", rnd(40), rnd(256)):
        text = "#".join(pat[:i] for i in range(1, len(pat)))
        none_set([text, pat[:-1], pat[1:], pat[:-1] + "#" + pat[-1]], [pat], f"prefixes of a {len(pat)}-byte pattern")
        want = _check(hip, [text + pat, text, pat + text], [pat], f"... and the pattern after its prefixes ({len(pat)} B)")
        assert int(want[0, 0]) == 0b101
    # multi-byte UTF-8 and lone surrogates
    texts = ["été à la plage", "ete a la plage", "€uro 5€", "\U0001d53d is a field", "a\ud800b", "\ud800", "ab", "x\udc00\ud800y", "日本語のテキスト", ""]
    pats = ["é", "à la", "€", "5€", "\U0001d53d", "\ud800", "a\ud800", "\udc00\ud800", "本語", "語の", "e", "\udc00"]
    want = _check(hip, texts, pats, "utf-8")
    assert int(want[5, 0]) == 0b0010110000 and int(want[0, 0]) == 1 and int(want[8, 0]) == 1 << 8
    # the match only in the very last row of a partial last group
    for n in (65, 130, 191):
        texts = ["abab"] * (n - 1) + ["needle"]
        want = _check(hip, texts, ["needle", "abab", "needl", "eedle "], f"last row of {n}")
        assert int(sum(bin(int(x)).count("1") for x in want[0])) == 1 and int(want[0, -1]) == 1 << ((n - 1) % 64)
        assert int(sum(bin(int(x)).count("1") for x in want[1])) == n - 1 and not want[3].any()


def test_output_does_not_depend_on_the_buffer_and_bits_beyond_n_rows_are_zero(hip):
    for n in (1, 63, 65, 1000):
        texts, rs = _corpus(n, seed=100 + n, typical=200)
        pats = ["a", "b", "ab", " ", "zz"] + _patterns(texts, rs, 8)
        ones, zeros = _scan(hip, texts, pats, prefill=0xFF), _scan(hip, texts, pats, prefill=0x00)
        assert np.array_equal(ones, zeros) and np.array_equal(ones, _expect(texts, pats))
        assert ones[0].any() and not ones[4].any()
        if n % 64:
            assert not (ones[:, -1] >> np.uint64(n % 64)).any(), "bits at or beyond n_rows must be written as 0"


def test_bitmap_count_equals_the_host_popcount(hip):
    lib = hip.load()
    rs = np.random.RandomState(11)
    out = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for n in (1, 63, 64, 65, 1000, 200001, 1 << 20):
        words = (n + 63) // 64
        for kind in ("random", "ones", "zeros", "stray"):
            w = rs.randint(0, 1 << 63, size=words, dtype=np.int64).view(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=words).astype(np.uint64)
            if kind == "ones":
                w[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
            elif kind == "zeros":
                w[:] = 0
            bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:n]
            if kind == "stray" and n % 64:                      # the last word's bits beyond n_rows all set: not counted
                w[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
            d = torch.from_numpy(w.view(np.int64)).cuda()
            hip.check(lib.arx_bitmap_count(d.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_bitmap_count")
            assert int(out.item()) == int(bits.sum()), (n, kind)


# ---- DocumentStore ----------------------------------------------------------------------------------------------------------------------
TREES = [
    {"$contains": "ab"}, {"$contains": "abba ab"}, {"$not_contains": "ab"}, {"$not_contains": "bab"}, {"$contains": "zz"}, {"$not_contains": "zz"},
    {"$and": [{"$contains": "abba"}, {"$not_contains": "bab"}]},
    {"$or": [{"$contains": "aab aab"}, {"$contains": "b  a"}]},
    {"$and": [{"$or": [{"$contains": "abba"}, {"$not_contains": " "}]}, {"$not_contains": "aaba"},
              {"$or": [{"$and": [{"$contains": "ba b"}, {"$contains": "abba"}]}, {"$contains": "bb ab"}, {"$not_contains": "a"}]}]},
    {"$or": [{"$and": [{"$not_contains": "ab"}, {"$not_contains": "ba"}]}, {"$and": [{"$contains": "ab"}, {"$contains": "ab"}]}]},
]


@pytest.mark.parametrize("n", [1, 64, 65, 1000, 70001])
def test_document_store_allow_equals_the_host_evaluation(hip, n):
    texts, _ = _corpus(n, seed=7 + n, typical=60)
    store = DocumentStore(texts, device="cuda:0", slab_rows=257)         # several slabs
    blob, off = pack_documents(texts)
    assert store.n_bytes == blob.shape[0] and np.array_equal(store.row_off.cpu().numpy(), off)
    assert np.array_equal(store.blob[:store.n_bytes].cpu().numpy(), blob)
    sizes = []
    for f in TREES:
        tree = compile_where_document(f)
        mask = evaluate_host(tree, texts)
        words, n_allowed = store.allow(tree)
        assert words.dtype == torch.int64 and words.shape == ((n + 63) // 64,) and words.is_cuda
        got = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, mask), (f, "bits below n_rows")
        assert n_allowed == int(mask.sum()), (f, n_allowed, int(mask.sum()))
        sizes.append(n_allowed)
    if n >= 1000:
        assert 0 < min(s for s in sizes if s) < n // 2 < max(sizes) <= n
    bits = store.contains(["ab", "zz", "ab"])
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), _expect(texts, ["ab", "zz", "ab"]))
    with pytest.raises(ValueError):
        store.contains(["a" * 257])
    with pytest.raises(ValueError):
        store.contains([f"p{i}" for i in range(33)])


def test_document_store_of_no_rows_and_of_empty_rows(hip):
    store = DocumentStore([], device="cuda:0")
    words, n_allowed = store.allow(compile_where_document({"$not_contains": "a"}))
    assert words.shape == (0,) and n_allowed == 0
    store = DocumentStore(["", "", ""], device="cuda:0")
    words, n_allowed = store.allow(compile_where_document({"$not_contains": "a"}))
    assert n_allowed == 3 and int(words[0].item()) & 7 == 7
    assert store.allow(compile_where_document({"$contains": "a"}))[1] == 0


# ---- HipCollection.query(where_document=...) ---------------------------------------------------------------------------------------------
def _score_bits(out):
    return [np.array(s, np.float32).view(np.int32).tolist() for s in out["scores"]]


def test_collection_query_where_document(hip):
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.where import compile_where, evaluate
    from oracle import search_oracle as SO
    from tests.test_gpu_filtered_search import _collection
    emb, meta = _collection()
    n = len(meta)
    texts = [m["text"] for m in meta]
    coll = HipCollection(emb, meta, documents=True)
    plain = HipCollection(emb, meta)
    q = SO.unit_rows_f16(12, 128, 9)
    qd = torch.from_numpy(q).cuda()
    half = {"$or": [{"$contains": "alpha beta"}, {"$contains": "gamma delta"}]}
    few = {"$and": [{"$contains": "alpha alpha alpha"}, {"$contains": "delta delta delta"}]}
    none = {"$contains": "Alpha"}                               # case-sensitive: the texts are lower case
    counts = {}
    for name, f, n_results in (("half", half, 10), ("half-32", half, 32), ("few", few, 10), ("none", none, 5),
                               ("not", {"$not_contains": "alpha"}, 10)):
        mask = evaluate_host(compile_where_document(f), texts)
        rows = np.nonzero(mask)[0]
        counts[name] = rows.shape[0]
        want_n = min(n_results, rows.shape[0])
        out = coll.query(query_embeddings=q, n_results=n_results, where_document=f)
        # (a) the host mask of f handed to the filtered search as `allow`
        allow = torch.from_numpy(pack_bitmap(mask).view(np.int64)).cuda()
        s, i = coll.index.search(qd, n_results, allow=allow, n_allowed=int(mask.sum()))
        s, i = s.cpu().numpy(), i.cpu().numpy()
        for qi in range(q.shape[0]):
            keep = i[qi] >= 0
            assert len(out["indices"][qi]) == want_n, (name, "list length")
            assert out["indices"][qi] == i[qi][keep].tolist(), (name, qi)
            assert _score_bits(out)[qi] == s[qi][keep].view(np.int32).tolist(), (name, qi)
            assert all(mask[r] for r in out["indices"][qi])
            assert out["documents"][qi] == [texts[r] for r in out["indices"][qi]]
        # (b) the unfiltered query of a collection built from the satisfying rows alone, ids mapped back
        if rows.shape[0]:
            sub = HipCollection(emb[rows], [meta[r] for r in rows]).query(query_embeddings=q, n_results=want_n)
            assert [[int(rows[j]) for j in l] for l in sub["indices"]] == out["indices"], name
            assert _score_bits(sub) == _score_bits(out), name
        else:
            assert out["indices"] == [[] for _ in range(q.shape[0])] and out["ids"] == out["indices"] and out["scores"] == out["indices"]
    assert 0.3 * n < counts["half"] < 0.7 * n and 0 < counts["few"] < 10 and counts["none"] == 0, counts
    # with a `where` as well: the AND of the two host masks
    for where in ({"section": "abstract"}, {"$and": [{"section": {"$ne": "Methods"}}, {"quality_score": {"$gte": 0.9}}]}, {"paper_id": "none such"}):
        both = evaluate(compile_where(where), meta) & evaluate_host(compile_where_document(half), texts)
        out = coll.query(query_embeddings=q, n_results=10, where=where, where_document=half)
        allow = torch.from_numpy(pack_bitmap(both).view(np.int64)).cuda()
        s, i = coll.index.search(qd, 10, allow=allow, n_allowed=int(both.sum()))
        s, i = s.cpu().numpy(), i.cpu().numpy()
        for qi in range(q.shape[0]):
            keep = i[qi] >= 0
            assert out["indices"][qi] == i[qi][keep].tolist() and len(out["indices"][qi]) == min(10, int(both.sum())), (where, qi)
            assert _score_bits(out)[qi] == s[qi][keep].view(np.int32).tolist()
    # without where_document nothing changes: the same answer as a collection built without documents
    a, b = coll.query(query_embeddings=q, n_results=10), plain.query(query_embeddings=q, n_results=10)
    assert a["indices"] == b["indices"] and _score_bits(a) == _score_bits(b)

    class LengthReranker:                                        # anything with HipCrossEncoder's `predict`
        def predict(self, pairs, **kw):
            return np.array([len(doc) for _, doc in pairs], np.float32)
    out = coll.query(query_embeddings=q, query_texts=["alpha beta"] * 12, n_results=5, n_candidates=20, reranker=LengthReranker(), where_document=half)
    cand = coll.query(query_embeddings=q, n_results=20, where_document=half)
    mask = evaluate_host(compile_where_document(half), texts)
    for qi in range(12):
        assert all(mask[r] for r in out["indices"][qi]) and len(out["indices"][qi]) == 5
        assert set(out["indices"][qi]) <= set(cand["indices"][qi])                   # the cross-encoder saw the filtered candidates
        assert out["rerank_scores"][qi] == sorted(out["rerank_scores"][qi], reverse=True)
    # refusals
    with pytest.raises(ValueError, match="hybrid_alpha"):
        coll.query(query_embeddings=q, query_texts=["a"] * 12, where_document=half, hybrid_alpha=0.5)
    with pytest.raises(ValueError, match="documents=True"):
        plain.query(query_embeddings=q, where_document=half)
    with pytest.raises(ValueError, match="\\$regex"):
        coll.query(query_embeddings=q, where_document={"$regex": "a.*"})
    with pytest.raises(ValueError, match="257 bytes"):
        coll.query(query_embeddings=q, where_document={"$contains": "a" * 257})


def test_collection_shard_scans_its_own_rows(hip):
    """rank 1 of 2 (no process group: the shard's own search): the document store covers rows [lo, hi) and the ids are global."""
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    from tests.test_gpu_filtered_search import _collection
    emb, meta = _collection(n=1001)
    coll = HipCollection(emb, meta, rank=1, world=2, documents=True)
    lo, hi = coll.lo, coll.hi
    assert coll.documents.n_rows == hi - lo and 0 < lo < hi == 1001
    f = {"$contains": "beta gamma"}
    mask = evaluate_host(compile_where_document(f), [m["text"] for m in meta[lo:hi]])
    words, n_allowed = coll.documents.allow(compile_where_document(f))
    assert n_allowed == int(mask.sum()) > 0
    q = torch.from_numpy(SO.unit_rows_f16(5, 128, 4)).cuda()
    s, i = coll.index.search(q, 10, allow=words, n_allowed=n_allowed)
    i = i.cpu().numpy()
    assert ((i >= lo) & (i < hi)).all() and all(mask[j - lo] for j in i.ravel())


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def test_cli_where_document_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script with --queries and --where-document: every hit's text contains the string and the lists are the top-10 of the
    chunks that contain it (the fp16 rows the script wrote, the queries as it encoded them, filtered in Python)."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from oracle import search_oracle as SO
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=60, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text("\n".join(" ".join(words[i:i + 6]) for i in range(0, 48, 6)) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    GEN._model, GEN._model_name = None, None
    kept = GEN.load_chunks_parallel(tmp_path / "in", 0.9, 4)
    # a word out of the corpus itself that some, but not most, chunks contain
    cands = sorted({w for c in kept[:50] for w in c["text"].split(" ")})
    hits = {p: sum(p in c["text"] for c in kept) for p in cands}
    needle = min(cands, key=lambda p: (abs(hits[p] - 40), p))
    assert 10 < hits[needle] < len(kept) // 2, (needle, hits[needle], len(kept))
    rc = GEN.main([str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
                   "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"),
                   "--where-document", json.dumps({"$contains": needle})])
    assert rc == 0
    ok = np.array([needle in c["text"] for c in kept])
    res = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
    qs = (tmp_path / "queries.txt").read_text().split("\n")[:-1]
    assert [r["query"] for r in res] == qs
    arr = np.load(tmp_path / "embeddings_saved" / "embeddings.npy")
    assert arr.shape[0] == len(kept)
    qd = torch.empty((len(qs), 384), dtype=torch.float16, device="cuda")
    GEN._model.encode(qs, normalize_embeddings=True, device_f16_out=qd, low_latency=True)
    rows = np.nonzero(ok)[0]
    rs2, ri2 = SO.topk_search(arr[rows].astype(np.float16), qd.cpu().numpy(), 11)
    for qi, r in enumerate(res):
        got = [h["index"] for h in r["results"]]
        assert len(got) == 10 and all(needle in kept[j]["text"] for j in got), "a hit whose text does not contain the string"
        assert [h["chunk_id"] for h in r["results"]] == [kept[j]["chunk_id"] for j in got]
        assert all(set(h) == {"rank", "score", "index", "chunk_id"} for h in r["results"])       # search_results.json keeps its shape
        if got != rows[ri2[qi, :10]].tolist():                   # the same chunks as the Python-side filtering of an exhaustive search,
            assert set(got) == set(rows[ri2[qi, :10]].tolist()) or rs2[qi, 9] - rs2[qi, 10] < 1e-6      # up to exact score ties
    GEN._model, GEN._model_name = None, None
