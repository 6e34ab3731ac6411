"""`$regex` / `$not_regex` on the device: `arx_text_regex` through `DocumentStore.regex` against `evaluate_host` (the table interpreter
`regex_dfa.match_host`), bit for bit, and `HipCollection(document_regex=True).query` against `ShardIndex.search(allow=...)` with a
bitmap built on the host by Python's `re`.  Every comparison is exact (bits, ids, score bits)."""
import dataclasses
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd.where import pack_bitmap
from arxiv_rag_amd.where_document import DocumentStore, compile_where_document, evaluate_host
from tests.test_regex_dfa_host import translate

pytestmark = pytest.mark.gpu

WAVES = (0, 1, 2, 4, 8, 16)                                     # every shape of arx_text_regex_tuned
NEAR_256 = "a[ab]{6}c|d[de]{6}f"                                # 256 states after minimisation
EIGHT = ["a*", "ab", "^b", "a$", "^x*😀$", "(?i)QZ\\d$", NEAR_256, "[^a-z\\s]é."]


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _expect(texts, patterns):
    """uint64 [P, ceil(n / 64)] from the table interpreter."""
    return np.stack([pack_bitmap(evaluate_host(("regex", p), texts)) for p in patterns])


def _bits(store, patterns, waves=0):
    """`DocumentStore.regex` into a buffer of all-ones -> uint64 [P, words] on the host."""
    out = torch.full((len(patterns), store.n_words), -1, dtype=torch.int64, device="cuda")
    got = store.regex(patterns, out=out, waves_per_block=waves)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _check(texts, patterns, what, shapes=WAVES, store=None):
    store = store or DocumentStore(texts, device="cuda:0")
    want = _expect(texts, patterns)
    for waves in shapes:
        got = _bits(store, patterns, waves)
        if not np.array_equal(got, want):
            p, w = np.argwhere(got != want)[0]
            diff = int(got[p, w] ^ want[p, w])
            r = int(w) * 64 + (diff & -diff).bit_length() - 1
            row = repr(texts[r][:40]) if r < len(texts) else "beyond n_rows"
            raise AssertionError(f"{what}, waves_per_block={waves}: regex {patterns[p]!r} row {r} ({row}): device "
                                 f"{bool(got[p, w] >> np.uint64(r % 64) & np.uint64(1))}, host {bool(want[p, w] >> np.uint64(r % 64) & np.uint64(1))}; "
                                 f"{int((got != want).sum())} words differ")
    return want


PIECES = ["a", "b", "ab", "ba", "x", "c", "d", "de", "f", "é", "😀", " ", "Qz7", "qZ", "abbabac", "deddedf", "9"]


def _corpus(n, seed):
    """n short rows of PIECES (0 to 12 of them: empty rows, 1-byte rows, a multi-byte character at any offset)."""
    rs = np.random.RandomState(seed)
    return ["".join(rs.choice(PIECES, size=rs.randint(0, 13))) for _ in range(n)]


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129, 4097])
def test_eight_regexes_equal_the_table_interpreter_for_every_launch_shape(hip, n_rows):
    texts = _corpus(n_rows, n_rows)
    want = _check(texts, EIGHT, f"n_rows={n_rows}")
    assert want[0].tolist() == pack_bitmap(np.ones(n_rows, bool)).tolist()        # `a*` matches every row, and no bit at or beyond n_rows is set
    if n_rows >= 129:
        assert all(0 < int(sum(bin(int(w)).count("1") for w in want[p])) < n_rows for p in (1, 2, 3, 6)), "a regex that tells rows apart"


def test_constructed_rows(hip):
    # a match, and a multi-byte character, at every offset against the 16-byte chunks a lane reads; the rows are contiguous in the blob,
    # so row k starts at a different alignment for every k
    texts = ["x" * k + "abcd" + "y" * (k % 4) for k in range(48)] + ["x" * k + "😀" for k in range(20)] + ["x" * k + "é" + "z" * (k % 3) for k in range(20)]
    # `ab` must not match across rows: row r ends in `a` and row r + 1 starts with `b`; `^` and `$` are row ends, not chunk or blob ends
    texts += ["xa", "bx", "a", "b", "", "", "a", "", "b", "ab", "xxab", "abxx", "b" * 16, "a" * 16, "b" * 17, "x" * 15 + "a", "b"]
    long_row = "ab" * 35000 + "Qz9"                              # >= 70 000 bytes: the only "Qz9" sits in its last bytes
    texts += ["q", long_row, "", "z", "Qz9", "Qz9 "]
    patterns = ["abcd", "^x*😀$", "[^a-z]$", "ab", "^b", "a$", "(?i)QZ\\d$", "^(ab)+Qz9$"]
    want = _check(texts, patterns, "constructed")
    hit = {p: [r for r in range(len(texts)) if want[i, r >> 6] >> np.uint64(r & 63) & np.uint64(1)] for i, p in enumerate(patterns)}
    base = 48 + 40
    assert hit["abcd"] == list(range(48)) and hit["^x*😀$"] == list(range(48, 68))
    assert [r - base for r in hit["ab"] if base <= r < base + 17] == [9, 10, 11]                       # not rows 0|1, 2|3, 6|8
    assert [r - base for r in hit["^b"] if base <= r < base + 17] == [1, 3, 8, 12, 14, 16]
    assert [r - base for r in hit["a$"] if base <= r < base + 17] == [0, 2, 6, 13, 15]
    assert hit["^(ab)+Qz9$"] == [base + 18] and hit["(?i)QZ\\d$"] == [base + 18, base + 21]
    # the same bits wherever the blob starts against the 16-byte grid
    store = DocumentStore(texts, device="cuda:0")
    for shift in (1, 5, 15):
        buf = torch.zeros(store.n_bytes + 32, dtype=torch.uint8, device="cuda")
        buf[shift:shift + store.n_bytes] = store.blob[:store.n_bytes]
        moved = DocumentStore(texts[:1], device="cuda:0")
        moved.n_rows, moved.n_words, moved.n_bytes, moved.row_off = store.n_rows, store.n_words, store.n_bytes, store.row_off
        moved.blob = buf[shift:shift + store.n_bytes]
        assert moved.blob.data_ptr() % 16 == (buf.data_ptr() + shift) % 16 and (buf.data_ptr() % 16) == 0
        assert np.array_equal(_bits(moved, patterns), want), shift


def test_empty_rows_only_and_single_patterns(hip):
    texts = [""] * 70
    want = _check(texts, ["a*", "^$", "a", "$"], "empty rows", shapes=(0, 1))
    assert [int(w[0]) for w in want] == [2**64 - 1, 2**64 - 1, 0, 2**64 - 1] and [int(w[1]) for w in want] == [63, 63, 0, 63]
    _check(_corpus(300, 5), [NEAR_256], "one 256-state table", shapes=(0, 16))
    store = DocumentStore([], device="cuda:0")
    assert store.regex(["a"]).shape == (1, 0)
    with pytest.raises(ValueError, match="1..8"):
        DocumentStore(["a"], device="cuda:0").regex(["a"] * 9)


def test_literal_regex_gives_the_bitmap_of_contains(hip):
    texts = _corpus(2000, 11)
    store = DocumentStore(texts, device="cuda:0")
    literals = ["ab", "abba", "é", "😀b", "Qz7", "deddedf", " a", "zzz"]
    escaped = [re.escape(s).replace("\\ ", " ") for s in literals]
    a, b = store.regex(escaped), store.contains(literals)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and int((a != 0).sum()) > 0
    tree = compile_where_document({"$and": [{"$regex": "^(ab|ba)"}, {"$not_regex": "é"}, {"$or": [{"$contains": "x"}, {"$not_contains": "a"}]}]}, regex=True)
    words, n_allowed = store.allow(tree)
    mask = evaluate_host(tree, texts)
    assert n_allowed == int(mask.sum()) and 0 < n_allowed < len(texts)
    assert np.array_equal(words.cpu().numpy().view(np.uint64) & pack_bitmap(np.ones(len(texts), bool)), pack_bitmap(mask))


def _re_mask(f, texts):
    """bool [n]: a where_document filter evaluated with Python's `re` and `in`."""
    (op, val), = f.items()
    if op in ("$and", "$or"):
        parts = [_re_mask(g, texts) for g in val]
        return np.logical_and.reduce(parts) if op == "$and" else np.logical_or.reduce(parts)
    if op in ("$regex", "$not_regex"):
        tp, flags = translate(val)
        hit = np.array([bool(re.search(tp, t, flags)) for t in texts])
    else:
        hit = np.array([val in t for t in texts])
    return ~hit if op.startswith("$not") else hit


def _score_bits(out):
    return [np.asarray(s, np.float32).view(np.int32).tolist() for s in out["scores"]]


def test_collection_query_with_regex_filters(hip):
    from arxiv_rag_amd import config as C
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from arxiv_rag_amd.where import compile_where, evaluate
    from oracle import search_oracle as SO
    from tests.helpers import synthetic_vocab
    from tests.test_gpu_filtered_search import _collection
    emb, meta = _collection()
    n = len(meta)
    texts = [m["text"] for m in meta]
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    tok = WordPieceTokenizer.from_vocab(synthetic_vocab(cfg), cfg)
    coll = HipCollection(emb, meta, documents=True, document_regex=True)
    dev = HipCollection(emb, meta, documents=True, document_regex=True, where_on_device=True)
    hyb = HipCollection(emb, meta, documents=True, document_regex=True, keyword=True, tokenizer=tok, hybrid_filters=True)
    plain = HipCollection(emb, meta, documents=True)
    q = SO.unit_rows_f16(12, 128, 9)
    qd = torch.from_numpy(q).cuda()
    starts = {"$regex": "^(alpha|beta) (gamma|delta)( \\w+)*$"}
    mixed = {"$and": [{"$contains": "alpha beta"}, {"$not_regex": "(?i)DELTA$|^gamma"}]}
    rare = {"$regex": "^(alpha ){5,}"}
    where = {"$and": [{"section": {"$ne": "Methods"}}, {"quality_score": {"$gte": 0.9}}]}

    def expect(mask, n_results):
        allow = torch.from_numpy(pack_bitmap(mask).view(np.int64)).cuda()
        s, i = coll.index.search(qd, n_results, allow=allow, n_allowed=int(mask.sum()))
        return s.cpu().numpy(), i.cpu().numpy()

    def same(out, s, i, what):
        for qi in range(q.shape[0]):
            keep = i[qi] >= 0
            assert out["indices"][qi] == i[qi][keep].tolist(), (what, qi)
            assert _score_bits(out)[qi] == s[qi][keep].view(np.int32).tolist(), (what, qi)

    counts = {}
    for name, f, n_results in (("starts", starts, 10), ("mixed", mixed, 32), ("rare", rare, 10)):
        mask = _re_mask(f, texts)
        counts[name] = int(mask.sum())
        assert np.array_equal(mask, evaluate_host(compile_where_document(f, regex=True), texts)), name
        s, i = expect(mask, n_results)
        for which, c in (("default", coll), ("hybrid_filters", hyb)):
            same(c.query(query_embeddings=q, n_results=n_results, where_document=f), s, i, (name, which))
        both = mask & evaluate(compile_where(where), meta)
        s, i = expect(both, n_results)
        for which, c in (("default", coll), ("where_on_device", dev)):
            same(c.query(query_embeddings=q, n_results=n_results, where=where, where_document=f), s, i, (name, which, "with where"))
    assert 0.05 * n < counts["starts"] < 0.5 * n and 0 < counts["mixed"] < 0.5 * n and 0 < counts["rare"] < 0.05 * n, counts
    # one filter per query: a regex, the mixed tree, none
    per_query = [(starts, mixed, None, rare)[j % 4] for j in range(q.shape[0])]
    for which, c, kw in (("default", coll, {}), ("where_on_device", dev, {"where": where}), ("hybrid_filters", hyb, {})):
        out = c.query(query_embeddings=q, n_results=10, where_document=per_query, **kw)
        for qi, f in enumerate(per_query):
            mask = np.ones(n, bool) if f is None else _re_mask(f, texts)
            if kw:
                mask = mask & evaluate(compile_where(where), meta)
            s, i = expect(mask, 10)
            keep = i[qi] >= 0
            assert out["indices"][qi] == i[qi][keep].tolist() and _score_bits(out)[qi] == s[qi][keep].view(np.int32).tolist(), (which, qi)
    # the keyword side of a hybrid query takes the regex bitmap too: at alpha = 1 the fused ranking is the filtered dense one
    dense = hyb.query(query_embeddings=q, n_results=10, where_document=mixed)
    fused = hyb.query(query_embeddings=q, query_texts=["alpha beta"] * 12, n_results=10, hybrid_alpha=1.0, where_document=mixed)
    assert fused["indices"] == dense["indices"]
    mask = _re_mask(mixed, texts)
    half = hyb.query(query_embeddings=q, query_texts=["alpha beta"] * 12, n_results=10, hybrid_alpha=0.5, where_document=mixed)
    assert all(mask[r] for rows in half["indices"] for r in rows) and all(len(rows) == 10 for rows in half["indices"])
    # without the flag the refusal stays
    with pytest.raises(ValueError, match="unknown operator '\\$regex'"):
        plain.query(query_embeddings=q, where_document=starts)
    with pytest.raises(ValueError, match="unknown operator '\\$not_regex'"):
        plain.query(query_embeddings=q, where_document=[mixed] * 12)
    with pytest.raises(ValueError, match="look-around"):
        coll.query(query_embeddings=q, where_document={"$regex": "(?=a)b"})
