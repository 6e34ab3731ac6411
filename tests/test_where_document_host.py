"""Chroma `where_document` filters on the host: validation, the pure-Python definition, packing, the CLI's refusals and the C ABI's
declarations (the device scan itself: tests/test_gpu_where_document.py)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd.where_document import (MAX_PATTERN_BYTES, MAX_PATTERNS, compile_where_document, encode_text, evaluate_host, pack_documents,
                                          pack_patterns, patterns_of)

ROOT = Path(__file__).resolve().parents[1]


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_valid_trees_compile_and_patterns_are_distinct_in_first_seen_order():
    assert compile_where_document({"$contains": "abc"}) == ("contains", "abc")
    assert compile_where_document({"$not_contains": "abc"}) == ("not_contains", "abc")
    f = {"$and": [{"$contains": "b"}, {"$or": [{"$not_contains": "a"}, {"$contains": "b"}, {"$and": [{"$contains": "c"}, {"$contains": "a"}]}]}]}
    tree = compile_where_document(f)
    assert tree == ("and", (("contains", "b"), ("or", (("not_contains", "a"), ("contains", "b"), ("and", (("contains", "c"), ("contains", "a")))))))
    assert patterns_of(tree) == ["b", "a", "c"]
    assert patterns_of(compile_where_document({"$or": [{"$contains": "x"}] * 5})) == ["x"]
    assert compile_where_document({"$or": ({"$contains": "x"},)}) == ("or", (("contains", "x"),))      # a tuple is a list too


@pytest.mark.parametrize("bad,part", [
    ({"$regex": "a.*"}, "$regex"), ({"$not_regex": "a"}, "$not_regex"), ({"$like": "a"}, "$like"), ({"text": "a"}, "'text'"),
    ({"$contains": ""}, "non-empty string"), ({"$not_contains": ""}, "$not_contains"),
    ({"$contains": 3}, "must be a string"), ({"$contains": None}, "$contains"), ({"$contains": ["a"]}, "$contains"), ({"$contains": b"a"}, "$contains"),
    ({"$and": []}, "$and"), ({"$or": []}, "$or"), ({"$and": {"$contains": "a"}}, "$and"), ({"$or": "a"}, "$or"),
    ({"$contains": "a", "$not_contains": "b"}, "one operator"), ({}, "non-empty dict"), ([], "non-empty dict"), ("a", "non-empty dict"), (None, "non-empty dict"),
    ({"$and": [{"$contains": "a"}, {"$or": [{"$contains": "b"}, {"$regex": "c"}]}]}, "$regex"),
    ({"$and": [{"$contains": "a"}, {"$contains": ""}]}, "non-empty string"),
    ({"$or": [{"$contains": "a"}, "b"]}, "non-empty dict"),
])
def test_malformed_filters_raise_value_error_naming_the_part(bad, part):
    with pytest.raises(ValueError) as e:
        compile_where_document(bad)
    assert "where_document" in str(e.value) and part in str(e.value), str(e.value)


def test_limits_are_counted_in_utf8_bytes_and_in_distinct_patterns():
    assert (MAX_PATTERN_BYTES, MAX_PATTERNS) == (256, 32)
    compile_where_document({"$contains": "a" * 256})
    with pytest.raises(ValueError, match="257 bytes"):
        compile_where_document({"$contains": "a" * 257})
    euro = "€"                                            # 3 bytes as UTF-8
    compile_where_document({"$contains": euro * 85 + "a"})    # 256 bytes
    with pytest.raises(ValueError, match="258 bytes"):
        compile_where_document({"$not_contains": euro * 86})  # 86 characters, 258 bytes
    with pytest.raises(ValueError, match="259 bytes"):
        compile_where_document({"$contains": "\ud800" * 85 + "abcd"})      # a lone surrogate is 3 bytes under surrogatepass
    leaves = [{"$contains": f"p{i}"} for i in range(33)]
    assert len(patterns_of(compile_where_document({"$or": leaves[:32]}))) == 32
    assert len(patterns_of(compile_where_document({"$or": leaves[:32] + leaves[:7]}))) == 32      # duplicates do not count
    with pytest.raises(ValueError, match="33 distinct patterns"):
        compile_where_document({"$or": leaves})
    with pytest.raises(ValueError, match="33 distinct patterns"):
        compile_where_document({"$and": [{"$or": leaves[:20]}, {"$or": [{"$not_contains": f"p{i}"} for i in range(20, 33)]}]})
    with pytest.raises(ValueError):
        pack_patterns(["a"] * 33)
    with pytest.raises(ValueError):
        pack_patterns([])
    with pytest.raises(ValueError):
        pack_patterns(["a" * 257])
    with pytest.raises(ValueError):
        pack_patterns(["a", ""])
    blob, off = pack_patterns(["ab", euro, "ab"])
    assert blob.tobytes() == b"ab\xe2\x82\xacab" and off.tolist() == [0, 2, 5, 7] and off.dtype == np.int32 and blob.dtype == np.uint8


# ---- the definition --------------------------------------------------------------------------------------------------------------------
TEXTS = ["", "a", "The Lipschitz constant", "lipschitz again", "banana bandana", "abab", "Lipschitz and banana", "x" * 300 + "Lip" + "schitz"]


def test_evaluate_host_against_hand_written_expectations():
    def ev(f):
        return evaluate_host(compile_where_document(f), TEXTS).tolist()
    assert ev({"$contains": "Lipschitz"}) == [False, False, True, False, False, False, True, True]
    assert ev({"$contains": "lipschitz"}) == [False, False, False, True, False, False, False, False]          # case-sensitive
    assert ev({"$not_contains": "a"}) == [True, False, False, False, False, False, False, True]               # the empty text contains nothing
    assert ev({"$not_contains": "Lipschitz"}) == [True, True, False, True, True, True, False, False]
    assert ev({"$contains": "ana b"}) == [False, False, False, False, True, False, False, False]
    assert ev({"$contains": "bab"}) == [False, False, False, False, False, True, False, False]
    assert ev({"$and": [{"$contains": "Lipschitz"}, {"$contains": "banana"}]}) == [False, False, False, False, False, False, True, False]
    assert ev({"$or": [{"$contains": "lipschitz"}, {"$contains": "banana"}]}) == [False, False, False, True, True, False, True, False]
    assert ev({"$and": [{"$or": [{"$contains": "Lipschitz"}, {"$contains": "lipschitz"}]}, {"$not_contains": "banana"},
                        {"$or": [{"$not_contains": "x"}, {"$and": [{"$contains": "xL"}, {"$contains": "tz"}]}]}]}) \
        == [False, False, True, True, False, False, False, True]
    out = evaluate_host(("contains", "a"), [])
    assert out.shape == (0,) and out.dtype == bool


# ---- packing, and the claim the device path rests on -----------------------------------------------------------------------------------
def test_pack_documents_offsets_empty_strings_non_ascii_and_a_lone_surrogate():
    texts = ["", "abc", "", "été", "€", "\U0001d53d x", "a\ud800b", "", ""]
    blob, off = pack_documents(texts)
    assert blob.dtype == np.uint8 and off.dtype == np.int64 and off.shape == (len(texts) + 1,)
    assert off.tolist() == [0, 0, 3, 3, 8, 11, 17, 22, 22, 22] and blob.shape[0] == 22
    for r, t in enumerate(texts):
        assert blob[off[r]:off[r + 1]].tobytes() == t.encode("utf-8", "surrogatepass")
    assert blob[off[6]:off[7]].tobytes() == b"a\xed\xa0\x80b"
    with pytest.raises(UnicodeEncodeError):
        "a\ud800b".encode("utf-8")                            # why the packing says surrogatepass
    blob, off = pack_documents([])
    assert blob.shape == (0,) and off.tolist() == [0]
    blob, off = pack_documents(["", ""])
    assert blob.shape == (0,) and off.tolist() == [0, 0, 0]


def test_str_containment_equals_byte_containment_of_the_encodings():
    """Python `s in t` == `bytes.find` on the UTF-8 encodings, on seeded random strings over a small alphabet with 1-, 2-, 3- and 4-byte
    characters and a lone surrogate: UTF-8 is self-synchronising, so a byte match cannot begin or end inside a character."""
    rs = np.random.RandomState(7)
    alphabet = ["a", "b", "é", "è", "€", "₭", "\U0001d53d", "\U0001d53e", "\ud800"]
    assert sorted({len(encode_text(c)) for c in alphabet}) == [1, 2, 3, 4]
    n_true = n_false = 0
    for _ in range(4000):
        t = "".join(alphabet[i] for i in rs.randint(len(alphabet), size=rs.randint(0, 40)))
        s = "".join(alphabet[i] for i in rs.randint(len(alphabet), size=rs.randint(1, 5)))
        want = s in t
        assert (encode_text(t).find(encode_text(s)) >= 0) == want, (t, s)
        n_true += want
        n_false += not want
    assert n_true > 300 and n_false > 300


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def _boom(name):
    raise AssertionError("the model must not be loaded")


def test_cli_where_document_is_parsed_and_refused_before_any_model_is_loaded(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    args = GEN.build_parser().parse_args(["in", "--queries", "q.txt", "--where-document", '{"$contains": "Lipschitz"}'])
    assert GEN.check_where_document_args(args) is None and args.where_document_filter == {"$contains": "Lipschitz"}
    args = GEN.build_parser().parse_args(["in"])
    assert GEN.check_where_document_args(args) is None and args.where_document_filter is None
    args = GEN.build_parser().parse_args(["in", "--where", '{"section": "abstract"}', "--where-document", '{"$not_contains": "x"}'])
    assert GEN.check_where_args(args) is None and GEN.check_where_document_args(args) is None       # the two filters combine
    (tmp_path / "in").mkdir()
    for extra, msg in ((["--where-document", "{$contains: a}"], "not valid JSON"),
                       (["--where-document", '{"$regex": "a.*"}'], "$regex"),
                       (["--where-document", '{"$contains": ""}'], "non-empty string"),
                       (["--where-document", '{"$contains": 5}'], "must be a string"),
                       (["--where-document", '{"$and": []}'], "$and"),
                       (["--where-document", '{"$contains": "a", "$not_contains": "b"}'], "one operator"),
                       (["--where-document", "[]"], "non-empty dict"),
                       (["--where-document", '{"$contains": "' + "a" * 257 + '"}'], "257 bytes"),
                       (["--where-document", '{"$contains": "a"}', "--hybrid-alpha", "0.7"], "--hybrid-alpha")):
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma", "--queries", str(tmp_path / "q.txt")] + extra, model_factory=_boom)
        assert rc == 2
        out = capsys.readouterr().out
        assert msg in out and "--where-document" in out, out


def test_search_queries_refuses_where_document_with_hybrid_alpha():
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    with pytest.raises(ValueError, match="hybrid_alpha"):
        GEN.search_queries(None, [], None, ["q"], where_document={"$contains": "a"}, hybrid_alpha=0.5)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_text_scan_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    new = {"arx_text_contains", "arx_bitmap_count"}
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in new:
        assert hasattr(lib, name), name
    bound = _lib.load()
    assert bound.arx_version() == 112                          # purely additive
    # host-only argument checks (nothing is launched): what the entry points refuse
    one = ctypes.c_void_p(16)
    for args in ((one, one, 0, one, one, 1, one, None), (one, one, -5, one, one, 1, one, None), (one, one, 10, one, one, 0, one, None),
                 (one, one, 10, one, one, 33, one, None), (None, one, 10, one, one, 1, one, None), (one, None, 10, one, one, 1, one, None),
                 (one, one, 10, None, one, 1, one, None), (one, one, 10, one, None, 1, one, None), (one, one, 10, one, one, 1, None, None)):
        assert bound.arx_text_contains(*args) == -1, args
        assert bound.arx_last_error()
    assert b"n_pat=33" in (bound.arx_text_contains(one, one, 10, one, one, 33, one, None), bound.arx_last_error())[1]
    for args in ((one, 0, one, None), (None, 10, one, None), (one, 10, None, None)):
        assert bound.arx_bitmap_count(*args) == -1, args


def test_text_scan_kernels_do_not_spill_or_use_scratch():
    """What csrc/build.sh recorded for textscan.hip (as tests/test_build_resources.py reads it for every object)."""
    from tests.test_build_resources import BUILD, PAT
    f = BUILD / "textscan.resources.txt"
    assert f.exists(), "no _build/textscan.resources.txt: csrc/build.sh did not compile textscan.hip"
    ks = {m.group(1): (int(m.group(4)), int(m.group(7)), int(m.group(5))) for m in PAT.finditer(f.read_text())}
    for name in ("text_contains_kernel", "bitmap_count_kernel"):
        assert any(name in k for k in ks), name
    bad = {k: v for k, v in ks.items() if v[0] or v[1]}
    assert not bad, bad
    assert all(v[2] >= 4 for k, v in ks.items() if "text_contains_kernel" in k), ks       # a streaming kernel: latency is hidden by resident waves
