"""Host side of the BM25 index built on the device (CPU): the four new symbols of the C ABI, their argument errors before any launch,
the workspace formula, the build flags of the new file, the flattening of word-piece lists, `WordPieceTokenizer.full_pieces_flat`
against `_full_pieces`, and the opt-in flag of `HipCollection`, `search_queries` and the CLI."""
import ctypes
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd import keyword as KW

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_bm25_build_workspace_bytes": 3, "arx_bm25_build_postings": 13, "arx_bm25_build_postings_tuned": 15, "arx_bm25_build_impacts": 11}


def test_library_exports_the_new_symbols_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        decl = re.search(rf"\n(?:int32_t|int64_t) {name}\s*\(([^;]*)\);", hdr).group(1)
        assert len(_lib.EXPORTS[name][1]) == len(decl.split(",")) == n_args, name
    assert _lib.EXPORTS["arx_bm25_build_impacts"][1][8] is ctypes.c_double                # avgdl
    assert _lib.EXPORTS["arx_bm25_build_postings_tuned"][1][:12] == _lib.EXPORTS["arx_bm25_build_postings"][1][:12]
    assert hdr.index("arx_bm25_scores(") < hdr.index("arx_bm25_build_postings(") < hdr.index("arx_gemm_bf16(")      # in the BM25 section
    assert "Building the keyword index on the device" in (ROOT / "INTEGRATION.md").read_text()
    assert "build_postings_device" in (KW.__doc__ or "")


def test_workspace_formula_and_its_limits():
    from arxiv_rag_amd import _lib
    ws = _lib.load().arx_bm25_build_workspace_bytes
    for bad in ((-1, 1, 10), (1 << 31, 1, 10), (10, -1, 10), (10, 1 << 32, 10), (10, 1, 0), (10, 1, -5), (10, 1, (1 << 24) + 1)):
        assert ws(*bad) == -1, bad
    for n_tokens, n_docs, vocab in ((0, 0, 1), (1, 1, 1), (255, 3, 256), (256, 3, 257), (4_500_000, 50_000, 30522), ((1 << 31) - 1, (1 << 32) - 1, 1 << 24)):
        assert ws(n_tokens, n_docs, vocab) == 4 * (-(-4 * n_tokens // 256) * 256) + 4 * 256 * 2048, (n_tokens, n_docs, vocab)


def test_every_argument_error_is_refused_before_any_launch():
    """Nothing is launched: the pointers are never followed and the stream is null."""
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def post(pieces=one, n_tokens=1000, doc_ptr=one, n_docs=10, vocab=100, term_ptr=one, post_row=one, post_tf=one, n_post=one, bad=one, ws=one,
             ws_bytes=1 << 40, tile_tokens=0, max_blocks=0, tuned=True):
        if tuned:
            rc = lib.arx_bm25_build_postings_tuned(pieces, n_tokens, doc_ptr, n_docs, vocab, term_ptr, post_row, post_tf, n_post, bad, ws, ws_bytes,
                                                   tile_tokens, max_blocks, None)
        else:
            rc = lib.arx_bm25_build_postings(pieces, n_tokens, doc_ptr, n_docs, vocab, term_ptr, post_row, post_tf, n_post, bad, ws, ws_bytes, None)
        return rc, lib.arx_last_error().decode()

    for tuned in (True, False):
        for kw in (dict(pieces=None), dict(doc_ptr=None), dict(term_ptr=None), dict(post_row=None), dict(post_tf=None), dict(n_post=None),
                   dict(bad=None)):
            rc, msg = post(tuned=tuned, **kw)
            assert rc == -1 and "null pointer" in msg, (kw, msg)
        for kw, text in ((dict(n_tokens=-1), "n_tokens=-1"), (dict(n_tokens=1 << 31), "n_tokens=2147483648"), (dict(n_docs=-1), "n_docs=-1"),
                         (dict(n_docs=1 << 32), "n_docs=4294967296"), (dict(vocab=0), "vocab=0"), (dict(vocab=(1 << 24) + 1), "vocab=16777217"),
                         (dict(ws_bytes=64), "workspace too small"), (dict(ws=None), "workspace too small"),
                         (dict(ws_bytes=lib.arx_bm25_build_workspace_bytes(1000, 10, 100) - 1), "workspace too small")):
            rc, msg = post(tuned=tuned, **kw)
            assert rc == -1 and text in msg, (kw, msg)
    for kw, text in ((dict(tile_tokens=100), "tile_tokens=100"), (dict(tile_tokens=255), "tile_tokens=255"), (dict(tile_tokens=65536 + 256), "tile_tokens=65792"),
                     (dict(tile_tokens=-256), "tile_tokens=-256"), (dict(max_blocks=-1), "max_blocks=-1"), (dict(max_blocks=2049), "max_blocks=2049")):
        rc, msg = post(**kw)
        assert rc == -1 and text in msg, (kw, msg)

    def imp(term_ptr=one, post_row=one, post_tf=one, P=100, doc_ptr=one, n_docs=10, idf=one, vocab=100, avgdl=3.5, post_w=one):
        rc = lib.arx_bm25_build_impacts(term_ptr, post_row, post_tf, P, doc_ptr, n_docs, idf, vocab, avgdl, post_w, None)
        return rc, lib.arx_last_error().decode()

    for kw in (dict(term_ptr=None), dict(post_row=None), dict(post_tf=None), dict(doc_ptr=None), dict(idf=None), dict(post_w=None)):
        rc, msg = imp(**kw)
        assert rc == -1 and "null pointer" in msg, (kw, msg)
    for kw, text in ((dict(P=-1), "n_postings=-1"), (dict(P=1 << 31), "n_postings=2147483648"), (dict(n_docs=-1), "n_docs=-1"),
                     (dict(n_docs=1 << 32), "n_docs=4294967296"), (dict(vocab=0), "vocab=0"), (dict(vocab=(1 << 24) + 1), "vocab=16777217"),
                     (dict(avgdl=-1.0), "avgdl=-1"), (dict(avgdl=float("nan")), "avgdl=")):
        rc, msg = imp(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert imp(P=0)[0] == 0                                      # no postings: nothing to launch


def test_build_script_compiles_the_new_file_with_contraction_off():
    sh = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    loop = re.search(r"for f in ([^;]*); do", sh).group(1).split()
    assert "bm25_build" in loop and "$BLD/bm25_build.o" in sh.splitlines()[-2]
    per_file = re.search(r'PER_FILE="";(.*)&& PER_FILE="-ffp-contract=off"', sh).group(1)
    assert "$f = bm25_build" in per_file and "$f = fuse" in per_file
    assert "hipcc $FLAGS $PER_FILE" in sh                          # (after the default flags: the last -ffp-contract wins)
    src = (ROOT / "arxiv_rag_amd" / "csrc" / "bm25_build.hip").read_text()
    assert "#pragma clang fp contract(off)" in src
    assert f"BM25_K1 = {KW.BM25_K1}, BM25_B = {KW.BM25_B};" in src
    assert f"BLD_TILE = {KW.BUILD_TILE_TOKENS};" in src and f"BLD_NT = {KW.BUILD_ROUND_TOKENS};" in src


def test_new_kernels_do_not_spill():
    from tests.test_build_resources import BUILD, PAT
    f = BUILD / "bm25_build.resources.txt"
    if not f.exists():
        pytest.skip("no _build/*.resources.txt (library not built by csrc/build.sh in this tree)")
    ks = {m.group(1): (int(m.group(4)), int(m.group(7))) for m in PAT.finditer(f.read_text())}
    assert len(ks) == 9 and all(v == (0, 0) for v in ks.values()), ks


def test_flattening_matches_the_generator_path():
    rs = np.random.RandomState(3)
    for lists in ([], [[]], [[], [], []], [[5]], [rs.randint(0, 30522, size=rs.randint(0, 40)).tolist() for _ in range(200)],
                  [np.array([3, 1, 2], np.int64), (7, 7), []]):
        flat, doc_ptr = KW.flatten_pieces(lists)
        n = len(lists)
        dl = np.fromiter((len(p) for p in lists), np.int64, n)                           # as build_postings reads them
        terms = np.fromiter((t for p in lists for t in p), np.int64, int(dl.sum()))
        assert flat.dtype == np.int32 and doc_ptr.dtype == np.int64 and doc_ptr.shape == (n + 1,)
        assert np.array_equal(flat, terms) and np.array_equal(np.diff(doc_ptr), dl) and doc_ptr[0] == 0
    assert KW.flatten_pieces([[-1, 30522]])[0].tolist() == [-1, 30522]                    # range errors are build_postings_device's to raise
    with pytest.raises(ValueError):
        KW.flatten_pieces([[1 << 31]])


@pytest.mark.parametrize("cfg", [C.TINY_MPNET, C.TINY_BERT])
def test_full_pieces_flat_equals_full_pieces(cfg):
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from tests.helpers import synthetic_vocab
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1]
    rs = np.random.RandomState(5)
    texts = ["", "naïve café 中文 " + words[3], " ".join(words[:40]) + " !?", "   ", words[7]]
    texts += [" ".join(rs.choice(words, size=rs.randint(0, 25))) for _ in range(40)]
    texts.append(" ".join(rs.choice(words, size=700)))                                   # longer than the default piece cap (512)
    texts.append("über " + words[1])
    assert len(texts) % 7 != 0
    ref = tok._full_pieces(texts)
    assert len(ref[-2]) > WordPieceTokenizer.FLAT_PIECE_CAP and ref[0] == [] and max(map(len, ref[:-2])) > 16
    want_flat, want_ptr = KW.flatten_pieces(ref)
    # 7 does not divide the text count; a cap of 16 sends several rows of a batch to the HF path, first, middle and last ones included
    for kw in (dict(), dict(batch=7), dict(batch=7, piece_cap=16), dict(batch=1, piece_cap=1), dict(batch=len(texts)), dict(batch=10 ** 6, piece_cap=3)):
        flat, ptr = tok.full_pieces_flat(texts, **kw)
        assert flat.dtype == np.int32 and ptr.dtype == np.int64
        assert np.array_equal(ptr, want_ptr) and np.array_equal(flat, want_flat), kw
    flat, ptr = tok.full_pieces_flat([])
    assert flat.shape == (0,) and ptr.tolist() == [0]
    # without the native feeder: HF `tokenizers` alone
    plain = WordPieceTokenizer.from_vocab(vocab, cfg)
    plain._native = None
    flat, ptr = plain.full_pieces_flat(texts, batch=7)
    assert np.array_equal(ptr, want_ptr) and np.array_equal(flat, want_flat)
    with pytest.raises(ValueError):
        tok.full_pieces_flat(texts, batch=0)


def test_device_build_refuses_a_bad_doc_ptr_on_the_host():
    for flat, ptr in (([1, 2, 3], [0, 2]), ([1, 2, 3], [1, 3]), ([1, 2, 3], [0, 2, 1, 3]), ([1, 2, 3], [])):
        with pytest.raises(ValueError, match="doc_ptr must be non-decreasing"):
            KW.build_postings_device(np.array(flat, np.int32), np.array(ptr, np.int64), 10, device="cuda:0")


# ---- the opt-in flag ------------------------------------------------------------------------------------------------------------------
def test_collection_and_search_queries_refuse_the_flag_without_a_keyword_index():
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.store import HipCollection
    with pytest.raises(ValueError, match="keyword_build_on_device=True needs keyword=True"):
        HipCollection(np.zeros((4, 8), np.float32), [{}] * 4, keyword_build_on_device=True)
    with pytest.raises(ValueError, match="keyword_build_on_device needs hybrid_alpha"):
        GEN.search_queries(None, [], None, ["q"], keyword_build_on_device=True)
    with pytest.raises(AttributeError):                          # the checks pass; the (absent) model is reached
        GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, keyword_build_on_device=True)


def test_cli_flag(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    P = GEN.build_parser()
    assert P.parse_args(["in"]).keyword_build_on_device is False
    ok = P.parse_args(["in", "--hybrid-alpha", "0.7", "--keyword-build-on-device"])
    assert ok.keyword_build_on_device is True and GEN.check_keyword_build_args(ok) is None
    both = P.parse_args(["in", "--hybrid-alpha", "0.7", "--keyword-build-on-device", "--hybrid-on-device", "--hybrid-filters"])
    assert all(check(both) is None for check in (GEN.check_keyword_build_args, GEN.check_hybrid_device_args, GEN.check_hybrid_args))
    import argparse
    assert GEN.check_keyword_build_args(argparse.Namespace()) is None                     # partial namespaces, as other tests build them
    assert "needs --hybrid-alpha" in GEN.check_keyword_build_args(P.parse_args(["in", "--keyword-build-on-device"]))
    (tmp_path / "in").mkdir()
    (tmp_path / "q.txt").write_text("one query\n")

    def boom(name):
        raise AssertionError("the model must not be loaded")
    rc = GEN.main([str(tmp_path / "in"), "--skip-chroma", "--queries", str(tmp_path / "q.txt"), "--keyword-build-on-device"], model_factory=boom)
    assert rc == 2 and "--keyword-build-on-device needs --hybrid-alpha" in capsys.readouterr().out
