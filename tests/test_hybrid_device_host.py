"""Host side of hybrid search on the device (CPU): the three new symbols of the C ABI, their argument errors before any launch, the
workspace formula, the opt-in flag of `retrieve`, `HipCollection`, `search_queries` and the CLI (every limit and message of today
unchanged without it), and the resource figures of the new kernels."""
import argparse
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_bm25_search_wide", "arx_bm25_wide_workspace_bytes", "arx_hybrid_fuse"}


def test_library_exports_the_new_symbols_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
        decl = re.search(rf"\n(?:int32_t|int64_t) {name}\s*\(([^;]*)\);", hdr).group(1)
        assert len(_lib.EXPORTS[name][1]) == len(decl.split(",")), name
    assert len(_lib.EXPORTS["arx_bm25_search_wide"][1]) == len(_lib.EXPORTS["arx_bm25_search_filtered_tuned"][1]) == 20
    assert _lib.EXPORTS["arx_hybrid_fuse"][1][7] is ctypes.c_double                      # alpha
    assert "distinct" in hdr and "Hybrid search on the device" in (ROOT / "INTEGRATION.md").read_text()


def test_wide_workspace_formula_and_its_limits():
    from arxiv_rag_amd import _lib
    ws = _lib.load().arx_bm25_wide_workspace_bytes
    for bad in ((1000, 4, 0), (1000, 4, 1025), (1000, 4, -1), (0, 4, 10), (1000, 0, 10)):
        assert ws(*bad) == -1, bad
    for n_rows, nq, n in ((1, 1, 1), (1000, 4, 32), (5000, 3, 1024), (10 ** 6, 64, 1024), (10 ** 6, 64, 50), (10 ** 6, 1, 1)):
        blocks = min(-(-n_rows // 1024), 512, 65536 // n)
        assert ws(n_rows, nq, n) == -(-blocks * nq * n * 8 // 256) * 256, (n_rows, nq, n)
    assert ws(10 ** 6, 1, 1024) == 64 * 1024 * 8                 # a single query still spreads over 64 blocks at n = 1024


def test_every_argument_error_is_refused_before_any_launch_with_the_field_named():
    """Nothing is launched: the pointers are never followed and the stream is null."""
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def wide(term_ptr=one, post_row=one, post_w=one, vocab=100, n_rows=5000, allow=None, n_filters=0, filter_of=None, q_terms=one, q_nterms=one,
             nq=4, n=50, out_s=one, out_i=one, idx_base=0, ws=one, ws_bytes=1 << 40, tile_rows=0, max_blocks=0):
        rc = lib.arx_bm25_search_wide(term_ptr, post_row, post_w, vocab, n_rows, allow, n_filters, filter_of, q_terms, q_nterms, nq, n, out_s,
                                      out_i, idx_base, ws, ws_bytes, tile_rows, max_blocks, None)
        return rc, lib.arx_last_error().decode()

    for kw in (dict(term_ptr=None), dict(post_row=None), dict(post_w=None), dict(q_terms=None), dict(q_nterms=None), dict(out_s=None),
               dict(out_i=None)):
        rc, msg = wide(**kw)
        assert rc == -1 and "null pointer" in msg, (kw, msg)
    for kw, text in ((dict(filter_of=one), "filter_of needs allow"), (dict(allow=one, n_filters=0), "n_filters=0"), (dict(vocab=0), "vocab=0"),
                     (dict(n_rows=0), "n_rows=0"), (dict(n_rows=1 << 31), "n_rows=2147483648"), (dict(nq=0), "n_queries=0"),
                     (dict(nq=65536), "n_queries=65536"), (dict(n=0), "n=0"), (dict(n=1025), "n=1025"), (dict(idx_base=-1), "idx_base"),
                     (dict(max_blocks=-1), "max_blocks"), (dict(tile_rows=1000), "tile_rows=1000"), (dict(tile_rows=13312), "tile_rows=13312"),
                     (dict(ws_bytes=64, n_rows=50000), "workspace too small"), (dict(ws=None, n_rows=50000), "workspace too small")):
        rc, msg = wide(**kw)
        assert rc == -1 and text in msg, (kw, msg)

    def fuse(ds=one, di=one, n_dense=32, ks=one, ki=one, n_kw=32, nq=2, alpha=0.7, k=10, of=one, oi=one, od=one, ok=one):
        rc = lib.arx_hybrid_fuse(ds, di, n_dense, ks, ki, n_kw, nq, alpha, k, of, oi, od, ok, None)
        return rc, lib.arx_last_error().decode()

    for kw in (dict(ds=None), dict(di=None), dict(ks=None), dict(ki=None), dict(of=None), dict(oi=None), dict(od=None), dict(ok=None)):
        rc, msg = fuse(**kw)
        assert rc == -1 and "null pointer" in msg, (kw, msg)
    for kw, text in ((dict(n_dense=0), "n_dense=0"), (dict(n_dense=1025), "n_dense=1025"), (dict(n_kw=0), "n_kw=0"), (dict(n_kw=1025), "n_kw=1025"),
                     (dict(k=0), "k=0"), (dict(k=1025), "k=1025"), (dict(nq=0), "n_queries=0"), (dict(alpha=1.5), "alpha=1.5"),
                     (dict(alpha=-0.1), "alpha=-0.1"), (dict(alpha=float("nan")), "alpha=")):
        rc, msg = fuse(**kw)
        assert rc == -1 and text in msg, (kw, msg)


# ---- the opt-in flag ------------------------------------------------------------------------------------------------------------------
class _Keyword:
    """Stands where a KeywordIndex would: a query that passes every check reaches the encoder, which is absent."""


def _collection_without_a_device(**attrs):
    from arxiv_rag_amd.store import HipCollection
    coll = object.__new__(HipCollection)
    coll.group_key, coll.world, coll._keep, coll.documents, coll.keyword, coll.encoder = None, 1, None, None, _Keyword(), None
    for k, v in attrs.items():
        setattr(coll, k, v)
    return coll


TODAY_33 = "n_candidates=33 must be in [n_results, 32] (the candidate lists' length limit)"
ENCODER = "pass query_embeddings, or query_texts with an encoder"


def test_collection_limits_are_unchanged_without_the_flag_and_lifted_with_it():
    from arxiv_rag_amd.store import HipCollection
    hy = dict(query_texts=["a", "b"], hybrid_alpha=0.7)
    for coll in (_collection_without_a_device(), _collection_without_a_device(hybrid_on_device=False)):
        with pytest.raises(ValueError) as e:
            coll.query(**hy, n_candidates=33)
        assert str(e.value) == TODAY_33
        with pytest.raises(ValueError) as e:
            coll.query(**hy, n_candidates=50, reranker=object())
        assert str(e.value) == "n_candidates=50 must be in [n_results, 32] (the candidate lists' length limit)"
        with pytest.raises(ValueError, match="min_score cannot be combined with hybrid_alpha"):      # the only other way to 50 candidates
            coll.query(**hy, n_candidates=50, reranker=object(), min_score=float("-inf"))
    flagged = _collection_without_a_device(hybrid_on_device=True)
    for kw in (dict(n_candidates=33), dict(n_candidates=50, reranker=object()), dict(n_candidates=1024, n_results=1024), dict()):
        with pytest.raises(ValueError, match=ENCODER):           # every check passes; the (absent) encoder is reached
            flagged.query(**hy, **kw)
    # the new refusals, each with its reason
    with pytest.raises(ValueError, match=r"n_candidates=1025 must be at most 1024 with hybrid_on_device"):
        flagged.query(**hy, n_candidates=1025)
    with pytest.raises(ValueError, match=r"n_candidates=9 must be in \[n_results, 1024\]"):
        flagged.query(**hy, n_candidates=9)
    with pytest.raises(ValueError, match=r"n_candidates=50 > 32 needs a single GPU rank: a cross-rank merge of long candidate lists is out of scope"):
        _collection_without_a_device(hybrid_on_device=True, world=2).query(**hy, n_candidates=50)
    both = _collection_without_a_device(hybrid_on_device=True, hybrid_filters=True)
    with pytest.raises(ValueError, match=r"n_candidates=50 > 32 cannot be combined with per-query filter lists: the range search .* one bitmap per call"):
        both.query(**hy, n_candidates=50, where=[{"a": 1}, None])
    with pytest.raises(ValueError, match=ENCODER):               # up to 32 candidates per-query lists and more ranks stay allowed
        both.query(**hy, n_candidates=32, where=[{"a": 1}, None])
    with pytest.raises(ValueError, match=ENCODER):
        _collection_without_a_device(hybrid_on_device=True, world=2).query(**hy, n_candidates=32)
    # what stays refused with hybrid_alpha either way
    q = np.zeros((2, 64), np.float16)
    for kw, text in ((dict(mmr_lambda=0.5), "mmr_lambda cannot be combined with reranker or hybrid_alpha"),
                     (dict(group_by=True), "group_by cannot be combined with hybrid_alpha"),
                     (dict(min_score=0.5), "min_score cannot be combined with hybrid_alpha"),
                     (dict(where={"a": 1}), "where cannot be combined with hybrid_alpha: the BM25 keyword search has no row filter")):
        with pytest.raises(ValueError, match=text):
            _collection_without_a_device(hybrid_on_device=True, group_key="paper_id").query(query_embeddings=q, n_candidates=50, **hy, **kw)
    # without hybrid_alpha the flag changes nothing
    with pytest.raises(ValueError, match=r"n_candidates=50 must be in \[n_results, 32\] \(the search's k limit\)"):
        flagged.query(query_texts=["a"], reranker=object(), n_candidates=50)
    with pytest.raises(ValueError, match="hybrid_on_device=True needs keyword=True"):
        HipCollection(np.zeros((4, 8), np.float32), [{}] * 4, hybrid_on_device=True)


def test_retrieve_refuses_before_it_touches_the_index():
    from arxiv_rag_amd.retrieval import check_hybrid_on_device, retrieve
    q = np.zeros((2, 8), np.float16)
    for kw, text in ((dict(n_candidates=1025), "at most 1024"), (dict(n_candidates=33, where=[{"a": 1}, None]), "per-query filter lists"),
                     (dict(n_candidates=33, where_document=[None, {"$contains": "x"}]), "per-query filter lists"),
                     (dict(n_candidates=33, world=2), "single GPU rank")):
        with pytest.raises(ValueError, match=text):
            retrieve(None, q, None, 10, hybrid_alpha=0.7, hybrid_on_device=True, **kw)
    assert check_hybrid_on_device(1024) is None and check_hybrid_on_device(32, per_query_filters=True, world=4) is None


def test_search_queries_and_cli_flag(tmp_path, capsys, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="hybrid_on_device needs hybrid_alpha"):
        GEN.search_queries(None, [], None, ["q"], hybrid_on_device=True)
    with pytest.raises(ValueError, match="at most 1024"):
        GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, hybrid_on_device=True, reranker=object(), rerank_top_k=2000)
    with pytest.raises(ValueError, match="per-query filter lists"):
        GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, hybrid_on_device=True, hybrid_filters=True, reranker=object(), rerank_top_k=50,
                           where=[{"a": 1}])
    with pytest.raises(AttributeError):                          # the checks pass; the (absent) model is reached
        GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, hybrid_on_device=True, reranker=object(), rerank_top_k=50)
    P = GEN.build_parser()
    assert P.parse_args(["in"]).hybrid_on_device is False
    assert GEN.check_hybrid_device_args(argparse.Namespace()) is None              # partial namespaces, as other tests build them
    recipe = ["--hybrid-alpha", "0.7", "--rerank-model", "m", "--rerank-top-k", "50", "--top-k", "10"]
    today = "--rerank-top-k 50: the search returns at most k <= 32 candidates per query"
    assert GEN.check_rerank_args(P.parse_args(["in"] + recipe)) == today
    assert GEN.check_rerank_args(argparse.Namespace(rerank_model="m", rerank_top_k=50, top_k=10)) == today
    assert GEN.check_rerank_args(P.parse_args(["in", "--rerank-model", "m", "--rerank-top-k", "50", "--hybrid-on-device"])) == today   # no --hybrid-alpha
    ok = P.parse_args(["in"] + recipe + ["--hybrid-on-device"])
    assert GEN.check_rerank_args(ok) is None and GEN.check_hybrid_args(ok) is None and GEN.check_hybrid_device_args(ok) is None
    assert "1024" in GEN.check_rerank_args(P.parse_args(["in"] + recipe[:4] + ["--rerank-top-k", "1025", "--hybrid-on-device"]))
    assert GEN.check_rerank_args(P.parse_args(["in"] + recipe[:4] + ["--rerank-top-k", "1024", "--top-k", "10", "--hybrid-on-device"])) is None
    # refused before any model is loaded
    (tmp_path / "in").mkdir()
    (tmp_path / "q.txt").write_text("one query\n")
    (tmp_path / "w.jsonl").write_text('{"section": "abstract"}\n')

    def boom(name):
        raise AssertionError("the model must not be loaded")
    head = [str(tmp_path / "in"), "--skip-chroma", "--queries", str(tmp_path / "q.txt")]
    for extra, msg in ((["--hybrid-on-device"], "--hybrid-on-device needs --hybrid-alpha"),
                       (recipe, today),
                       (recipe + ["--hybrid-on-device", "--hybrid-filters", "--where-file", str(tmp_path / "w.jsonl")], "cannot be combined with --where-file")):
        rc = GEN.main(head + extra, model_factory=boom)
        assert rc == 2 and msg in capsys.readouterr().out, extra
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in GEN.check_hybrid_device_args(ok)
    assert GEN.check_hybrid_device_args(P.parse_args(["in", "--hybrid-alpha", "0.7", "--rerank-model", "m", "--hybrid-on-device"])) is None


def test_new_kernels_do_not_spill_and_keep_two_blocks_per_cu():
    """What csrc/build.sh recorded for bm25.hip and fuse.hip (as tests/test_build_resources.py reads it for every object)."""
    from tests.test_build_resources import BUILD, PAT
    if not (BUILD / "bm25.resources.txt").exists() or not (BUILD / "fuse.resources.txt").exists():
        pytest.skip("no _build/*.resources.txt (library not built by csrc/build.sh in this tree)")
    ks = {}
    for f in ("bm25.resources.txt", "fuse.resources.txt"):
        ks.update({m.group(1): (int(m.group(4)), int(m.group(7)), int(m.group(5))) for m in PAT.finditer((BUILD / f).read_text())})
    wide = {k: v for k, v in ks.items() if "bm25_search_kernel" in k}          # the one top-n kernel: arx_bm25_search_wide runs it too
    assert len(wide) == 2 and any("ILb1E" in k for k in wide) and any("ILb0E" in k for k in wide), list(ks)
    new = {**wide, **{k: v for k, v in ks.items() if "bm25_merge_kernel" in k or "hybrid_fuse_kernel" in k}}
    assert len(new) == 4 and all(v[0] == 0 and v[1] == 0 for v in new.values()), new
    assert all(v[2] >= 4 for v in wide.values()), wide        # two 8-wave blocks per CU (the LDS budget of the 10240-row tile)
