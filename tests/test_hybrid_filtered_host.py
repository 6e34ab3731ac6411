"""Host side of hybrid search under row filters (CPU): the two new symbols of the C ABI, every argument error of the C call before any
launch, the opt-in flag of `HipCollection`, `search_queries` and the CLI (every refusal unchanged without it), the resource figures of
the filtered kernel, and `KeywordIndex.search_distributed(allow=...)` with each rank's own bitmap over a world-2 gloo group."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_bm25_search_filtered", "arx_bm25_search_filtered_tuned"}
NO_FILTER = "the BM25 keyword search has no row filter"


def test_library_exports_the_filtered_search_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
    # three arguments more than the unfiltered calls, as the header declares them
    for name, base in (("arx_bm25_search_filtered", "arx_bm25_search"), ("arx_bm25_search_filtered_tuned", "arx_bm25_search_tuned")):
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", hdr).group(1)
        assert len(_lib.EXPORTS[name][1]) == len(decl.split(",")) == len(_lib.EXPORTS[base][1]) + 3, name
    assert len(_lib.EXPORTS["arx_bm25_search_filtered"][1]) == 18 and len(_lib.EXPORTS["arx_bm25_search_filtered_tuned"][1]) == 20
    assert _lib.load().arx_version() == 112                    # purely additive
    assert "Hybrid search with filters" in (ROOT / "INTEGRATION.md").read_text()


def test_every_argument_error_is_refused_before_any_launch_with_the_field_named():
    """Nothing is launched: the pointers are never followed and the stream is null."""
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def call(term_ptr=one, post_row=one, post_w=one, vocab=100, n_rows=5000, allow=one, n_filters=1, filter_of=None, q_terms=one, q_nterms=one,
             nq=4, n=10, out_s=one, out_i=one, idx_base=0, ws=one, ws_bytes=1 << 40, tile_rows=0, max_blocks=0, tuned=True):
        head = (term_ptr, post_row, post_w, vocab, n_rows, allow, n_filters, filter_of, q_terms, q_nterms, nq, n, out_s, out_i, idx_base, ws,
                ws_bytes)
        rc = lib.arx_bm25_search_filtered_tuned(*head, tile_rows, max_blocks, None) if tuned else lib.arx_bm25_search_filtered(*head, None)
        return rc, lib.arx_last_error().decode()

    for tuned in (True, False):
        for kw in (dict(term_ptr=None), dict(post_row=None), dict(post_w=None), dict(q_terms=None), dict(q_nterms=None), dict(out_s=None),
                   dict(out_i=None)):
            rc, msg = call(tuned=tuned, **kw)
            assert rc == -1 and "null pointer" in msg, (kw, msg)
        for kw, text in ((dict(allow=None), "allow"), (dict(n_filters=0), "n_filters=0"), (dict(n_filters=-2), "n_filters=-2"),
                         (dict(vocab=0), "vocab=0"), (dict(n_rows=0), "n_rows=0"), (dict(n_rows=1 << 31), "n_rows=2147483648"),
                         (dict(nq=0), "n_queries=0"), (dict(nq=65536), "n_queries=65536"), (dict(n=0), "n=0"), (dict(n=33), "n=33"),
                         (dict(idx_base=-1), "idx_base"), (dict(ws_bytes=64, n_rows=50000), "workspace too small"),
                         (dict(ws=None, n_rows=50000), "workspace too small")):
            rc, msg = call(tuned=tuned, **kw)
            assert rc == -1 and text in msg, (kw, msg)
    for kw, text in ((dict(max_blocks=-1), "max_blocks"), (dict(tile_rows=1000), "tile_rows=1000"), (dict(tile_rows=512), "tile_rows=512"),
                     (dict(tile_rows=13312), "tile_rows=13312")):
        rc, msg = call(**kw)
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


FILTER_CASES = ((dict(where={"a": 1}), "where cannot be combined with hybrid_alpha: " + NO_FILTER),
                (dict(where=[{"a": 1}, None]), "where cannot be combined with hybrid_alpha: " + NO_FILTER),
                (dict(where_document=[{"$contains": "a"}, None]), "where cannot be combined with hybrid_alpha: " + NO_FILTER),
                (dict(where_document={"$contains": "a"}), "where_document cannot be combined with hybrid_alpha: " + NO_FILTER))
DEDUP_TEXT = "a collection built with dedup_threshold cannot be queried with hybrid_alpha: " + NO_FILTER


def test_collection_refusals_are_unchanged_without_the_flag_and_lifted_with_it():
    from arxiv_rag_amd.store import HipCollection
    hy = dict(query_texts=["a", "b"], hybrid_alpha=0.7)
    for coll in (_collection_without_a_device(), _collection_without_a_device(hybrid_filters=False)):
        for kw, text in FILTER_CASES:
            with pytest.raises(ValueError) as e:
                coll.query(**hy, **kw)
            assert str(e.value) == text, kw
    with pytest.raises(ValueError) as e:
        _collection_without_a_device(_keep=object()).query(**hy)
    assert str(e.value) == DEDUP_TEXT
    # with the flag the same calls pass the filter checks (and stop where the query would be encoded: there is no encoder here)
    flagged = _collection_without_a_device(hybrid_filters=True, documents=object(), _keep=object())
    for kw, _ in FILTER_CASES + ((dict(), None),):
        with pytest.raises(ValueError, match="pass query_embeddings, or query_texts with an encoder"):
            flagged.query(**hy, **kw)
    # what stays refused either way
    q = np.zeros((2, 64), np.float16)
    for kw, text in ((dict(mmr_lambda=0.5), "mmr_lambda cannot be combined with reranker or hybrid_alpha"),
                     (dict(group_by=True), "group_by cannot be combined with hybrid_alpha"),
                     (dict(min_score=0.5), "min_score cannot be combined with hybrid_alpha")):
        with pytest.raises(ValueError, match=text):
            _collection_without_a_device(hybrid_filters=True, group_key="paper_id").query(query_embeddings=q, where={"a": 1}, **hy, **kw)
    with pytest.raises(ValueError, match="hybrid_filters=True needs keyword=True"):
        HipCollection(np.zeros((4, 8), np.float32), [{}] * 4, hybrid_filters=True)


def test_search_queries_refusals_are_unchanged_without_the_flag(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cases = ((dict(where={"a": 1}), "where cannot be combined with hybrid_alpha: " + NO_FILTER),
             (dict(where=[{"a": 1}]), "where cannot be combined with hybrid_alpha: " + NO_FILTER),
             (dict(where_document={"$contains": "a"}), "where_document cannot be combined with hybrid_alpha: " + NO_FILTER),
             (dict(keep_mask=np.ones(3, bool)), "keep_mask cannot be combined with hybrid_alpha: " + NO_FILTER))
    for kw, text in cases:
        for flag in ({}, dict(hybrid_filters=False)):
            with pytest.raises(ValueError) as e:
                GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, **kw, **flag)
            assert str(e.value) == text, kw
        with pytest.raises(AttributeError):                    # with the flag the checks pass; the (absent) model is reached
            GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, hybrid_filters=True, **kw)
    for kw, text in ((dict(mmr_lambda=0.5), "mmr_lambda"), (dict(group_by_paper=True), "group_by"), (dict(min_score=0.5), "min_score")):
        with pytest.raises(ValueError, match=text):
            GEN.search_queries(None, [], None, ["q"], hybrid_alpha=0.7, hybrid_filters=True, where={"a": 1}, **kw)


def _boom(name):
    raise AssertionError("the model must not be loaded")


def test_cli_flag_is_off_by_default_and_checked_before_any_model_is_loaded(tmp_path, capsys, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    P = GEN.build_parser()
    args = P.parse_args(["in"])
    assert args.hybrid_filters is False and GEN.check_hybrid_filters_args(args) is None
    assert GEN.check_hybrid_filters_args(argparse.Namespace()) is None           # partial namespaces, as other tests build them
    (tmp_path / "in").mkdir()
    (tmp_path / "q.txt").write_text("one query\n")
    (tmp_path / "w.jsonl").write_text('{"section": "abstract"}\n')
    q = ["--queries", str(tmp_path / "q.txt")]
    where = ["--where", '{"section": "abstract"}']
    # the flag alone, without --hybrid-alpha, or without a filter: refused before any model is loaded
    for extra, msg in ((["--hybrid-filters"], "needs --hybrid-alpha"),
                       (q + ["--hybrid-filters"], "needs --hybrid-alpha"),
                       (q + where + ["--hybrid-filters"], "needs --hybrid-alpha"),
                       (q + ["--hybrid-filters", "--hybrid-alpha", "0.7"], "needs --where, --where-file, --where-document or --dedup-threshold")):
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma"] + extra, model_factory=_boom)
        out = capsys.readouterr().out
        assert rc == 2 and msg in out and "--hybrid-filters" in out, (extra, out)
    # without the flag every combination is refused with the old text
    old = ((where, "--where cannot be combined with --hybrid-alpha: " + NO_FILTER),
           (["--where-file", str(tmp_path / "w.jsonl")], "--where-file cannot be combined with --hybrid-alpha: " + NO_FILTER),
           (["--where-document", '{"$contains": "a"}'], "--where-document cannot be combined with --hybrid-alpha: " + NO_FILTER),
           (["--dedup-threshold", "0.9"], "--dedup-threshold cannot be combined with --hybrid-alpha and --queries: " + NO_FILTER))
    for extra, msg in old:
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma", "--hybrid-alpha", "0.7"] + q + extra, model_factory=_boom)
        assert rc == 2 and f"Error: {msg}\n" == capsys.readouterr().out, extra
    # with it they pass every check
    checks = (GEN.check_rerank_args, GEN.check_hybrid_args, GEN.check_hybrid_filters_args, GEN.check_where_args, GEN.check_where_file_args,
              GEN.check_where_device_args, GEN.check_where_document_args, GEN.check_mmr_args, GEN.check_dedup_args, GEN.check_group_args,
              GEN.check_range_args)
    for extra, _ in old:
        args = P.parse_args(["in", "--hybrid-alpha", "0.7", "--hybrid-filters"] + q + extra)
        assert [c(args) for c in checks] == [None] * len(checks), extra
    # still refused next to the flag
    for extra, msg in ((["--mmr-lambda", "0.5"], "--mmr-lambda"), (["--group-by-paper"], "--group-by-paper"), (["--min-score", "0.5"], "--min-score")):
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma", "--hybrid-alpha", "0.7", "--hybrid-filters"] + q + where + extra, model_factory=_boom)
        assert rc == 2 and msg in capsys.readouterr().out, extra


def test_check_dedup_args_with_the_flag_returns_none_where_it_returns_the_message_today(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bare = argparse.Namespace(dedup_threshold=0.9, hybrid_alpha=0.7, queries="q.txt")
    assert GEN.check_dedup_args(bare) == "--dedup-threshold cannot be combined with --hybrid-alpha and --queries: " + NO_FILTER
    assert GEN.check_dedup_args(argparse.Namespace(**vars(bare), hybrid_filters=False)) == GEN.check_dedup_args(bare)
    assert GEN.check_dedup_args(argparse.Namespace(**vars(bare), hybrid_filters=True)) is None
    # bare namespaces of the other checks: absent = off, the old message
    assert NO_FILTER in GEN.check_where_args(argparse.Namespace(where="{}", hybrid_alpha=0.7))
    assert NO_FILTER in GEN.check_where_document_args(argparse.Namespace(where_document="{}", hybrid_alpha=0.7))
    assert NO_FILTER in GEN.check_where_file_args(argparse.Namespace(where_file="f", where=None, hybrid_alpha=0.7))


def test_keyword_search_refuses_wrong_bitmaps_on_the_host():
    """`_check_filters` needs no launch: shapes, dtypes and devices are compared on the host."""
    torch = pytest.importorskip("torch")
    from arxiv_rag_amd.keyword import KeywordIndex
    idx = object.__new__(KeywordIndex)
    idx.n_rows, idx.device = 130, torch.device("cpu")
    ok = torch.zeros(3, dtype=torch.int64)
    allow, fo = idx._check_filters(ok, None, 5)
    assert allow.shape == (1, 3) and fo is None
    allow, fo = idx._check_filters(torch.zeros((4, 3), dtype=torch.int64), torch.zeros(5, dtype=torch.int32), 5)
    assert allow.shape == (4, 3) and fo.shape == (5,)
    for bad_allow, bad_fo in ((torch.zeros(2, dtype=torch.int64), None), (torch.zeros(3, dtype=torch.int32), None), (np.zeros(3, np.int64), None),
                              (torch.zeros((0, 3), dtype=torch.int64), None), (torch.zeros((2, 2, 3), dtype=torch.int64), None),
                              (ok, torch.zeros(5, dtype=torch.int64)), (ok, torch.zeros(4, dtype=torch.int32)), (ok, [0] * 5),
                              (ok, torch.zeros((5, 1), dtype=torch.int32))):
        with pytest.raises(ValueError, match="allow|filter_of"):
            idx._check_filters(bad_allow, bad_fo, 5)


def test_filtered_kernel_does_not_spill_or_use_scratch():
    """What csrc/build.sh recorded for bm25.hip (as tests/test_build_resources.py reads it for every object)."""
    from tests.test_build_resources import BUILD, PAT
    f = BUILD / "bm25.resources.txt"
    if not f.exists():
        pytest.skip("no _build/bm25.resources.txt (library not built by csrc/build.sh in this tree)")
    ks = {m.group(1): (int(m.group(4)), int(m.group(7)), int(m.group(5))) for m in PAT.finditer(f.read_text())}
    search = {k: v for k, v in ks.items() if "bm25_search_kernel" in k}
    assert len(search) == 2 and any("ILb1E" in k for k in search) and any("ILb0E" in k for k in search), list(ks)   # <true> and <false>
    assert all(v[0] == 0 and v[1] == 0 for v in search.values()), search
    # two 8-wave blocks per CU (the LDS budget of the default 10240-row tile) need 4 waves per SIMD
    assert all(v[2] >= 4 for v in search.values()), search


# ---- world size 2 (gloo, CPU tensors) -----------------------------------------------------------------------------------------------
# The kernel needs a GPU; what is under test here is `search_distributed(allow=, filter_of=)`: every rank applies ITS OWN bitmaps and the
# merge is unchanged.  `KeywordIndex.search` and the merge kernel are replaced by numpy statements of their definitions, the exchange
# (`gather_partials`) is the real one.
_WORKER = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, os.environ["ARX_ROOT"])
import torch
import torch.distributed as dist
from arxiv_rag_amd import index as IX, keyword as KW
from arxiv_rag_amd.index import shard_bounds
from arxiv_rag_amd.where import pack_bitmap
from tests import bm25_fp64 as R

V, N_DOCS, n = 97, 211, 8
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
docs = R.zipf_corpus(N_DOCS, V, 23, seed=11, empty_every=17)
lo, hi = shard_bounds(len(docs), world, rank)
stats = KW.KeywordStats.from_pieces(docs[lo:hi], V).all_reduce(KW._host_group())
term_ptr, rows, tf, dl = KW.build_postings(docs[lo:hi], V)
w32 = KW.impacts_f64(term_ptr, rows, tf, dl, stats).astype(np.float32)
rs = np.random.RandomState(3)
masks = np.stack([rs.rand(N_DOCS) < p for p in (0.5, 0.1, 1.0)])          # GLOBAL masks; a rank packs its own slice
filter_of = [0, 1, 2, 1, 0, 5]                                              # (5: outside [0, 3) -> no row)
queries = [[3, 9], [1], [2, 5, 40], [3, 9], [0, 1, 2, 3, 4, 5, 6, 7], [1]]
seen = {}

def topn(s32, ok, base):
    cand = np.flatnonzero(ok)
    order = cand[np.lexsort((cand, -s32[cand].astype(np.float64)))][:n]
    s = np.full(n, -np.inf, np.float32); i = np.full(n, -1, np.int64)
    s[:len(order)], i[:len(order)] = s32[order], order + base
    return s, i

def numpy_search(self, queries, n=n, tile_rows=0, max_blocks=0, allow=None, filter_of=None):
    allow, filter_of = self._check_filters(allow, filter_of, len(queries))
    seen["allow"], seen["filter_of"] = allow.numpy().view(np.uint64).copy(), filter_of.numpy().copy()
    out = []
    for q, f in zip(queries, filter_of.tolist()):
        s32 = np.zeros(self.n_rows, np.float32); has = np.zeros(self.n_rows, bool)
        for t in sorted(q):
            a, b = term_ptr[t], term_ptr[t + 1]
            s32[rows[a:b]] += w32[a:b]; has[rows[a:b]] = True
        ok = np.zeros(self.n_rows, bool)
        if 0 <= f < allow.shape[0]:
            ok = np.unpackbits(allow[f].numpy().view(np.uint8), bitorder="little")[:self.n_rows].astype(bool)
        out.append(topn(s32, has & ok, self.idx_base))
    return torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out]))

def numpy_merge(all_s, all_i, k):
    S = all_s.numpy().transpose(1, 0, 2).reshape(all_s.shape[1], -1); I = all_i.numpy().transpose(1, 0, 2).reshape(all_s.shape[1], -1)
    out_s = np.full((S.shape[0], k), -np.inf, np.float32); out_i = np.full((S.shape[0], k), -1, np.int64)
    for q in range(S.shape[0]):
        keep = np.flatnonzero(I[q] >= 0)
        order = keep[np.lexsort((I[q][keep], -S[q][keep].astype(np.float64)))][:k]
        out_s[q, :len(order)], out_i[q, :len(order)] = S[q][order], I[q][order]
    return torch.from_numpy(out_s), torch.from_numpy(out_i)

KW.KeywordIndex.search = numpy_search
IX.merge_partials = numpy_merge
idx = object.__new__(KW.KeywordIndex)
idx.n_rows, idx.idx_base, idx.device = hi - lo, lo, torch.device("cpu")
mine = torch.from_numpy(np.stack([pack_bitmap(m[lo:hi]) for m in masks]).view(np.int64))
s, i = idx.search_distributed(queries, n, allow=mine, filter_of=torch.tensor(filter_of, dtype=torch.int32))
assert np.array_equal(seen["allow"], np.stack([pack_bitmap(m[lo:hi]) for m in masks])) and seen["filter_of"].tolist() == filter_of
if rank == world - 1:
    print("RESULT", json.dumps([s.numpy().astype(np.float64).tolist(), i.numpy().tolist()]).replace("-Infinity", "null"))
dist.barrier()
dist.destroy_process_group()
'''


def _run_world(tmp_path, world):
    w = tmp_path / f"worker{world}.py"
    w.write_text(_WORKER)
    env = {**os.environ, "ARX_ROOT": str(ROOT), "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", f"--nproc-per-node={world}", "--master-port", str(29760 + world), str(w)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0][len("RESULT "):])


def test_search_distributed_with_each_ranks_own_bitmap_world_2_gloo_equals_the_single_index(tmp_path):
    one, two = _run_world(tmp_path, 1), _run_world(tmp_path, 2)
    assert two == one
    scores, ids = one
    assert ids[5] == [-1] * 8 and scores[5] == [None] * 8          # filter_of outside [0, n_filters): no row
    assert ids[0] != ids[3] and ids[0][0] >= 0 and ids[2][0] >= 0    # the same query under two filters; real hits
    # the single-index answer is the definition's: every hit is allowed by its query's global mask
    rs = np.random.RandomState(3)
    masks = np.stack([rs.rand(211) < p for p in (0.5, 0.1, 1.0)])
    for q, f in enumerate([0, 1, 2, 1, 0]):
        assert all(masks[f][r] for r in ids[q] if r >= 0), q
