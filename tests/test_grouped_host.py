"""Host side of the grouped search (CPU): the runs of a metadata key and the reappearing-key error (arxiv_rag_amd/grouping.py), every
refusal of `HipCollection.query(group_by=True)`, of `search_queries(group_by_paper=True)` and of the CLI's --group-by-paper checks, the
C ABI's new symbols with the workspace function's -1 cases, and S and K of the exactness argument against a brute-force count."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd.grouping import check_grouped_query, groups_touched, runs_from_keys, select_count

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_topk_grouped_workspace_bytes", "arx_topk_search_grouped", "arx_topk_search_grouped_tuned", "arx_topk_grouped_stats",
       "arx_group_runs_info"}


def test_runs_are_consecutive_equal_keys():
    group_of, keys = runs_from_keys(["a", "a", "b", "c", "c", "c", None, None, "d"])
    assert group_of.dtype == np.int32 and group_of.tolist() == [0, 0, 1, 2, 2, 2, 3, 3, 4] and keys == ["a", "b", "c", None, "d"]
    group_of, keys = runs_from_keys([])
    assert group_of.shape == (0,) and keys == []
    group_of, keys = runs_from_keys(["x"] * 5)
    assert group_of.tolist() == [0] * 5 and keys == ["x"]
    rs = np.random.RandomState(0)
    lengths = rs.randint(1, 9, size=300)
    group_of, keys = runs_from_keys([f"p{j}" for j, ln in enumerate(lengths) for _ in range(ln)])
    assert np.array_equal(group_of, np.repeat(np.arange(300), lengths)) and keys == [f"p{j}" for j in range(300)]


def test_a_key_that_reappears_after_its_run_ended_names_the_key_and_both_rows():
    with pytest.raises(ValueError) as e:
        runs_from_keys(["a", "a", "b", "a"])
    assert "'a'" in str(e.value) and "row 1" in str(e.value) and "row 3" in str(e.value)
    with pytest.raises(ValueError) as e:
        runs_from_keys(["a", "b", "b", "c", "b"], base=1000)
    assert "'b'" in str(e.value) and "row 1002" in str(e.value) and "row 1004" in str(e.value)


def test_collection_derives_the_runs_from_its_ranks_metadata_and_refuses_a_split_paper():
    """The derivation runs before anything touches a device: a paper whose chunks are not consecutive is refused on any machine."""
    from arxiv_rag_amd.store import HipCollection
    meta = [{"paper_id": p, "chunk_id": f"c{r}"} for r, p in enumerate(["p0", "p0", "p1", "p0"])]
    with pytest.raises(ValueError) as e:
        HipCollection(np.zeros((4, 64), np.float32), meta, group_key="paper_id")
    assert "'p0'" in str(e.value) and "row 1" in str(e.value) and "row 3" in str(e.value)


@pytest.mark.parametrize("R", [1, 2, 64, 65, 66, 129])
def test_s_and_k_against_a_brute_force_count_of_the_groups_a_run_can_touch(R):
    brute = max(len({r // 64 for r in range(off, off + R)}) for off in range(64))
    assert groups_touched(R) == brute == (R + 62) // 64 + 1
    for P in (1, 10, 32):
        assert select_count(P, R) == P * brute


def test_k_512_and_513():
    assert select_count(32, 961) == 512 and select_count(32, 962) == 32 * 17 and select_count(27, 1090) == 513


def _collection_without_a_device(**attrs):
    from arxiv_rag_amd.store import HipCollection
    coll = object.__new__(HipCollection)
    coll.group_key, coll.world, coll._keep, coll.documents = "paper_id", 1, None, None
    for k, v in attrs.items():
        setattr(coll, k, v)
    return coll


def test_query_refuses_what_group_by_does_not_compose_with():
    q = np.zeros((2, 64), np.float16)
    coll = _collection_without_a_device()
    for kw, text in ((dict(reranker=object(), query_texts=["a", "b"]), "reranker"), (dict(hybrid_alpha=0.5, query_texts=["a", "b"]), "hybrid_alpha"),
                     (dict(mmr_lambda=0.5), "mmr_lambda"), (dict(where=[{"a": 1}, None]), "per-query filter lists"),
                     (dict(where_document=[{"$contains": "a"}, None]), "per-query filter lists"), (dict(n_results=33), "n_results=33"),
                     (dict(n_results=0), "n_results=0"), (dict(chunks_per_group=9), "chunks_per_group=9"),
                     (dict(chunks_per_group=0), "chunks_per_group=0")):
        with pytest.raises(ValueError) as e:
            coll.query(query_embeddings=q, group_by=True, **kw)
        assert text in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError, match="world == 1.*straddle"):
        _collection_without_a_device(world=2).query(query_embeddings=q, group_by=True)
    with pytest.raises(ValueError, match="group_key"):
        _collection_without_a_device(group_key=None).query(query_embeddings=q, group_by=True)


def test_search_queries_refuses_the_same():
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    for kw, text in ((dict(reranker=object()), "reranker"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(mmr_lambda=0.5), "mmr_lambda"),
                     (dict(where=[{"a": 1}]), "per-query filter lists"), (dict(chunks_per_paper=9), "chunks_per_group=9"),
                     (dict(top_k=33), "n_results=33")):
        with pytest.raises(ValueError) as e:
            GEN.search_queries(None, [], None, ["q"], group_by_paper=True, **kw)
        assert text in str(e.value), (kw, str(e.value))


def test_search_queries_refuses_more_than_one_rank(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="straddle"):
        GEN.search_queries(None, [], None, ["q"], group_by_paper=True)


def _boom(name):
    raise AssertionError("the model must not be loaded")


def test_cli_group_flags_are_checked_before_any_model_is_loaded(tmp_path, capsys, monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = GEN.build_parser().parse_args(["in"])
    assert args.group_by_paper is False and args.chunks_per_paper == 1 and GEN.check_group_args(args) is None
    args = GEN.build_parser().parse_args(["in", "--queries", "q.txt", "--group-by-paper", "--chunks-per-paper", "3"])
    assert args.group_by_paper is True and args.chunks_per_paper == 3 and GEN.check_group_args(args) is None
    (tmp_path / "in").mkdir()
    (tmp_path / "w.jsonl").write_text("null\n")
    (tmp_path / "q.txt").write_text("one query\n")
    q = ["--queries", str(tmp_path / "q.txt")]
    for extra, msg in ((["--chunks-per-paper", "2"], "needs --group-by-paper"),
                       (["--group-by-paper"], "needs --queries"),
                       (q + ["--group-by-paper", "--rerank-model", "x"], "--rerank-model"),
                       (q + ["--group-by-paper", "--hybrid-alpha", "0.7"], "--hybrid-alpha"),
                       (q + ["--group-by-paper", "--mmr-lambda", "0.5"], "--mmr-lambda"),
                       (q + ["--group-by-paper", "--where-file", str(tmp_path / "w.jsonl")], "--where-file"),
                       (q + ["--group-by-paper", "--top-k", "33"], "--top-k 33"),
                       (q + ["--group-by-paper", "--top-k", "0"], "--top-k 0"),
                       (q + ["--group-by-paper", "--chunks-per-paper", "9"], "--chunks-per-paper 9"),
                       (q + ["--group-by-paper", "--chunks-per-paper", "0"], "--chunks-per-paper 0")):
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma"] + extra, model_factory=_boom)
        out = capsys.readouterr().out
        assert rc == 2 and msg in out, (extra, out)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert GEN.main([str(tmp_path / "in"), "--skip-chroma"] + q + ["--group-by-paper"], model_factory=_boom) == 2
    assert "single GPU rank" in capsys.readouterr().out


def test_check_grouped_query_is_silent_without_group_by():
    check_grouped_query(1000, 1000, grouped=False, has_group_key=False, reranker=object(), hybrid_alpha=0.5, mmr_lambda=0.5,
                        per_query_filters=True, world=8)


def test_library_exports_the_grouped_search_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
    assert len(_lib.EXPORTS["arx_topk_search_grouped"][1]) == 19 and len(_lib.EXPORTS["arx_topk_search_grouped_tuned"][1]) == 21
    bound = _lib.load()
    # host-only argument checks (no GPU involved): shapes the grouped search refuses
    f = bound.arx_topk_grouped_workspace_bytes
    assert f(1000, 64, 768, 10, 3) > 0 and f(1, 1, 64, 1, 1) > 0 and f(1000, 64, 768, 32, 8) > 0
    for bad in ((1000, 64, 768, 33, 3), (1000, 64, 768, 0, 3), (1000, 64, 768, 10, 9), (1000, 64, 768, 10, 0), (1000, 64, 100, 10, 3),
                (1000, 64, 0, 10, 3), (0, 1, 64, 1, 1), (1000, 0, 64, 1, 1), (1 << 36, 1, 64, 1, 1)):
        assert f(*bad) == -1, bad
    assert f(1000, 5000, 64, 32, 8) == f(1000, 1024, 64, 32, 8)      # internal batches of at most 1 024 queries
    assert f(1000, 64, 768, 10, 1) == f(1000, 64, 768, 10, 8)        # chunks_per_group does not enter
    # the formula of include/arx.h
    def formula(n, nq, P):
        qb = min(nq, 1024); ldg = (qb + 63) // 64 * 64; G = (n + 63) // 64; T = min((n + 255) // 256, 128)
        return sum((b + 255) // 256 * 256 for b in (64, 4 * G * ldg, 8 * G, 4 * qb, 4 * qb * P, 8 * qb * P, 4 * T * qb * P, 8 * T * qb * P))
    for n, nq, P in ((1000, 64, 10), (1, 1, 1), (12805, 1100, 32), (1 << 20, 64, 10)):
        assert f(n, nq, 768, P, 3) == formula(n, nq, P), (n, nq, P)


def test_grouped_kernels_do_not_spill_or_use_scratch():
    """What csrc/build.sh recorded for grouped.hip (as tests/test_build_resources.py reads it for every object)."""
    from tests.test_build_resources import BUILD, PAT
    f = BUILD / "grouped.resources.txt"
    if not f.exists():
        pytest.skip("no _build/grouped.resources.txt (library not built by csrc/build.sh in this tree)")
    ks = {m.group(1): (int(m.group(4)), int(m.group(7))) for m in PAT.finditer(f.read_text())}
    for name in ("masked_groupmax_kernel", "grouped_tail_kernel", "grouped_exhaustive_kernel", "grouped_chunks_kernel", "group_runs_kernel",
                 "filter_merge_kernel"):
        assert any(name in k for k in ks), name
    assert sum("masked_groupmax_kernel" in k for k in ks) == 3        # 64-, 128- and 256-query tiles
    bad = {k: v for k, v in ks.items() if v[0] or v[1]}
    assert not bad, bad
