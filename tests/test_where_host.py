"""Host side of the filtered search (CPU): Chroma `where` filters compiled and evaluated column-wise (arxiv_rag_amd/where.py) against a
per-row Python evaluation written here, the bitmap packing, the CLI's --where handling, and the C ABI's new symbols."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd.where import compile_where, evaluate, pack_bitmap

ROOT = Path(__file__).resolve().parents[1]


def _kind(v):
    return "b" if isinstance(v, bool) else "n" if isinstance(v, (int, float)) else "s" if isinstance(v, str) else None


def _row_ok(where, m):
    """The reference: one row, straight from Chroma's rules (missing key / other type fails everything but $ne / $nin)."""
    res = []
    for key, cond in where.items():
        if key in ("$and", "$or"):
            sub = [_row_ok(w, m) for w in cond]
            res.append(all(sub) if key == "$and" else any(sub))
            continue
        for op, x in (cond.items() if isinstance(cond, dict) else [("$eq", cond)]):
            v = m.get(key)
            if op in ("$in", "$nin"):
                hit = any(_kind(v) == _kind(y) and v == y for y in x)
                res.append(hit if op == "$in" else not hit)
                continue
            same = _kind(v) is not None and _kind(v) == _kind(x)
            if op == "$ne":
                res.append(not (same and v == x))
            else:
                res.append(same and {"$eq": v == x, "$gt": v > x, "$gte": v >= x, "$lt": v < x, "$lte": v <= x}[op] if same else False)
    return all(res)


def _synthetic(n=3000, seed=5):
    rs = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        m = {"paper_id": f"0704.{r // 7:04d}", "chunk_index": int(r % 7)}
        u = rs.rand()
        if u < 0.8:
            m["section"] = ["abstract", "Introduction", "Methods", "Results", ""][rs.randint(5)]
        elif u < 0.9:
            m["section"] = int(rs.randint(3))                    # a number where strings are expected
        if rs.rand() < 0.9:
            m["quality_score"] = float(np.round(rs.uniform(0.8, 1.0), 2)) if rs.rand() < 0.9 else "high"
        if rs.rand() < 0.3:
            m["reviewed"] = bool(rs.randint(2))
        if rs.rand() < 0.05:
            m["section"] = None
        rows.append(m)
    return rows


FILTERS = [
    {"section": "abstract"},
    {"section": {"$eq": "Methods"}},
    {"section": {"$ne": "Methods"}},
    {"section": {"$gt": "Introduction"}},
    {"section": {"$lte": "Methods"}},
    {"section": ""},
    {"section": 1},
    {"section": {"$in": ["abstract", "Results"]}},
    {"section": {"$nin": ["abstract", "Results"]}},
    {"section": {"$in": [0, 2]}},
    {"quality_score": {"$gte": 0.95}},
    {"quality_score": {"$gt": 0.9, "$lt": 0.95}},
    {"quality_score": {"$lte": 0.8}},
    {"quality_score": {"$ne": 0.9}},
    {"quality_score": "high"},
    {"quality_score": {"$in": [0.9, 0.95, 1]}},
    {"chunk_index": 3},
    {"chunk_index": {"$lt": 2}},
    {"chunk_index": 3.0},
    {"reviewed": True},
    {"reviewed": {"$ne": False}},
    {"reviewed": {"$in": [True]}},
    {"reviewed": 1},
    {"paper_id": {"$in": ["0704.0001", "0704.0100", "0704.0417", "nope"]}},
    {"paper_id": {"$gte": "0704.0400"}},
    {"absent": "x"},
    {"absent": {"$ne": "x"}},
    {"absent": {"$nin": [1, 2]}},
    {"section": "abstract", "quality_score": {"$gte": 0.9}},
    {"$and": [{"section": "abstract"}, {"quality_score": {"$gte": 0.95}}]},
    {"$or": [{"section": "abstract"}, {"chunk_index": {"$in": [0, 6]}}]},
    {"$and": [{"$or": [{"section": "Results"}, {"section": {"$ne": "Methods"}}]}, {"$or": [{"reviewed": True}, {"quality_score": {"$lt": 0.85}}]},
              {"paper_id": {"$nin": ["0704.0003"]}}]},
    {"$or": [{"$and": [{"chunk_index": {"$gte": 2}}, {"chunk_index": {"$lte": 4}}]}, {"absent": 1}]},
]


@pytest.mark.parametrize("lo_hi", [(0, None), (100, 1777), (2999, 3000), (5, 5)])
def test_evaluate_equals_the_per_row_evaluation_on_a_synthetic_table(lo_hi):
    rows = _synthetic()
    lo, hi = lo_hi[0], len(rows) if lo_hi[1] is None else lo_hi[1]
    some = 0
    for w in FILTERS:
        got = evaluate(compile_where(w), rows, lo, hi)
        want = np.array([_row_ok(w, rows[r]) for r in range(lo, hi)], dtype=bool)
        assert got.dtype == bool and got.shape == (hi - lo,)
        assert np.array_equal(got, want), (w, np.nonzero(got != want)[0][:5])
        some += int(want.any() and not want.all())
    if hi - lo > 1000:
        assert some > 20                                          # the filters are not vacuous on this table


def test_evaluate_on_the_harness_metadata():
    meta = json.loads((ROOT / "tests" / "golden" / "harness" / "expected_metadata.json").read_text())
    meta += [m for i in range(2) for m in json.loads((ROOT / "tests" / "golden" / "harness" / "expected_batched" /
                                                      f"metadata_batch_{i:04d}.json").read_text())]
    sections = sorted({m["section"] for m in meta if isinstance(m["section"], str)})     # (some harness chunks have none)
    filters = [{"section": s} for s in sections] + [{"paper_id": meta[0]["paper_id"]}, {"quality_score": {"$gte": 0.95}},
                                                    {"quality_score": {"$lt": 0.95}}, {"text_length": {"$gt": 20}},
                                                    {"$or": [{"section": sections[0]}, {"quality_score": {"$gte": 0.99}}]},
                                                    {"batch_index": 1}, {"chunk_id": {"$nin": [meta[1]["chunk_id"]]}}]
    for w in filters:
        got = evaluate(compile_where(w), meta)
        assert np.array_equal(got, np.array([_row_ok(w, m) for m in meta])), w
    assert evaluate(compile_where({"section": sections[0]}), meta).any()


def test_columns_are_cached_per_metadata_object():
    rows = _synthetic(200)
    cache = {}
    a = evaluate(compile_where({"section": "abstract"}), rows, cache=cache)
    col = cache[(id(rows), "section")][1]
    b = evaluate(compile_where({"section": {"$ne": "abstract"}}), rows, 10, 50, cache=cache)
    assert cache[(id(rows), "section")][1] is col and len(cache) == 1
    assert np.array_equal(b, ~a[10:50])


@pytest.mark.parametrize("bad,part", [
    ({}, "non-empty dict"), ("section", "non-empty dict"), ({"section": {"$like": "a"}}, "$like"), ({"$not": [{"a": 1}]}, "$not"),
    ({"$and": []}, "$and"), ({"$or": []}, "$or"), ({"$and": {"a": 1}}, "$and"), ({"$or": [{}]}, "non-empty dict"),
    ({"section": ["a", "b"]}, "section"), ({"section": {"$eq": ["a"]}}, "$eq"), ({"section": {"$eq": None}}, "$eq"),
    ({"section": {"$in": "abstract"}}, "$in"), ({"section": {"$in": []}}, "$in"), ({"section": {"$nin": [["a"]]}}, "$nin"),
    ({"section": {"$in": ["a", 1]}}, "$in"), ({"section": {}}, "section"), ({"quality_score": {"$gt": {"x": 1}}}, "$gt"),
    ({"reviewed": {"$gt": True}}, "$gt"), ({"$and": [{"a": 1}, {"b": {"$regex": "x"}}]}, "$regex"),
])
def test_malformed_filters_raise_value_error_naming_the_part(bad, part):
    with pytest.raises(ValueError) as e:
        compile_where(bad)
    assert part in str(e.value), str(e.value)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_pack_bitmap_round_trips(n):
    rs = np.random.RandomState(n)
    for mask in (rs.rand(n) < 0.5, np.ones(n, bool), np.zeros(n, bool)):
        words = pack_bitmap(mask)
        assert words.dtype == np.uint64 and words.shape == ((n + 63) // 64,)
        bits = np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")
        assert np.array_equal(bits[:n].astype(bool), mask) and not bits[n:].any()
        for r in range(n):                                        # the layout the kernels read: bit r & 63 of word r >> 6
            assert bool((int(words[r >> 6]) >> (r & 63)) & 1) == bool(mask[r])


def _boom(name):
    raise AssertionError("the model must not be loaded")


def test_cli_where_is_parsed_and_refused_before_any_model_is_loaded(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    args = GEN.build_parser().parse_args(["in", "--queries", "q.txt", "--where", '{"quality_score": {"$gte": 0.95}}'])
    assert GEN.check_where_args(args) is None and args.where_filter == {"quality_score": {"$gte": 0.95}}
    args = GEN.build_parser().parse_args(["in"])
    assert GEN.check_where_args(args) is None and args.where_filter is None
    (tmp_path / "in").mkdir()
    for extra, msg in ((["--where", "{section: abstract}"], "not valid JSON"),
                       (["--where", '{"section": {"$like": "a"}}'], "$like"),
                       (["--where", "[]"], "non-empty dict"),
                       (["--where", '{"section": "abstract"}', "--hybrid-alpha", "0.7"], "--hybrid-alpha")):
        rc = GEN.main([str(tmp_path / "in"), "--skip-chroma", "--queries", str(tmp_path / "q.txt")] + extra, model_factory=_boom)
        assert rc == 2
        assert msg in capsys.readouterr().out


def test_search_queries_refuses_where_with_hybrid_alpha():
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    with pytest.raises(ValueError, match="hybrid_alpha"):
        GEN.search_queries(None, [], None, ["q"], where={"section": "abstract"}, hybrid_alpha=0.5)


def test_library_exports_the_filtered_search_and_header_and_bindings_agree():
    from arxiv_rag_amd import _lib
    new = {"arx_topk_filtered_workspace_bytes", "arx_topk_search_filtered", "arx_topk_search_filtered_tuned", "arx_topk_filtered_stats"}
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in new:
        assert hasattr(lib, name), name
    bound = _lib.load()
    assert bound.arx_version() == 112
    # host-only argument checks (no GPU involved): shapes the filtered search refuses
    f = bound.arx_topk_filtered_workspace_bytes
    assert f(1000, 64, 768, 10) > 0 and f(1000, 64, 768, 33) == -1 and f(1000, 64, 100, 10) == -1 and f(0, 1, 64, 1) == -1
    assert f(1000, 5000, 64, 32) == f(1000, 1024, 64, 32)         # internal batches of at most 1 024 queries


def test_filter_kernels_do_not_spill_or_use_scratch():
    """What csrc/build.sh recorded for filter.hip (as tests/test_build_resources.py reads it for every object)."""
    from tests.test_build_resources import BUILD, PAT
    f = BUILD / "filter.resources.txt"
    if not f.exists():
        pytest.skip("no _build/filter.resources.txt (library not built by csrc/build.sh in this tree)")
    ks = {m.group(1): (int(m.group(4)), int(m.group(7))) for m in PAT.finditer(f.read_text())}
    for name in ("masked_groupmax_kernel", "masked_tail_kernel", "filter_scan_kernel", "filter_scatter_kernel", "masked_exhaustive_kernel",
                 "filter_merge_kernel"):
        assert any(name in k for k in ks), name
    assert sum("masked_groupmax_kernel" in k for k in ks) == 3        # 64-, 128- and 256-query tiles
    bad = {k: v for k, v in ks.items() if v[0] or v[1]}
    assert not bad, bad
