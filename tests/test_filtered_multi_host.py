"""Host side of the search with a different filter per query (arxiv_rag_amd/filter_sets.py, the CLI's --where-file): no GPU."""
import json
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import filter_sets as FS

ROOT = Path(__file__).resolve().parent.parent


def test_filter_pairs_are_canonicalised_and_deduplicated():
    a = {"section": "abstract", "quality_score": {"$gte": 0.95, "$lt": 1.0}}
    b = {"quality_score": {"$lt": 1.0, "$gte": 0.95}, "section": "abstract"}           # the same filter, keys in another order
    c = {"$and": [{"section": "abstract"}, {"chunk_index": 1}]}
    d = {"$and": [{"chunk_index": 1}, {"section": "abstract"}]}                         # (lists keep their order: another key)
    assert FS.canonical_pair(a, None) == FS.canonical_pair(b, None)
    assert FS.canonical_pair(a, None) != FS.canonical_pair(None, a)
    assert FS.canonical_pair(c, None) != FS.canonical_pair(d, None)
    doc = {"$contains": "alpha"}
    wheres = [a, None, b, c, None, a, d, None]
    docs = [None, None, None, doc, None, doc, None, doc]
    pairs, filter_of = FS.distinct_filters(wheres, docs)
    assert filter_of == [0, 1, 0, 2, 1, 3, 4, 5]
    assert pairs == [(a, None), (None, None), (c, doc), (a, doc), (d, None), (None, doc)]
    assert FS.distinct_filters([], []) == ([], [])
    with pytest.raises(ValueError):
        FS.distinct_filters([a], [])


def test_per_query_list():
    a = {"section": "abstract"}
    assert FS.per_query_list(None, 3, "where") == [None] * 3
    assert FS.per_query_list(a, 2, "where") == [a, a]
    assert FS.per_query_list((a, None), 2, "where") == [a, None]
    assert FS.is_per_query([a]) and FS.is_per_query((a,)) and not FS.is_per_query(a) and not FS.is_per_query(None)
    with pytest.raises(ValueError, match="2 entries for 3 queries"):
        FS.per_query_list([a, None], 3, "where")
    with pytest.raises(ValueError, match=r"where\[1\]"):
        FS.per_query_list([a, "abstract"], 2, "where")
    with pytest.raises(ValueError):
        FS.per_query_list("abstract", 2, "where")


@pytest.mark.parametrize("n_filters,max_filters", [(1, 64), (64, 64), (65, 64), (70, 64), (200, 64), (7, 2), (5, 1)])
def test_groups_hold_at_most_64_distinct_filters_and_the_order_is_restored(n_filters, max_filters):
    rs = np.random.RandomState(n_filters)
    filter_of = list(range(n_filters)) + rs.randint(n_filters, size=3 * n_filters + 5).tolist()      # every filter used, then any
    rs.shuffle(filter_of)
    groups = FS.filter_groups(filter_of, max_filters)
    assert len(groups) == (n_filters + max_filters - 1) // max_filters
    answer = [None] * len(filter_of)
    for positions, filters, local_of in groups:
        assert 1 <= len(filters) <= max_filters and filters == sorted(set(filters))
        assert positions == sorted(positions) and len(local_of) == len(positions)
        assert set(local_of) == set(range(len(filters)))                                # no bitmap is passed that no query uses
        for p, j in zip(positions, local_of):
            assert answer[p] is None, "a query in two calls"
            answer[p] = filters[j]                                                      # what the call would answer for that query
    assert answer == filter_of                                                          # every query once, with its own filter
    assert FS.filter_groups([]) == []
    with pytest.raises(ValueError):
        FS.filter_groups([0], 0)


def _args(tmp_path, filters, queries=("q one", "q two", "q three"), **kw):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    (tmp_path / "in").mkdir(exist_ok=True)
    (tmp_path / "queries.txt").write_text("\n".join(queries) + "\n")
    argv = [str(tmp_path / "in"), "--queries", str(tmp_path / "queries.txt")]
    if filters is not None:
        (tmp_path / "filters.jsonl").write_text("\n".join(f if isinstance(f, str) else json.dumps(f) for f in filters) + "\n")
        argv += ["--where-file", str(tmp_path / "filters.jsonl")]
    for key, val in kw.items():
        argv += ["--" + key.replace("_", "-"), str(val)]
    return GEN, argv


def test_check_where_file_args(tmp_path, capsys):
    filters = [{"section": "abstract"}, None, {"quality_score": {"$gte": 0.95}}]
    GEN, argv = _args(tmp_path, filters)
    args = GEN.build_parser().parse_args(argv)
    assert GEN.check_where_file_args(args) is None and args.where_filters == filters
    GEN, argv = _args(tmp_path, None)
    args = GEN.build_parser().parse_args(argv)
    assert GEN.check_where_file_args(args) is None and args.where_filters is None
    # exclusive with --where, refused with --hybrid-alpha (the wording of the other checks)
    GEN, argv = _args(tmp_path, filters, where='{"section": "abstract"}')
    assert "--where-file cannot be combined with --where" in GEN.check_where_file_args(GEN.build_parser().parse_args(argv))
    GEN, argv = _args(tmp_path, filters, hybrid_alpha=0.5)
    assert GEN.check_where_file_args(GEN.build_parser().parse_args(argv)) == \
        "--where-file cannot be combined with --hybrid-alpha: the BM25 keyword search has no row filter"
    # a line that is no filter
    for bad, word in (("{not json", "line 2 is not valid JSON"), ('"abstract"', "line 2"), ('{"section": {"$like": "a"}}', "$like")):
        GEN, argv = _args(tmp_path, [filters[0], bad, None])
        assert word in GEN.check_where_file_args(GEN.build_parser().parse_args(argv))
    # a line-count mismatch: exit status 2 and both counts
    GEN, argv = _args(tmp_path, filters[:2])
    msg = GEN.check_where_file_args(GEN.build_parser().parse_args(argv))
    assert "2 filters" in msg and "3 queries" in msg
    assert GEN.main(argv) == 2
    out = capsys.readouterr().out
    assert "2 filters" in out and "3 queries" in out
    GEN, argv = _args(tmp_path, filters, hybrid_alpha=0.5)
    assert GEN.main(argv) == 2
    argv = argv[:3] + ["--where-file", str(tmp_path / "no such file")]
    assert GEN.main(argv) == 2


def test_the_new_symbols_are_declared_and_bound():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    for name in ("arx_topk_filtered_multi_workspace_bytes", "arx_topk_search_filtered_multi", "arx_topk_search_filtered_multi_tuned",
                 "arx_topk_filtered_multi_stats"):
        assert name + "(" in hdr, f"{name} is not declared in include/arx.h"
        assert name in _lib.EXPORTS, f"{name} has no ctypes prototype"
    assert len(_lib.EXPORTS["arx_topk_search_filtered_multi_tuned"][1]) == len(_lib.EXPORTS["arx_topk_search_filtered_multi"][1]) + 2
    assert len(_lib.EXPORTS["arx_topk_filtered_multi_workspace_bytes"][1]) == 5
