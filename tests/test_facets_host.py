"""Facet counts on the host (no GPU): `facets.count_host`, the numpy interpreter of the arrays `arx_facet_count` reads, against
`facets.oracle`, a `collections.Counter` over the metadata dicts; spec resolution and its refusals; the ordering rule; the layout of
`arx_facet_key`; the exports of the built library.  Every comparison is exact."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import facets as F
from arxiv_rag_amd.where_device import MetadataColumns

ROOT = Path(__file__).resolve().parents[1]
NAN, INF = float("nan"), float("inf")
EDGES = [0.0, 0.5, 0.9, 1.0]


def make_metadata(n=400, seed=3):
    """Mixed kinds under one key, absent keys, NaN, +-inf, +-0.0, bools beside numbers, non-ASCII strings, a row that is no dict."""
    rs = np.random.RandomState(seed)
    sections = ["Introduction", "Methods", "Résumé", "结论", "Ωmega", ""]
    numbers = [0.0, -0.0, 0.5, 0.9, 1.0, 1, 2, -3, 2.5, NAN, INF, -INF, 1e300, np.float32(0.25), np.int64(7)]
    meta = []
    for r in range(n):
        m = {"paper_id": f"p{r // 7:03d}"}
        u = rs.randint(0, 10)
        if u < 6:
            m["section"] = sections[rs.randint(len(sections))]
        elif u == 6:
            m["section"] = 3                                   # a number under a key that mostly holds strings
        elif u == 7:
            m["section"] = True
        v = rs.randint(0, 12)
        if v < 8:
            m["score"] = numbers[rs.randint(len(numbers))]
        elif v == 8:
            m["score"] = bool(rs.randint(2))                   # a bool next to numbers
        elif v == 9:
            m["score"] = "high"
        if rs.randint(3):
            m["flag"] = bool(rs.randint(2))
        if rs.randint(2):
            m["year"] = int(rs.choice([2019, 2020, 2020, 2021]))
        meta.append(m)
    meta[5] = None
    return meta


def make_masks(n, seed=1):
    rs = np.random.RandomState(seed)
    contiguous = np.zeros(n, bool)
    contiguous[n // 3:n // 3 + n // 8] = True
    return np.stack([np.ones(n, bool), np.zeros(n, bool), rs.rand(n) < 0.5, rs.rand(n) < 0.02, contiguous])


SPECS = ["section", "score", "flag", "year", "paper_id", "absent_key", {"key": "section", "kind": "number"}, {"key": "section", "kind": "bool"},
         {"key": "score", "kind": "bool"}, {"key": "score", "kind": "string"}, {"key": "score", "edges": EDGES},
         {"key": "year", "edges": [2019, 2020, 2021]}, {"key": "flag", "kind": "string"}, {"key": "score", "kind": "number"}]


@pytest.mark.parametrize("top", [1, 3, 10, None])
def test_count_host_equals_the_oracle_in_all_three_modes(top):
    meta = make_metadata()
    n = len(meta)
    masks = make_masks(n)
    cols = MetadataColumns(meta)
    got = F.count_host(cols, SPECS, masks, top=top)
    want = F.oracle(meta, 0, n, SPECS, masks, top=top)
    assert len(got) == len(masks) and all(len(row) == len(SPECS) for row in got)
    for fi in range(len(masks)):
        for a, b, spec in zip(got[fi], want[fi], SPECS):
            assert a == b, (fi, spec, a, b)
            assert a["total"] == int(masks[fi].sum())
    full = F.count_host(cols, SPECS, masks, top=None)[0]
    by = {i: r for i, r in enumerate(full)}
    assert by[0]["values"][0] == "" or "" in by[0]["values"]                   # the empty string is a value
    assert "结论" in by[0]["values"] and "Résumé" in by[0]["values"]
    assert by[1]["values"] == ["high"]                                          # a bare key with a string anywhere: its strings
    assert by[13]["unbinned"] > 0                                               # the NaNs of `score`
    assert {0.0, INF, -INF, 1e300} <= set(by[13]["values"]) and sum(1 for v in by[13]["values"] if v == 0.0) == 1   # -0.0 folded
    assert by[5] == {"key": "absent_key", "values": [], "counts": [], "distinct": 0, "missing": n, "unbinned": 0, "total": n}
    assert by[10]["values"] == [(0.0, 0.5), (0.5, 0.9), (0.9, 1.0)] and by[10]["unbinned"] > 0 and all(c > 0 for c in by[10]["counts"])
    assert by[12]["values"] == [] and by[12]["missing"] == n                    # a kind no row has under the key
    for row in F.count_host(cols, SPECS, masks, top=None):                      # every key's counters sum to the allowed rows
        for r in row:
            assert sum(r["counts"]) + r["missing"] + r["unbinned"] == r["total"], r


def test_count_host_without_masks_and_on_a_row_range():
    meta = make_metadata(300, seed=9)
    got = F.count_host(MetadataColumns(meta, 40, 233), SPECS, None, top=None)
    assert got == F.oracle(meta, 40, 233, SPECS, None, top=None) and len(got) == 1
    assert got[0][0]["total"] == 193


def test_edges_take_values_exactly_on_every_edge():
    meta = [{"q": v} for v in [0.0, -0.0, 0.5, 0.9, 1.0, 1.0, np.nextafter(1.0, 2.0), np.nextafter(0.0, -1.0), 0.4999, NAN, "x"]] + [{}]
    spec = [{"key": "q", "edges": EDGES}]
    got = F.count_host(MetadataColumns(meta), spec)[0][0]
    assert got == F.oracle(meta, 0, len(meta), spec)[0][0]
    assert got["counts"] == [3, 1, 3] and got["unbinned"] == 3 and got["missing"] == 2 and got["total"] == 12 and got["distinct"] == 3


def test_bin_counts_host_sends_wild_codes_to_unbinned():
    kind = np.full(8, 2, np.uint8)
    val = np.array([0.0, 3.0, -1.0, 4.0, 2.5, 1e300, NAN, -0.0])
    got = F.bin_counts_host(F.CODE, 2, 4, None, kind, val)
    assert got.tolist() == [2, 0, 0, 1, 0, 5] and got.sum() == 8
    kind[1] = 1
    assert F.bin_counts_host(F.CODE, 2, 4, None, kind, val, np.arange(8) < 4).tolist() == [1, 0, 0, 0, 1, 2]


def test_the_ordering_rule_with_ties():
    meta = [{"s": s} for s in ["b", "a", "c", "b", "a", "d", "c", "e"]]
    cols = MetadataColumns(meta)
    r = F.count_host(cols, ["s"], None, top=None)[0][0]
    assert r["values"] == ["a", "b", "c", "d", "e"] and r["counts"] == [2, 2, 2, 1, 1] and r["distinct"] == 5
    r = F.count_host(cols, ["s"], None, top=4)[0][0]
    assert r["values"] == ["a", "b", "c", "d"] and r["distinct"] == 5           # count descending, then value ascending
    keys = F.order_keys(np.array([2, 0, 2, 7]))
    assert len(set(keys.tolist())) == 4
    assert F._pairs_from_keys(np.sort(keys)[::-1]) == [(3, 7), (0, 2), (2, 2)]  # zero counts are never listed
    nums = [{"x": v} for v in [3, 1.0, 1, 2, 3.0, 2]]
    r = F.count_host(MetadataColumns(nums), ["x"])[0][0]
    assert r["values"] == [1.0, 2.0, 3.0] and r["counts"] == [2, 2, 2]


def test_spec_resolution():
    meta = make_metadata()
    cols = MetadataColumns(meta)
    f = F.resolve(cols, "section")
    assert (f.mode, f.want_kind, f.values) == (F.CODE, 2, cols.strings("section")) and f.cuts is None
    f = F.resolve(cols, "score")                                                # a string is present: strings win for a bare key
    assert (f.mode, f.want_kind, f.values) == (F.CODE, 2, ["high"])
    f = F.resolve(cols, {"key": "score", "kind": "number"})
    assert (f.mode, f.want_kind) == (F.EXACT, 1) and np.array_equal(f.cuts, cols.numbers("score")) and f.n_bins == len(f.cuts)
    f = F.resolve(cols, "year")
    assert (f.mode, f.want_kind, f.values) == (F.EXACT, 1, [2019.0, 2020.0, 2021.0])
    f = F.resolve(cols, "flag")
    assert (f.mode, f.want_kind, f.values) == (F.CODE, 3, [False, True])
    f = F.resolve(cols, {"key": "score", "edges": (0, 1, 2)})
    assert (f.mode, f.want_kind, f.n_bins, f.interval) == (F.INTERVAL, 1, 2, True) and f.cuts.tolist() == [0.0, 1.0, 2.0]
    assert F.resolve(cols, "absent_key").n_bins == 0 and F.resolve(cols, {"key": "flag", "kind": "number"}).n_bins == 0
    only_nan = MetadataColumns([{"x": NAN}, {"x": NAN}, {}])
    r = F.count_host(only_nan, ["x"])[0][0]
    assert r == F.oracle(only_nan.metadata, 0, 3, ["x"])[0][0] and (r["values"], r["unbinned"], r["missing"]) == ([], 2, 1)


@pytest.mark.parametrize("spec, part", [
    (7, "key name or a dict"), (["section"], "key name or a dict"), ({}, "\"key\" must be"), ({"key": 3}, "\"key\" must be"),
    ({"key": "a", "bins": 3}, "unknown field"), ({"key": "a", "kind": "date"}, "kind='date'"),
    ({"key": "a", "edges": [1]}, "at least two"), ({"key": "a", "edges": "01"}, "at least two"), ({"key": "a", "edges": [0, NAN]}, "finite"),
    ({"key": "a", "edges": [0, INF]}, "finite"), ({"key": "a", "edges": [0, "1"]}, "finite"), ({"key": "a", "edges": [False, True]}, "finite"),
    ({"key": "a", "edges": [0, 0]}, "ascend strictly"), ({"key": "a", "edges": [0, 2, 1]}, "ascend strictly"),
    ({"key": "a", "edges": [0, 1], "kind": "string"}, "cannot be combined")])
def test_malformed_specs_are_value_errors(spec, part):
    cols = MetadataColumns([{"a": 1}])
    for call in (lambda: F.parse_spec(spec), lambda: F.resolve(cols, spec), lambda: F.count_host(cols, [spec]),
                 lambda: F.oracle([{"a": 1}], 0, 1, [spec])):
        with pytest.raises(ValueError, match=re.escape(part)):
            call()
    assert not cols._host and not cols._numbers                                # refused before a column was built


def test_top_and_the_distinct_value_limit_are_value_errors(monkeypatch):
    cols = MetadataColumns([{"a": i} for i in range(9)])
    for top in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="top="):
            F.count_host(cols, ["a"], top=top)
    monkeypatch.setattr(F, "MAX_BINS", 8)
    with pytest.raises(ValueError, match=r"'a' has 9 distinct values, at most 8"):
        F.resolve(cols, "a")
    with pytest.raises(ValueError, match="needs one"):                          # no host fallback behind the product path
        F.count(cols, ["a"])


def test_numbers_are_cached_and_dropped_with_the_columns():
    meta = [{"x": v} for v in [2, -0.0, 0.0, NAN, 2.0, True, "s", -1.5]]
    cols = MetadataColumns(meta)
    first = cols.numbers("x")
    assert first.tolist() == [-1.5, 0.0, 2.0] and not np.signbit(first[1]) and first.dtype == np.float64
    assert cols.numbers("x") is first and "x" in cols._strings
    meta.append({"x": 11})
    cols.drop()
    assert not cols._numbers and not cols._strings and not cols._host
    assert MetadataColumns(meta).numbers("x").tolist() == [-1.5, 0.0, 2.0, 11.0]


def test_a_mutable_collection_drops_the_columns_object_whenever_rows_change():
    """`HipCollection._drop_columns` forgets the whole `MetadataColumns`, number lists included (the GPU file checks the counts)."""
    import inspect
    from arxiv_rag_amd.store import HipCollection
    assert "_device_columns = {}, None" in inspect.getsource(HipCollection._drop_columns)
    for method in (HipCollection.add, HipCollection.compact):
        assert "self._drop_columns()" in inspect.getsource(method)


def test_facet_key_struct_matches_the_header():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    body = re.search(r"typedef struct arx_facet_key \{(.*?)\} arx_facet_key;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);\s*/\* offset\s+(\d+)", body, re.M)
    assert [f[2] for f in fields] == [n for n, _ in _lib.FacetKeyC._fields_] == ["kind", "val", "cuts", "mode", "want_kind", "n_bins",
                                                                               "reserved", "out_off"]
    ctype = {("uint8_t", "*"): ctypes.c_void_p, ("double", "*"): ctypes.c_void_p, ("int32_t", ""): ctypes.c_int32, ("int64_t", ""): ctypes.c_int64}
    for (t, star, name, off), (n2, t2) in zip(fields, _lib.FacetKeyC._fields_):
        assert ctype[(t, star)] is t2 and getattr(_lib.FacetKeyC, name).offset == int(off), name
    assert ctypes.sizeof(_lib.FacetKeyC) == 48
    for name, value in (("CODE", 0), ("EXACT", 1), ("INTERVAL", 2)):
        assert int(re.search(rf"#define ARX_FACET_{name}\s+(\d+)", hdr).group(1)) == value == getattr(_lib, f"FACET_{name}") == getattr(F, name)
    assert "sizeof(arx_facet_key) == 48" in (ROOT / "arxiv_rag_amd" / "csrc" / "facet.hip").read_text()


def test_the_built_library_exports_the_facet_entry_points():
    from arxiv_rag_amd import _lib
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("arx_facet_count", "arx_facet_count_tuned"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS and re.search(rf"int32_t {name}\(", (ROOT / "include" / "arx.h").read_text())


def test_cli_facets_arguments(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    parse = GEN.build_parser().parse_args
    args = parse(["in", "--queries", "q.txt", "--facets", "section, paper_id", "--facets-top", "3"])
    assert GEN.check_facets_args(args) is None and args.facet_keys == ["section", "paper_id"] and args.facets_top == 3
    args = parse(["in", "--queries", "q.txt"])
    assert GEN.check_facets_args(args) is None and args.facet_keys is None
    assert "--facets needs --queries" in GEN.check_facets_args(parse(["in", "--facets", "section"]))
    assert "--facets-top 5 needs --facets" in GEN.check_facets_args(parse(["in", "--queries", "q.txt", "--facets-top", "5"]))
    assert "separated by commas" in GEN.check_facets_args(parse(["in", "--queries", "q.txt", "--facets", "section,,x"]))
    assert "at least one" in GEN.check_facets_args(parse(["in", "--queries", "q.txt", "--facets", "section", "--facets-top", "0"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in GEN.check_facets_args(parse(["in", "--queries", "q.txt", "--facets", "section"]))
