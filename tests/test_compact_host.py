"""Host side of the mutable collection (INTEGRATION.md "Adding and deleting rows"): the C ABI's three compaction entry points and their
argument checks (refused before anything is launched, so no GPU is needed), and the bookkeeping of `add` / `delete` / `compact` /
`get` on pure-host pieces and on a stub collection."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_compact_plan", "arx_compact_rows", "arx_compact_text"}
ARX_ERR_ARG = -1


def test_the_three_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
    assert [len(_lib.EXPORTS[n][1]) for n in sorted(NEW)] == [5, 7, 8]
    assert re.search(r"#define\s+ARX_ERR_ARG\s+-1\b", hdr)


def _refused(call, *needles):
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    assert call(lib) == ARX_ERR_ARG
    msg = lib.arx_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_argument_errors_are_returned_before_any_launch():
    p = 4096                                                    # a non-null "pointer" that is never read: every call below is refused first
    _refused(lambda l: l.arx_compact_plan(None, 10, p, p, None), "keep")
    _refused(lambda l: l.arx_compact_plan(p, 10, None, p, None), "word_rank")
    _refused(lambda l: l.arx_compact_plan(p, 10, p, None, None), "out_count")
    _refused(lambda l: l.arx_compact_plan(p, -1, p, p, None), "n_rows", "-1")
    _refused(lambda l: l.arx_compact_plan(p, 1 << 36, p, p, None), "n_rows", str(1 << 36))
    for i, name in ((0, "src"), (1, "dst"), (4, "keep"), (5, "word_rank")):
        args = [p, p, 1536, 10, p, p, None]
        args[i] = None
        _refused(lambda l: l.arx_compact_rows(*args), name)
    _refused(lambda l: l.arx_compact_rows(p, p, 0, 10, p, p, None), "row_bytes", "0")
    _refused(lambda l: l.arx_compact_rows(p, p, 16385, 10, p, p, None), "row_bytes", "16385")
    _refused(lambda l: l.arx_compact_rows(p, p, 8, -5, p, p, None), "n_rows", "-5")
    for i, name in ((0, "blob"), (1, "row_off"), (3, "keep"), (4, "word_rank"), (5, "new_blob"), (6, "new_row_off")):
        args = [p, p, 10, p, p, p, p, None]
        args[i] = None
        _refused(lambda l: l.arx_compact_text(*args), name)
    _refused(lambda l: l.arx_compact_text(p, p, 1 << 40, p, p, p, p, None), "n_rows", str(1 << 40))


def test_old_to_new_map_and_host_plan():
    from arxiv_rag_amd.mutation import old_to_new, unpack_rows, word_rank_host
    from arxiv_rag_amd.where import pack_bitmap
    keep = np.array([1, 0, 0, 1, 1, 0, 1], bool)
    assert old_to_new(keep).tolist() == [0, -1, -1, 1, 2, -1, 3]
    assert old_to_new(np.zeros(3, bool)).tolist() == [-1, -1, -1] and old_to_new(np.zeros(0, bool)).tolist() == []
    rs = np.random.RandomState(0)
    for n in (1, 63, 64, 65, 257, 4099):
        keep = rs.rand(n) < 0.5
        words = pack_bitmap(keep)
        assert np.array_equal(unpack_rows(words, n), keep)
        want = np.concatenate([[0], np.cumsum([keep[a:a + 64].sum() for a in range(0, n, 64)])])
        assert np.array_equal(word_rank_host(words, n), want)
        r = int(rs.randint(n))                                   # the formula of include/arx.h
        if keep[r]:
            below = int(words[r >> 6]) & ((1 << (r & 63)) - 1)
            assert want[r >> 6] + bin(below).count("1") == old_to_new(keep)[r]


def test_id_map_duplicates_and_unknown_ids():
    from arxiv_rag_amd.mutation import build_id_map, rows_of_ids
    meta = [{"chunk_id": "a"}, {}, {"chunk_id": "b"}]
    ids = build_id_map(meta)
    assert ids == {"a": 0, "chunk_1": 1, "b": 2}
    assert rows_of_ids(ids, ["b", "a", "b"]) == [2, 0, 2]
    with pytest.raises(ValueError, match="unknown id 'zz'"):
        rows_of_ids(ids, ["a", "zz"])
    with pytest.raises(ValueError, match="duplicate id 'a'.*rows 0 and 2"):
        build_id_map([{"chunk_id": "a"}, {"chunk_id": "c"}, {"chunk_id": "a"}])
    more = build_id_map([{"chunk_id": "c"}, {}], base=3, into=ids)
    assert more == {"a": 0, "chunk_1": 1, "b": 2, "c": 3, "chunk_4": 4} and len(ids) == 3          # `into` is not changed
    with pytest.raises(ValueError, match="duplicate id 'b'.*rows 2 and 4"):
        build_id_map([{"chunk_id": "c"}, {"chunk_id": "b"}], base=3, into=ids)


def test_group_runs_continue_and_refuse():
    from arxiv_rag_amd.grouping import continue_runs, runs_from_keys
    old = ["p0", "p0", "p1", "p2", "p2"]
    g, keys = runs_from_keys(old)
    new = ["p2", "p3", "p3", "p4"]                               # the first new row continues the last run
    g2, keys2 = continue_runs(g, keys, new)
    whole, whole_keys = runs_from_keys(old + new)
    assert np.array_equal(np.concatenate([g, g2]), whole) and keys2 == whole_keys and keys == ["p0", "p1", "p2"]
    g3, keys3 = continue_runs(g, keys, ["p9"])
    assert g3.tolist() == [3] and keys3 == ["p0", "p1", "p2", "p9"]
    with pytest.raises(ValueError) as e:
        continue_runs(g, keys, ["p2", "p1"], base=100)
    with pytest.raises(ValueError) as ref:
        runs_from_keys(old + ["p2", "p1"], base=100)
    assert str(e.value) == str(ref.value) and "'p1'" in str(e.value) and "row 102" in str(e.value) and "row 106" in str(e.value)
    with pytest.raises(ValueError, match="'p2'"):
        continue_runs(g, keys, ["p3", "p2"])
    # after a compaction that removed run 1 entirely its value is unused: the key may come back, and new runs take fresh values
    g4, keys4 = continue_runs(g[[0, 1, 3, 4]], keys, ["p1", "p5"])
    assert g4.tolist() == [3, 4] and keys4 == ["p0", "p1", "p2", "p1", "p5"]
    e0, k0 = continue_runs(np.zeros(0, np.int32), [], ["x", "x", "y"])
    assert e0.tolist() == [0, 0, 1] and k0 == ["x", "y"]


def test_flat_pieces_append_and_compact():
    from arxiv_rag_amd.keyword import flatten_pieces
    from arxiv_rag_amd.mutation import append_pieces, compact_pieces, piece_lists
    lists = [[5, 6], [], [7], [8, 9, 10], []]
    flat, ptr = flatten_pieces(lists)
    assert piece_lists(flat, ptr) == lists
    f2, p2 = append_pieces(flat, ptr, *flatten_pieces([[1], [], [2, 3]]))
    assert piece_lists(f2, p2) == lists + [[1], [], [2, 3]] and f2.dtype == np.int32 and p2.dtype == np.int64
    keep = np.array([1, 1, 0, 1, 0, 0, 1, 1], bool)
    f3, p3 = compact_pieces(f2, p2, keep)
    assert piece_lists(f3, p3) == [[5, 6], [], [8, 9, 10], [], [2, 3]]
    f4, p4 = compact_pieces(f2, p2, np.zeros(8, bool))
    assert len(f4) == 0 and p4.tolist() == [0]


def _stub(capacity=8):
    """A collection's host state without a device: what `delete`, `get` and the refusals read."""
    import torch
    from arxiv_rag_amd.mutation import build_id_map
    from arxiv_rag_amd.store import HipCollection
    col = HipCollection.__new__(HipCollection)
    col.metadata = [{"chunk_id": f"c{j}", "text": f"t{j}", "paper_id": f"p{j // 2}"} for j in range(5)]
    col.capacity, col.dedup_threshold, col.n_total, col.lo, col.hi, col.dim = capacity, None, 5, 0, 5, 4
    col._ids, col._deleted, col._n_deleted, col._keep_mask, col._keep = build_id_map(col.metadata), None, 0, None, None
    col._buf = torch.zeros((capacity or 5, 4), dtype=torch.float16)
    return col


def test_without_capacity_add_delete_and_compact_raise():
    col = _stub(capacity=None)
    for call in (lambda: col.add(np.zeros((1, 4), np.float32), [{}]), lambda: col.delete(ids=["c0"]), lambda: col.compact()):
        with pytest.raises(ValueError, match="capacity"):
            call()
    assert col.get(["c3", "c1"])["ids"] == ["c3", "c1"]         # reading by id needs no capacity


def test_delete_and_get_bookkeeping_on_a_stub():
    from arxiv_rag_amd.mutation import unpack_rows
    col = _stub()
    with pytest.raises(ValueError, match="needs ids, where or where_document"):
        col.delete()
    with pytest.raises(ValueError, match="unknown id 'nope'"):
        col.delete(ids=["c1", "nope"])
    assert col.count() == 5 and col._deleted is None             # the refused call deleted nothing
    assert col.delete(ids=["c1", "c4"]) == 2 and col.count() == 3
    assert col._keep_mask.tolist() == [True, False, True, True, False]
    assert unpack_rows(col._keep.numpy(), 5).tolist() == col._keep_mask.tolist()
    got = col.get(["c3", "c0"])
    assert got["documents"] == ["t3", "t0"] and got["metadatas"][0]["paper_id"] == "p1"
    with pytest.raises(ValueError, match="unknown id 'c1'"):     # a deleted id is forgotten at once
        col.get(["c1"])
    with pytest.raises(ValueError, match="unknown id 'c1'"):
        col.delete(ids=["c1"])
    col.dedup_threshold = 0.9
    with pytest.raises(ValueError, match="dedup_threshold"):
        col.delete(ids=["c0"])


def test_add_refusals_change_nothing_on_a_stub():
    col = _stub(capacity=6)
    col.group_key, col._kw_pieces = None, None
    before = (list(col.metadata), dict(col._ids), col.n_total)
    with pytest.raises(ValueError, match="5 rows \\+ 2 new rows exceed capacity=6"):
        col.add(np.zeros((2, 4), np.float32), [{"chunk_id": "x"}, {"chunk_id": "y"}])
    with pytest.raises(ValueError, match="duplicate id 'c2'"):
        col.add(np.zeros((1, 4), np.float32), [{"chunk_id": "c2"}])
    with pytest.raises(ValueError, match="dim 4"):
        col.add(np.zeros((1, 5), np.float32), [{"chunk_id": "x"}])
    with pytest.raises(ValueError, match="one dict each"):
        col.add(np.zeros((1, 4), np.float32), [])
    assert (col.metadata, col._ids, col.n_total) == before
