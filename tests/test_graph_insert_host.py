"""The numpy restatements of the graph's maintenance (`graph.link_host`, `remap_host`, `insert_host`), the refusals of an insert and the
exports of `arx_graph_link` / `arx_graph_remap` (no GPU; INTEGRATION.md "Keeping the graph").  The kernels are checked against the
restatements in tests/test_gpu_graph_link.py, the host layer in tests/test_gpu_graph_insert.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import graph as G
from arxiv_rag_amd.mutation import old_to_new
from arxiv_rag_amd.topics import exact_scores_host
from arxiv_rag_amd.where import pack_bitmap
from tests.graph_cases import ring

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_graph_link": 11, "arx_graph_link_tuned": 12, "arx_graph_remap": 7}
N, DIM = 60, 64


def _rows(n=N, seed=5):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, DIM)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


def _ranked(X, t, rows):
    """`rows` by (exact score against row t desc, row asc), the NaN scores last"""
    sc = exact_scores_host(X[rows], X[t:t + 1])[:, 0]
    return [r for _, r in sorted(zip(G._keys_of(sc, rows), rows), reverse=True)]


def test_the_new_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        proto = re.search(rf"^int32_t {name}\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(_lib.EXPORTS[name][1]), name
        assert hasattr(lib, name), name


# ---- link_host ----------------------------------------------------------------------------------------------------------------------
def test_link_leaves_the_head_and_ranks_the_pool_by_exact_score():
    X = _rows()
    nb = np.full((N, 8), -1, np.int32)
    nb[7] = [50, 51, 52, 53, 20, 21, -1, -1]                      # head 50..53, tail 20 21
    got = G.link_host(X, nb, [7], [0, 5], [30, 31, 32, 33, 34])
    assert got[7, :4].tolist() == [50, 51, 52, 53]                # the head is untouched
    assert got[7, 4:].tolist() == _ranked(X, 7, [20, 21, 30, 31, 32, 33, 34])[:4]
    other = np.ones(N, bool)
    other[7] = False
    assert np.array_equal(got[other], nb[other])                  # no other row is written
    assert np.array_equal(nb[7], [50, 51, 52, 53, 20, 21, -1, -1])          # the argument is not changed


def test_link_drops_the_target_the_heads_rows_repeats_and_rows_out_of_range():
    X = _rows()
    nb = np.full((N, 8), -1, np.int32)
    nb[7] = [50, 51, -1, N + 3, 20, 21, 20, 7]                    # an invalid head entry hides nothing; the tail repeats 20 and names 7
    offers = [7, 50, 51, 20, 21, 30, 30, N, -1, np.iinfo(np.int32).max, -N, 31]
    got = G.link_host(X, nb, [7], [0, len(offers)], offers)
    assert got[7, :4].tolist() == [50, 51, -1, N + 3]
    assert got[7, 4:].tolist() == _ranked(X, 7, [20, 21, 30, 31])
    one = G.link_host(X, nb, [7], [0, 1], [7])                    # the offer is the target itself: the tail is re-ranked, nothing more
    assert one[7].tolist() == [50, 51, -1, N + 3] + _ranked(X, 7, [20, 21]) + [-1, -1]
    in_head = G.link_host(X, nb, [7], [0, 1], [51])
    in_tail = G.link_host(X, nb, [7], [0, 1], [21])
    assert np.array_equal(in_head, one) and np.array_equal(in_tail, one)
    n_rows = G.link_host(X, nb, [7], [0, 2], [40, 30], n_rows=35)  # rows at or past n_rows are no rows: 50 and 51 leave the head's set, 40 the pool
    assert n_rows[7].tolist() == [50, 51, -1, N + 3] + _ranked(X, 7, [20, 21, 30]) + [-1]


def test_link_ties_go_to_the_lower_row_a_nan_row_ranks_last_and_an_empty_pool_pads():
    X = _rows()
    X[40] = X[12]                                                # duplicates: equal scores against every row
    X[41] = X[12]
    X[33] = np.nan
    nb = np.full((N, 8), -1, np.int32)
    nb[7, :4] = [50, 51, 52, 53]
    with np.errstate(all="ignore"):
        got = G.link_host(X, nb, [7], [0, 4], [41, 33, 40, 12])
        assert got[7, 4:].tolist() == [12, 40, 41, 33]
        few = G.link_host(X, nb, [7], [0, 6], [41, 33, 40, 12, 30, 31])
    dups = [r for r in few[7, 4:].tolist() if r in (12, 40, 41)]
    assert 33 not in few[7].tolist() and dups == [12, 40, 41][:len(dups)]        # six rows for four places: the NaN row is the first to go
    empty = G.link_host(X, nb, [7, 9], [0, 0, 2], [9, N])         # no tail, no offer / only the target and a row out of range
    assert empty[7].tolist() == [50, 51, 52, 53, -1, -1, -1, -1] and empty[9].tolist() == [-1] * 8


def test_link_skips_targets_that_do_not_ascend_bad_targets_and_bad_offer_ranges():
    X = _rows()
    nb = ring(0, N, N)
    offers = list(range(20, 32))
    targets = [5, 5, 3, 9, -1, 12, 9, 14, N]                      # 1: a repeat, 2: descending, 4 8: no rows, 6: below slot 5's 12
    start = [0, 2, 4, 5, 6, 7, 8, 9, 10, 12]
    got = G.link_host(X, nb, targets, start, offers)
    want = nb.copy()
    for s in (0, 3, 5, 7):
        want = G.link_host(X, want, [targets[s]], [0, start[s + 1] - start[s]], offers[start[s]:start[s + 1]])
    assert np.array_equal(got, want) and not np.array_equal(got[[5, 9, 12, 14]], nb[[5, 9, 12, 14]])
    assert np.array_equal(got[3], nb[3])
    # a slot at or below ANY earlier target is skipped, not only one below its left neighbour: no row is ever written by two slots
    assert np.array_equal(G.link_host(X, nb, [5, 3, 5], [0, 1, 2, 3], [20, 21, 22]), G.link_host(X, nb, [5], [0, 1], [20]))
    for bad in ([3, 2], [-1, 2], [0, 13], [12, 12 + (1 << 31)]):   # decreasing, negative, beyond the offers
        assert np.array_equal(G.link_host(X, nb, [5], bad, offers), nb), bad
    assert np.array_equal(G.link_host(X, nb, [5], [12, 12], offers), G.link_host(X, nb, [5], [0, 0], []))    # an empty range is legal


def test_link_does_not_depend_on_the_order_or_the_repetition_of_the_offers():
    X = _rows()
    nb = ring(0, N, N)
    rs = np.random.RandomState(3)
    offers = rs.randint(-3, N + 3, 300)
    a = G.link_host(X, nb, [11], [0, 300], offers)
    b = G.link_host(X, nb, [11], [0, 600], np.concatenate([offers[::-1], offers]))
    assert np.array_equal(a, b)
    assert a[11, :4].tolist() == nb[11, :4].tolist()
    pool = sorted(set(int(r) for r in offers.tolist() + nb[11, 4:].tolist() if 0 <= r < N and r != 11) - set(nb[11, :4].tolist()))
    assert a[11, 4:].tolist() == _ranked(X, 11, pool)[:4]


# ---- remap_host ---------------------------------------------------------------------------------------------------------------------
def test_remap_agrees_with_old_to_new_and_fronts_the_survivors():
    rs = np.random.RandomState(8)
    n_old = 130
    nb = rs.randint(0, n_old, (n_old, 8)).astype(np.int32)
    nb[rs.rand(n_old, 8) < 0.1] = -1
    nb[3, 2], nb[4, 0], nb[5, 7] = n_old, np.iinfo(np.int32).max, -7
    for frac in (0.0, 0.01, 0.5):
        keep = rs.rand(n_old) >= frac
        new = old_to_new(keep)
        got = G.remap_host(nb[keep], keep)
        count = int(keep.sum())
        assert got.shape == (count, 8) and got.max() < count and got.min() >= -1
        for i, old_row in enumerate(np.nonzero(keep)[0]):
            want = [int(new[e]) for e in nb[old_row] if 0 <= e < n_old and keep[e]]
            assert got[i].tolist() == want + [-1] * (8 - len(want)), (frac, i)
        assert np.array_equal(G.remap_host(nb[keep], pack_bitmap(keep), n_old), got)
        assert np.array_equal(G.remap_host(nb[keep], pack_bitmap(keep).view(np.int64), n_old), got)
    keep = np.zeros(n_old, bool)
    keep[77] = True                                              # all but one row deleted: only a self-loop could survive
    nb[77] = [77, 1, 2, 77, -1, 3, 4, 5]
    assert G.remap_host(nb[keep], keep).tolist() == [[0, 0, -1, -1, -1, -1, -1, -1]]
    assert np.array_equal(G.remap_host(nb, np.ones(n_old, bool))[0], [e for e in nb[0] if e >= 0] + [-1] * int((nb[0] < 0).sum()))


# ---- insert_host --------------------------------------------------------------------------------------------------------------------
def _clustered(n, seed, n_clusters=6):
    rs = np.random.RandomState(seed)
    c = rs.randn(n_clusters, DIM)
    X = c[rs.randint(0, n_clusters, n)] + 0.5 * rs.randn(n, DIM)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


_world = {}


def world():
    """96 clustered rows, the exact degree-8 graph over the first 64 and the entries of the 32 rows to insert, computed once"""
    if not _world:
        X = _clustered(96, 2)
        S = exact_scores_host(X[:64], X[:64])
        knn = np.stack([[r for r in np.lexsort((np.arange(64), -S[:, j])) if r != j][:31] for j in range(64)]).astype(np.int32)
        ent = np.random.RandomState(4).randint(0, 64, (32, 4)).astype(np.int32)
        _world.update(X=X, base=G.assemble_host(knn, 8), ent=ent)
        _world["one"] = G.insert_host(X, _world["base"], 64, 96, ent, insert_ef=31)
    return _world


def test_insert_host_is_deterministic_and_links_every_new_row():
    w = world()
    X, base, ent = w["X"], w["base"], w["ent"]
    nb, info = w["one"]
    again, info2 = G.insert_host(X, base, 64, 96, ent, insert_ef=31)
    assert np.array_equal(nb, again) and info == info2
    assert nb.shape == (96, 8) and info["inserted"] == 32 and info["orphans"] == G.orphans_host(nb, 64, 96)
    assert np.array_equal(nb[:64, :4], base[:, :4])                # the old rows' heads stay
    assert (nb[64:, :4] >= 0).all() and nb.max() < 96
    for i, row in enumerate(nb):
        v = row[row >= 0]
        assert len(set(v.tolist())) == v.shape[0] and i not in v, i
    assert info["offers"] == 32 * 4 and ((nb[:64, 4:] >= 64).sum() > 0)           # new rows entered old rows' tails


def test_insert_host_in_two_batches_sees_the_first_batch_from_the_second():
    w = world()
    X, base, ent = w["X"], w["base"], w["ent"]
    two, info = G.insert_host(X, base, 64, 96, ent, insert_ef=31, batch=16)
    again, _ = G.insert_host(X, base, 64, 96, ent, insert_ef=31, batch=16)
    assert np.array_equal(two, again) and info["inserted"] == 32
    first, _ = G.insert_host(X, base, 64, 80, ent[:16], insert_ef=31)
    second, _ = G.insert_host(X, first, 80, 96, ent[16:], insert_ef=31)
    assert np.array_equal(two, second)                            # a batch is an insert of its own over the rows before it


def test_every_inserted_rows_head_is_its_best_candidates():
    """with every old row reachable (insert_ef = 64 = the rows there are, entries in every cluster) the walk finds the exact nearest
    rows, so a new row's list is its exact nearest rows among the old rows and its batch"""
    w = world()
    X, base = w["X"], w["base"]
    ent = np.tile(np.arange(0, 64, 2, dtype=np.int32), (32, 1))
    nb, _ = G.insert_host(X, base, 64, 96, ent, insert_ef=64)
    S = exact_scores_host(X, X[64:])
    for j in range(32):
        want = [r for r in np.lexsort((np.arange(96), -S[:, j])) if r != 64 + j][:4]
        assert nb[64 + j, :4].tolist() == want, j
        assert nb[64 + j].tolist() == [r for r in np.lexsort((np.arange(96), -S[:, j])) if r != 64 + j][:8], j


def test_every_refusal_of_an_insert():
    G.check_insert_args(32, 100, 100, 140, 140, 64)
    G.check_insert_args(8, 100, 100, 100, 140, 31)
    for args, part in (((40, 100, 100, 140, 140, 64), "degree=40"), ((32, 100, 99, 140, 140, 64), "lo=99"), ((32, 100, 101, 140, 140, 64), "lo=101"),
                       ((32, 100, 100, 141, 140, 64), "hi=141"), ((32, 100, 100, 99, 140, 64), "hi=99"), ((32, 100, 100, 140, 140, 30), "insert_ef=30"),
                       ((32, 100, 100, 140, 140, 513), "insert_ef=513"), ((32, 100, 100, 140, 140, 64.0), "insert_ef=64.0"),
                       ((32, 100, True, 140, 140, 64), "lo=True")):
        with pytest.raises(ValueError, match=part):
            G.check_insert_args(*args)
    w = world()
    with pytest.raises(ValueError, match="lo=60"):
        G.insert_host(w["X"], w["base"], 60, 96, w["ent"])
    with pytest.raises(ValueError, match="hi=97"):
        G.insert_host(w["X"], w["base"], 64, 97, w["ent"])
    with pytest.raises(ValueError, match="insert_ef=16"):
        G.insert_host(w["X"], w["base"], 64, 96, w["ent"], insert_ef=16)
    with pytest.raises(ValueError, match="degree=40"):
        G.insert_host(w["X"], np.full((64, 40), -1, np.int32), 64, 96, w["ent"])
