"""The numpy restatement of the graph search (`graph.search_host`, `assemble_host`), every Python-side refusal and the exports of
`arx_graph_search` (no GPU; INTEGRATION.md "Graph search").  The kernel is checked against the restatement in tests/test_gpu_graph.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import graph as G
from arxiv_rag_amd.topics import exact_scores_host
from arxiv_rag_amd.where import pack_bitmap
from tests.graph_cases import ring

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_graph_workspace_bytes": 8, "arx_graph_search": 21, "arx_graph_search_tuned": 22}
N, DIM = 300, 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_new_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        proto = re.search(rf"^int(?:32|64)_t {name}\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(_lib.EXPORTS[name][1]), name
        assert hasattr(lib, name), name
    ws = _lib.load().arx_graph_workspace_bytes                     # (n_rows, nq, dim, degree, k, ef, max_iters, n_entries)
    for legal in ((1000, 70, 768, 32, 10, 64, 64, 8), (1, 1, 64, 8, 1, 1, 1, 1), (10_000_000, 64, 8192, 64, 32, 512, 127, 64),
                  (1000, 1, 64, 8, 10, 512, 1016, 64), (1000, 1, 64, 32, 10, 256, 255, 32)):
        assert ws(*legal) > 0, legal
    for bad in ((1000, 1, 64, 32, 10, 256, 256, 8), (1000, 1, 64, 8, 10, 512, 1024, 1), (1000, 1, 64, 12, 10, 64, 64, 8),
                (1000, 1, 64, 72, 10, 64, 64, 8), (1000, 1, 64, 32, 33, 64, 64, 8), (1000, 1, 64, 32, 10, 9, 64, 8),
                (1000, 1, 64, 32, 10, 513, 1, 8), (1000, 1, 64, 32, 10, 64, 0, 8), (1000, 1, 64, 32, 10, 64, 1025, 8),
                (1000, 1, 64, 32, 10, 64, 64, 0), (1000, 1, 64, 32, 10, 64, 64, 65), (1000, 1, 96, 32, 10, 64, 64, 8),
                (0, 1, 64, 32, 10, 64, 64, 8), (1 << 31, 1, 64, 32, 10, 64, 64, 8), (1000, 0, 64, 32, 10, 64, 64, 8)):
        assert ws(*bad) < 0, bad
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert " graph " in build and "$BLD/graph.o" in build and "$f = graph" not in build      # built, linked, contraction at its default


# ---- search_host --------------------------------------------------------------------------------------------------------------------
def _rows(n=N, seed=5):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, DIM)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


def _ring(lo, hi, n=N):
    return ring(lo, hi, n)


def _brute(X, Q, k, rows=None):
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    s = np.full((Q.shape[0], k), -np.inf, np.float32)
    i = np.full((Q.shape[0], k), -1, np.int64)
    for q in range(Q.shape[0]):
        sc = exact_scores_host(X[rows], Q[q:q + 1])[:, 0]
        best = np.lexsort((rows, -sc))[:k]
        s[q, :best.shape[0]], i[q, :best.shape[0]] = sc[best], rows[best]
    return s, i


def test_connected_ring_fully_visited_is_the_brute_force_top_k():
    X, Q = _rows(), _rows(6, seed=9)
    ent = np.array([[7]] * 6, np.int32)
    s, i, scored, expanded = G.search_host(X, _ring(0, N), Q, ent, 10, 512, 1000)         # 1 + 1000 * 8 rows fit the visited table
    ws, wi = _brute(X, Q, 10)
    assert np.array_equal(i, wi) and np.array_equal(bits(s), bits(ws))
    assert scored.tolist() == [N] * 6 and expanded.tolist() == [N] * 6


def test_disconnected_rings_return_only_the_entry_ring():
    X, Q = _rows(), _rows(4, seed=9)
    nb = _ring(0, 150)
    nb[150:] = _ring(150, N)[150:]
    for entry, rows in ((20, np.arange(150)), (200, np.arange(150, N))):
        s, i, scored, _ = G.search_host(X, nb, Q, np.full((4, 1), entry, np.int32), 10, 512, 1000)
        ws, wi = _brute(X, Q, 10, rows)
        assert np.array_equal(i, wi) and np.array_equal(bits(s), bits(ws)) and scored.tolist() == [150] * 4


def test_bad_and_repeated_entries_and_neighbours_are_skipped():
    X, Q = _rows(), _rows(3, seed=9)
    nb = _ring(0, N)
    clean = G.search_host(X, nb, Q, np.full((3, 1), 7, np.int32), 10, 64, 20)
    dirty = np.concatenate([nb, nb[:, :4], np.full((N, 4), -1, np.int32)], axis=1)         # degree 16: repeats and -1
    dirty[:, 12], dirty[:, 13], dirty[:, 14] = N, np.iinfo(np.int32).max, np.arange(N)    # too large, and a self-loop
    ent = np.array([[-1, 7, N, 7, -5, np.iinfo(np.int32).max, 7, 7]] * 3, np.int32)
    got = G.search_host(X, dirty, Q, ent, 10, 64, 20)
    assert all(np.array_equal(a, b) for a, b in zip(clean, got))
    none = G.search_host(X, nb, Q, np.full((3, 2), -1, np.int32), 10, 64, 20)
    assert np.all(none[0] == -np.inf) and np.all(none[1] == -1) and none[2].tolist() == [0] * 3 and none[3].tolist() == [0] * 3


def test_identical_rows_tie_by_row_id_and_nan_ranks_last():
    X = _rows()
    X[200] = X[10]
    Q = X[10:11].copy()
    s, i, _, _ = G.search_host(X, _ring(0, N), Q, np.array([[0]], np.int32), 3, 512, 1000)
    assert i[0, :2].tolist() == [10, 200] and bits(s[0, 0]) == bits(s[0, 1])
    X[11] = np.nan
    s, i, _, _ = G.search_host(X, _ring(0, N), Q, np.array([[0]], np.int32), 32, 512, 1000)
    assert 11 not in i[0].tolist()
    s, i, scored, _ = G.search_host(X[:12], _ring(0, 12, 12), Q, np.array([[0]], np.int32), 12, 12, 12)
    assert i[0, -1] == 11 and bits(s[0, -1]) == 0x7FC00000 and scored[0] == 12 and not np.isnan(s[0, :-1]).any()


def test_one_iteration_scores_the_entries_and_the_first_parents_neighbours():
    X, Q = _rows(), _rows(2, seed=9)
    nb = _ring(0, N)
    ent = np.array([[50, 120]] * 2, np.int32)
    s, i, scored, expanded = G.search_host(X, nb, Q, ent, 10, 64, 1)
    for q in range(2):
        first = 50 if exact_scores_host(X[[50]], Q[q:q + 1])[0, 0] >= exact_scores_host(X[[120]], Q[q:q + 1])[0, 0] else 120
        rows = sorted({50, 120} | set(nb[first].tolist()))
        ws, wi = _brute(X, Q[q:q + 1], 10, rows)
        assert np.array_equal(i[q], wi[0]) and np.array_equal(bits(s[q]), bits(ws[0])) and scored[q] == 10 and expanded[q] == 1


def test_allow_returns_allowed_rows_and_walks_across_hidden_ones():
    X, Q = _rows(), _rows(4, seed=9)
    mask = np.zeros(N, bool)
    mask[200:260] = True                                         # the entry (row 7) and everything between are hidden bridges
    ent = np.full((4, 1), 7, np.int32)
    for allow in (mask, pack_bitmap(mask), pack_bitmap(mask).view(np.int64)):
        s, i, scored, _ = G.search_host(X, _ring(0, N), Q, ent, 10, 512, 1000, allow=allow)
        ws, wi = _brute(X, Q, 10, np.nonzero(mask)[0])
        assert np.array_equal(i, wi) and np.array_equal(bits(s), bits(ws)) and scored.tolist() == [N] * 4
    s, i, _, _ = G.search_host(X, _ring(0, N), Q, ent, 10, 16, 3, allow=mask)             # a short walk never reaches an allowed row
    assert np.all(i == -1) and np.all(s == -np.inf)


def test_a_query_answers_alone_what_it_answers_in_a_batch():
    X, Q = _rows(), _rows(5, seed=9)
    rs = np.random.RandomState(2)
    nb = rs.randint(0, N, (N, 8)).astype(np.int32)
    ent = rs.randint(0, N, (5, 4)).astype(np.int32)
    batch = G.search_host(X, nb, Q, ent, 10, 32, 12)
    for q in range(5):
        alone = G.search_host(X, nb, Q[q:q + 1], ent[q:q + 1], 10, 32, 12)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(alone, batch))
    assert (batch[2] < N).all() and (batch[3] == 12).all()


# ---- assemble_host ------------------------------------------------------------------------------------------------------------------
def test_assemble_host_on_a_hand_written_table():
    knn = np.array([[1, 2, 3, 4, 5],          # degree 8: H = 4, fwd = the first four
                    [0, 2, 3, 4, 5],
                    [0, 1, 3, 4, 5],
                    [0, 1, 2, 4, 5],
                    [5, 0, 1, 2, 3],
                    [4, 0, 1, -1, -1]], np.int32)
    want = np.array([[1, 2, 3, 4, 5, -1, -1, -1],        # rev(0) = 1 2 3 (pos 0), 4 5 (pos 1): 5 is new; later: 5, present
                     [0, 2, 3, 4, 5, -1, -1, -1],        # rev(1) = 0 (pos 0), 2 3 (pos 1), 4 5 (pos 2): 5 is new
                     [0, 1, 3, 4, 5, -1, -1, -1],        # rev(2) = 0 1 (pos 1), 3 (pos 2), 4 (pos 3)
                     [0, 1, 2, 4, 5, -1, -1, -1],        # rev(3) = 0 1 2 (pos 2): all present; later: 5
                     [5, 0, 1, 2, 3, -1, -1, -1],        # rev(4) = 5 (pos 0), 0 1 2 3 (pos 3): 3 is new; later: 3, present
                     [4, 0, 1, -1, -1, -1, -1, -1]], np.int32)          # rev(5) = 4 (pos 0): present
    got = G.assemble_host(knn, 8)
    assert np.array_equal(got, want)
    for row in got:
        v = row[row >= 0]
        assert len(set(v.tolist())) == v.shape[0] and np.all(row[v.shape[0]:] == -1)
    bad = knn.copy()
    bad[5, 3] = N                                                # an entry that names no row changes nothing
    bad[2, 4] = 2                                                # the row itself is no neighbour: row 2 loses its later entry
    got2 = G.assemble_host(bad, 8)
    assert np.array_equal(got2[[0, 1, 3, 4, 5]], want[[0, 1, 3, 4, 5]]) and got2[2].tolist() == [0, 1, 3, 4, -1, -1, -1, -1]
    with pytest.raises(ValueError, match="twice"):
        G.assemble_host(np.array([[1, 1], [0, 0]], np.int32), 8)


def test_assemble_host_on_random_lists_has_no_duplicates_and_a_clean_tail():
    rs = np.random.RandomState(4)
    n = 200
    knn = np.stack([rs.permutation(n)[:31] for _ in range(n)]).astype(np.int32)
    knn[rs.rand(n, 31) < 0.1] = -1
    for degree in (8, 16, 32):
        g = G.assemble_host(knn, degree)
        H = degree // 2
        for i, row in enumerate(g):
            v = row[row >= 0]
            assert len(set(v.tolist())) == v.shape[0] and np.all(row[v.shape[0]:] == -1) and i not in v
            valid = [r for r in knn[i].tolist() if r >= 0 and r != i]
            assert v[:min(H, len(valid))].tolist() == valid[:H]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_check_search_args():
    G.check_search_args(10, 64, 64, 32, 8)
    G.check_search_args(32, 512, 255, 32, 32)
    for args, part in (((0, 64, 64, 32, 8), "k=0"), ((33, 64, 64, 32, 8), "k=33"), ((10, 9, 64, 32, 8), "ef=9"), ((10, 513, 1, 32, 8), "ef=513"),
                       ((10, 64, 0, 32, 8), "max_iters=0"), ((10, 64, 1025, 8, 8), "max_iters=1025"), ((10, 64, 64, 12, 8), "degree=12"),
                       ((10, 64, 64, 72, 8), "degree=72"), ((10, 64, 64, 32, 0), "n_entries=0"), ((10, 64, 64, 32, 65), "n_entries=65"),
                       ((10, 64, 256, 32, 8), "visited table"), ((True, 64, 64, 32, 8), "k=True"), ((10, 64.0, 64, 32, 8), "ef=64.0")):
        with pytest.raises(ValueError, match=part):
            G.check_search_args(*args)
    assert G.max_iters_for(32, 8) == 255 and G.max_iters_for(8, 1) == 1023 and G.max_iters_for(64, 64) == 127


def test_every_refusal_of_check_query_with_graph():
    ok = dict(has_index=True, n_width=10)
    G.check_query_with_graph(64, **ok)
    G.check_query_with_graph(10, **ok)
    G.check_query_with_graph(512, **ok)
    for kw, part in ((dict(nprobe=4), "nprobe"), (dict(binary_candidates=40), "binary_candidates"), (dict(pq_candidates=40), "pq_candidates"),
                     (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"), (dict(min_score=0.1), "min_score"),
                     (dict(boost_weight=0.5), "boost_weight"), (dict(per_query_filters=True), "per-query filter lists"), (dict(world=2), "world"),
                     (dict(has_index=False), "build_graph"), (dict(stale=True), "stale"), (dict(n_entries=0), "graph_entries"),
                     (dict(n_entries=33), "graph_entries"), (dict(n_entries=8, n_entry_lists=4), "graph_entries"), (dict(n_width=33), "width")):
        with pytest.raises(ValueError, match=part):
            G.check_query_with_graph(64, **{**ok, **kw})
    for ef, part in ((9, "below k=10"), (513, "graph_ef=513"), (64.5, "graph_ef"), (None, "graph_ef")):
        with pytest.raises(ValueError, match=part):
            G.check_query_with_graph(ef, **ok)


def test_every_refusal_of_check_build_args():
    assert G.check_build_args(4096, 64, 32, None, 10) == 64
    assert G.check_build_args(10, 64, 8, None, 10) == 3 and G.check_build_args(10_000_000, 768, 32, None, 10) == 3162
    assert G.check_build_args(4096, 64, 32, 16, 10, nprobe=4, has_ivf=True) == 16
    for kw, part in ((dict(degree=40), "degree=40"), (dict(degree=12), "degree=12"), (dict(n_rows=0), "empty"), (dict(n_rows=1 << 31), "2\\^31"),
                     (dict(n_entry_lists=0), "n_entry_lists"), (dict(n_entry_lists=5000), "n_entry_lists"), (dict(nprobe=4), "go together"),
                     (dict(has_ivf=True), "go together"), (dict(dim=96), "dim"), (dict(iters=0), "iters")):
        a = {**dict(n_rows=4096, dim=64, degree=32, n_entry_lists=None, iters=10), **kw}
        with pytest.raises(ValueError, match=part):
            G.check_build_args(a["n_rows"], a["dim"], a["degree"], a["n_entry_lists"], a["iters"], nprobe=a.get("nprobe"), has_ivf=a.get("has_ivf", False))


def test_every_refusal_of_the_command_line_flags():
    import argparse
    from arxiv_rag_amd.generate_embeddings_parallel import build_parser, check_graph_args
    base = dict(graph_ef=64, graph_degree=32, graph_entries=8, queries="q.txt", nprobe=None, ivf_lists=None, binary_candidates=None,
                pq_candidates=None, boost_key=None, hybrid_alpha=None, group_by_paper=False, min_score=None, where_filters=None, top_k=10,
                rerank_model=None, rerank_top_k=32, mmr_lambda=None, mmr_fetch_k=32)
    assert check_graph_args(argparse.Namespace(**base)) is None
    assert check_graph_args(argparse.Namespace(**{**base, "graph_ef": None})) is None
    for kw, part in ((dict(graph_ef=0), "[1, 512]"), (dict(graph_ef=513), "[1, 512]"), (dict(graph_degree=12), "--graph-degree"),
                     (dict(graph_degree=40), "--graph-degree"), (dict(graph_entries=0), "--graph-entries"), (dict(graph_entries=33), "--graph-entries"),
                     (dict(queries=None), "--queries"), (dict(nprobe=4), "--nprobe"), (dict(ivf_lists=16), "--nprobe"),
                     (dict(binary_candidates=40), "--binary-candidates"), (dict(pq_candidates=40), "--pq-candidates"), (dict(boost_key="year"), "--boost-key"),
                     (dict(hybrid_alpha=0.5), "--hybrid-alpha"), (dict(group_by_paper=True), "--group-by-paper"), (dict(min_score=0.1), "--min-score"),
                     (dict(where_filters=[None]), "--where-file"), (dict(graph_ef=5), "below the 10 rows"),
                     (dict(graph_ef=20, mmr_lambda=0.5), "below the 32 rows"), (dict(graph_ef=20, rerank_model="m"), "below the 32 rows")):
        err = check_graph_args(argparse.Namespace(**{**base, **kw}))
        assert err and part in err, (kw, err)
    args = build_parser().parse_args(["in", "--queries", "q.txt", "--graph-ef", "64"])
    assert (args.graph_ef, args.graph_degree, args.graph_entries) == (64, 32, 8)
    assert build_parser().parse_args(["in"]).graph_ef is None
