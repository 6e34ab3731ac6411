"""Host side of topic clustering (INTEGRATION.md "Topics"; no GPU): the C ABI's new entry points and their argument checks (refused
before anything is launched), the numpy restatement (`topics.sums_host`, `topics.finish_host`) against plain float64
(tests/topics_fp64.py) within the derived bounds, every refusal of `kmeans`, and one tiny case worked by hand."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

from tests import topics_fp64 as R

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_cluster_sums": 11, "arx_cluster_sums_tuned": 13, "arx_cluster_sums_workspace_bytes": 3, "arx_cluster_finish": 8}
ARX_ERR_ARG = -1
U = 2.0 ** -24


def test_the_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert len(_lib.EXPORTS[name][1]) == n_args, name
    assert "cluster" in (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()


def test_workspace_bytes_formula_and_contract():
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    for n, C, dim in ((0, 1, 64), (1, 1, 64), (256, 7, 192), (257, 7, 192), (1 << 20, 1024, 768), (300, 4096, 8192)):
        assert lib.arx_cluster_sums_workspace_bytes(n, C, dim) == (math.ceil(n / 256) + C) * dim * 4
    for n, C, dim in ((-1, 1, 64), (1 << 31, 1, 64), (10, 0, 64), (10, 4097, 64), (10, 4, 32), (10, 4, 96), (10, 4, 8256)):
        assert lib.arx_cluster_sums_workspace_bytes(n, C, dim) == -1


def _refused(call, *needles):
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    assert call(lib) == ARX_ERR_ARG
    msg = lib.arx_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_argument_errors_are_returned_before_any_launch():
    p = 4096                                                    # a non-null, 16-byte aligned "pointer" that is never read
    big = 1 << 40
    ok = [p, 100, 64, p, 100, p, 4, p, big, p]                  # rows n_rows dim order n_members start C partials ws_bytes sums
    def sums(i, v, *needles, tuned=None):
        a = list(ok)
        a[i] = v
        if tuned is None:
            _refused(lambda l: l.arx_cluster_sums(*a, None), *needles)
        _refused(lambda l: l.arx_cluster_sums_tuned(*a, *(tuned or (256, 0)), None), *needles)
    sums(2, 96, "dim", "96"); sums(2, 0, "dim"); sums(2, 8256, "dim", "8256")
    sums(6, 0, "C=0"); sums(6, 4097, "C=4097")
    sums(1, -1, "n_rows", "-1"); sums(1, 1 << 31, "n_rows", str(1 << 31))
    sums(4, -2, "n_members", "-2"); sums(4, 1 << 31, "n_members")
    sums(0, None, "rows"); sums(0, p + 2, "rows", "aligned"); sums(3, None, "order"); sums(5, None, "start"); sums(7, None, "partials")
    sums(9, None, "sums"); sums(7, p + 4, "aligned")
    sums(8, (1 + 4) * 64 * 4 - 1, "ws_bytes", str((1 + 4) * 64 * 4))
    sums(2, 64, "block_threads", "100", tuned=(100, 1)); sums(2, 64, "block_threads", tuned=(2048, 1)); sums(2, 64, "block_threads", tuned=(0, 1))
    sums(2, 64, "runs_per_block", "65", tuned=(256, 65)); sums(2, 64, "runs_per_block", tuned=(256, -1))
    fin = [p, p, p, 4, 64, p, p]                                # sums start prev C dim out_f32 out_f16
    for i, name in ((0, "sums"), (1, "start"), (2, "prev"), (5, "out_f32"), (6, "out_f16")):
        a = list(fin)
        a[i] = None
        _refused(lambda l: l.arx_cluster_finish(*a, None), name)
    _refused(lambda l: l.arx_cluster_finish(p, p, p, 0, 64, p, p, None), "C=0")
    _refused(lambda l: l.arx_cluster_finish(p, p, p, 4, 100, p, p, None), "dim", "100")


SIZES = (0, 1, 255, 256, 257, 600, 131)


def hand_labels(n, sizes, seed):
    """labels with exactly these cluster sizes, the members interleaved over the rows."""
    assert sum(sizes) == n
    lab = np.concatenate([np.full(m, c) for c, m in enumerate(sizes)])
    return np.random.RandomState(seed).permutation(lab).astype(np.int32)


@pytest.mark.parametrize("dim", [64, 192])
def test_sums_host_against_float64_within_the_two_level_bound(dim):
    from arxiv_rag_amd import topics as T
    X = (np.random.RandomState(dim).randn(1500, dim) * 0.3).astype(np.float16)
    labels = hand_labels(1500, SIZES, 1)
    order, start, sizes = T.members_host(labels, len(SIZES))
    assert sizes.tolist() == list(SIZES) and all(np.all(np.diff(order[start[c]:start[c + 1]]) > 0) for c in range(len(SIZES)))
    S = T.sums_host(X, order, start)
    assert S.dtype == np.float32 and not S[0].any()
    S64, A64 = R.cluster_sums(X, labels, len(SIZES))
    for c, m in enumerate(SIZES):
        assert (np.abs(S[c].astype(np.float64) - S64[c]) <= R.sum_bound(m) * A64[c]).all(), c
    # the contract's order, spelled out for one cluster: runs of 256 members in ascending row order, then the runs in order
    rows = np.nonzero(labels == 5)[0]
    want = np.zeros(dim, np.float32)
    for a in range(0, 600, 256):
        p = np.zeros(dim, np.float32)
        for r in rows[a:a + 256]:
            p = p + X[r].astype(np.float32)
        want = want + p
    assert np.array_equal(S[5].view(np.uint32), want.view(np.uint32))


def test_sums_host_defined_behaviour_on_bad_members():
    from arxiv_rag_amd import topics as T
    X = np.random.RandomState(3).randn(40, 64).astype(np.float16)
    order = np.array([3, -1, 5, 40, 7, 9, 11], np.int32)
    got = T.sums_host(X, order, np.array([0, 5, 7]))
    want = T.sums_host(X, np.array([3, 5, 7, 9, 11], np.int32), np.array([0, 3, 5]))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert T.clamp_starts([0, 5, 3, 9, 6], 7).tolist() == [0, 5, 5, 7, 7] and T.clamp_starts([-4, 2], 7).tolist() == [0, 2]
    dec = T.sums_host(X, order, np.array([0, 5, 3, 99]))         # a start that decreases once: the clamped ranges [0, 5) [5, 5) [5, 7)
    assert np.array_equal(dec[[0, 2]].view(np.uint32), got.view(np.uint32)) and not dec[1].any()


@pytest.mark.parametrize("dim", [64, 192, 8192])
def test_finish_host_against_float64(dim):
    from arxiv_rag_amd import topics as T
    rs = np.random.RandomState(dim)
    S = (rs.randn(6, dim) * 20).astype(np.float32)
    S[2] = 0.0                                                  # an all-zero sum
    S[4, 0] = np.inf                                            # a norm that is not finite
    start = np.array([0, 10, 10, 20, 30, 40, 50])               # cluster 1 is empty
    prev = rs.randn(6, dim).astype(np.float32)
    c32, c16 = T.finish_host(S, start, prev)
    assert c32.dtype == np.float32 and c16.dtype == np.float16
    for c in (1, 2, 4):
        assert np.array_equal(c32[c].view(np.uint32), prev[c].view(np.uint32)), c
    want = R.normalise(S[[0, 3, 5]])
    assert (np.abs(c32[[0, 3, 5]] - want) <= 4 * dim * U * np.abs(want)).all()
    assert np.array_equal(c16.view(np.uint16), c32.astype(np.float16).view(np.uint16))
    # the fixed order of the sum of squares, spelled out
    v = np.zeros(64, np.float32)
    for d0 in range(0, dim, 64):
        v = v + S[0, d0:d0 + 64] * S[0, d0:d0 + 64]
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    assert len(set(v.view(np.uint32).tolist())) == 1 and v[0] == T.sum_squares_host(S[:1])[0]


def test_every_refusal_of_kmeans_is_a_value_error():
    from arxiv_rag_amd import topics as T
    ok = dict(n=100, dim=64, n_clusters=4, iters=3)
    T.check_args(**ok)
    bad = [dict(n_clusters=0), dict(n_clusters=101), dict(n_clusters=-1), dict(n_clusters=2.0), dict(n_clusters=True), dict(iters=0),
           dict(iters=-3), dict(iters=1.5), dict(dim=32), dict(dim=96), dict(dim=8256), dict(n=10000, n_clusters=4097),
           dict(init=np.zeros((3, 64), np.float32)), dict(init=np.zeros((4, 65), np.float32)), dict(init=np.zeros(64, np.float32)),
           dict(init=np.full((4, 64), np.nan, np.float32)), dict(init=np.full((4, 64), np.inf, np.float32))]
    for kw in bad:
        with pytest.raises(ValueError):
            T.check_args(**{**ok, **kw})
    assert T.check_args(n=10000, dim=64, n_clusters=4096, iters=1) is None
    init = T.check_args(**ok, init=np.ones((4, 64), np.float64))
    assert init.dtype == np.float32 and init.flags["C_CONTIGUOUS"]
    X = np.zeros((10, 64), np.float16)
    for kw in (dict(n_clusters=11), dict(n_clusters=2, iters=0), dict(n_clusters=2, init=np.zeros((2, 63)))):
        with pytest.raises(ValueError):
            T.kmeans_host(X, **kw)
    with pytest.raises(ValueError):                             # the device entry refuses before it touches a device
        T.kmeans(X, 2)


def test_cli_flags_and_their_refusals(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    P = GEN.build_parser()
    a = P.parse_args(["in"])
    assert (a.topics, a.topics_iters, a.topics_seed) == (None, 20, 0) and GEN.check_topics_args(a) is None
    ok = ["in", "--queries", "q.txt", "--topics", "12", "--topics-iters", "5", "--topics-seed", "3"]
    a = P.parse_args(ok)
    assert (a.topics, a.topics_iters, a.topics_seed) == (12, 5, 3) and GEN.check_topics_args(a) is None
    assert "--queries" in GEN.check_topics_args(P.parse_args(["in", "--topics", "12"]))
    assert "[1, 4096]" in GEN.check_topics_args(P.parse_args(ok[:3] + ["--topics", "0"]))
    assert "[1, 4096]" in GEN.check_topics_args(P.parse_args(ok[:3] + ["--topics", "4097"]))
    assert "--topics-iters 0" in GEN.check_topics_args(P.parse_args(ok[:5] + ["--topics-iters", "0"]))
    a = P.parse_args(ok)
    a.where_filters = [None, {"section": "Methods"}]
    assert "--where-file" in GEN.check_topics_args(a)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in GEN.check_topics_args(P.parse_args(ok))


def test_default_init_rows_are_the_documented_draw():
    from arxiv_rag_amd import topics as T
    got = T.default_init_rows(1000, 16, 5)
    assert got.tolist() == sorted(np.random.default_rng(5).choice(1000, 16, replace=False).tolist()) and len(set(got.tolist())) == 16


def test_tiny_case_by_hand_empty_clusters_and_ties():
    """Six rows on three axes of a 64-dim space; centroids 0 and 1 start identical, centroid 3 starts away from every row.
         rows 0, 1 = e0      rows 2, 3 = e1      row 4 = (e0 + e1) / sqrt 2 exactly tied between e0 and e1      row 5 = e2
         init: c0 = c1 = e0, c2 = e1, c3 = -e2, c4 = e2
    Assign 1: rows 0, 1 tie between c0 and c1 -> the lower, 0; rows 2, 3 -> 2; row 4 scores 0.707 against c0, c1 and c2 -> the lowest,
    0; row 5 -> 4.  Sizes 3 0 2 0 1.  Update: c0 = normalised (2 + 0.707, 0.707, 0 ...) = (0.968, 0.253); c1 and c3 are empty and keep
    their values, so c1 is still e0.
    Assign 2: rows 0, 1 score 0.968 against c0 and 1 against c1 -> 1 (an empty cluster is not relocated, but it can win rows back);
    row 4 scores 0.86 against c0 and 0.707 against c1, c2 -> stays.  Two labels change.  Update: c0 = row 4 normalised, c1 = e0.
    Assign 3: nothing changes; the loop stops with iterations = 3 and the centroids assign 3 used.  c3 = -e2 was empty throughout."""
    from arxiv_rag_amd import topics as T
    e = np.eye(64, dtype=np.float32)
    h = np.float16(1 / np.sqrt(2))
    X = np.stack([e[0], e[0], e[1], e[1], h * (e[0] + e[1]), e[2]]).astype(np.float16)
    init = np.stack([e[0], e[0], e[1], -e[2], e[2]])
    r = T.kmeans_host(X, 5, iters=10, init=init)
    assert [lab.tolist() for lab in r["labels_history"]] == [[0, 0, 2, 2, 0, 4], [1, 1, 2, 2, 0, 4], [1, 1, 2, 2, 0, 4]]
    assert r["labels"].tolist() == [1, 1, 2, 2, 0, 4] and r["sizes"].tolist() == [1, 2, 2, 0, 1]
    assert r["iterations"] == 3 and r["changed"] == [6, 2, 0]
    assert np.array_equal(r["centroids"][1], e[0]) and np.array_equal(r["centroids"][3], -e[2])     # c3 empty: the init value, bit for bit
    assert np.array_equal(r["centroids"][2], e[1]) and np.array_equal(r["centroids"][4], e[2])
    assert np.allclose(r["centroids"][0][:2], 1 / np.sqrt(2), atol=1e-6) and not r["centroids"][0][2:].any()
    two = T.kmeans_host(X, 5, iters=2, init=init)               # stopped after assign 2: c1 was empty in the one update and kept e0
    s = np.array([2 + float(h), float(h)])
    assert np.allclose(two["centroids"][0][:2], s / np.linalg.norm(s), atol=1e-6) and np.array_equal(two["centroids"][1], e[0])
    assert two["iterations"] == 2 and two["sizes"].tolist() == [1, 2, 2, 0, 1]
    c16 = r["centroids_f16"].astype(np.float64)
    want = np.mean([1.0, 1.0, 1.0, 1.0, float(h) * (c16[0, 0] + c16[0, 1]), 1.0])
    assert abs(r["objective"] - want) < 1e-12
    one = T.kmeans_host(X, 5, iters=1, init=init)               # iters = 1: one assign, the centroids it used are the init
    assert one["iterations"] == 1 and np.array_equal(one["centroids"], init) and one["labels"].tolist() == [0, 0, 2, 2, 0, 4]
    # the default init: rows 0 and 1 are identical, so a draw that holds both gives two identical centroids
    full = T.kmeans_host(X, 6, iters=5, seed=0)
    assert full["sizes"].tolist() == [2, 0, 2, 0, 1, 1] and full["labels"].tolist() == [0, 0, 2, 2, 4, 5]
