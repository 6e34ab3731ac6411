"""The numpy restatement of the binary-code search (`binary.pack_host`, `candidates_host`, `search_host`), every Python-side refusal
and the exports of `arx_binary_pack` / `arx_binary_candidates` (no GPU; INTEGRATION.md "Binary-code search").  The C entry points'
argument refusals need the HIP runtime loaded and are checked in tests/test_gpu_binary.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import binary as B
from arxiv_rag_amd import ivf as I
from arxiv_rag_amd.where import pack_bitmap

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_binary_pack": 6, "arx_binary_workspace_bytes": 4, "arx_binary_candidates": 13, "arx_binary_candidates_tuned": 14}


def _rows(n, dim, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(-4, 5, (n, dim)).astype(np.float16)       # small integers: many zeros, many values equal to a centre entry


@pytest.mark.parametrize("dim", [64, 128])
def test_pack_host_against_a_per_element_loop(dim):
    X = _rows(9, dim, dim)
    X[0, :6] = (np.nan, np.inf, -np.inf, 0.0, -0.0, 65504.0)
    X[1, -3:] = (np.nan, -0.0, np.inf)
    centre = np.random.RandomState(1).randint(-2, 3, dim).astype(np.float32)
    centre[5] = np.inf                                           # nothing is above it, not even +inf
    X[2] = centre.astype(np.float16)                             # a row equal to the centre: all zero bits
    for c in (None, centre):
        got = B.pack_host(X, c)
        assert got.dtype == np.uint64 and got.shape == (9, dim // 64)
        for r in range(X.shape[0]):
            for j in range(dim):
                x, cj = np.float32(X[r, j]), np.float32(0.0 if c is None else c[j])
                want = bool(x > cj) if not np.isnan(x) else False
                assert (int(got[r, j >> 6]) >> (j & 63)) & 1 == int(want), (r, j)
        bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")      # the row bitmaps' convention
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits.astype(bool), X.astype(np.float32) > (0 if c is None else c))
    z = B.pack_host(X, None)
    assert (int(z[0, 0]) & 0x3f) == 0b100010                     # NaN 0, +inf 1, -inf 0, +0 0, -0 0, 65504 1
    assert not B.pack_host(X, centre)[2].any()
    assert B.pack_host(X[:0], None).shape == (0, dim // 64)
    for bad in (X.astype(np.float32), X[0], np.zeros((2, 96), np.float16), np.zeros((2, 8256), np.float16)):
        with pytest.raises(ValueError):
            B.pack_host(bad)


def _brute_candidates(codes, qcodes, R, mask):
    out = []
    for q in range(qcodes.shape[0]):
        tuples = sorted((sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(codes[r], qcodes[q])), r) for r in range(codes.shape[0]) if mask[r])
        out.append(tuples[:R])
    return out


@pytest.mark.parametrize("dim", [64, 192])
def test_candidates_host_against_a_brute_force_sort(dim):
    X, Q = _rows(150, dim, 3), _rows(5, dim, 4)
    X[77] = X[12]
    Q[0] = X[12]
    codes, qcodes = B.pack_host(X), B.pack_host(Q)
    mask = np.random.RandomState(5).rand(150) < 0.5
    garbage = pack_bitmap(np.ones(150, bool)).copy()
    garbage[-1] |= np.uint64(0xffff) << np.uint64(48)            # bits beyond n_rows
    for allow, m in ((None, np.ones(150, bool)), (mask, mask), (pack_bitmap(mask), mask), (pack_bitmap(mask).view(np.int64), mask),
                     (np.zeros(150, bool), np.zeros(150, bool)), (garbage, np.ones(150, bool))):
        for R in (1, 10, 256):
            cand, dist, count = B.candidates_host(codes, qcodes, R, allow)
            assert cand.dtype == np.int32 and dist.dtype == np.int32 and count.dtype == np.int64 and cand.shape == (5, R)
            for q, want in enumerate(_brute_candidates(codes, qcodes, R, m)):
                n = len(want)
                assert count[q] == n == min(R, int(m.sum()))
                assert [(int(d), int(r)) for d, r in zip(dist[q, :n], cand[q, :n])] == want
                assert (cand[q, n:] == -1).all() and (dist[q, n:] == -1).all()
    cand, dist, _ = B.candidates_host(codes, qcodes, 10)
    assert cand[0, :2].tolist() == [12, 77] and dist[0, :2].tolist() == [0, 0]     # ties go to the lower row
    e = B.candidates_host(codes[:0], qcodes, 4)
    assert (e[0] == -1).all() and (e[1] == -1).all() and e[2].tolist() == [0] * 5


@pytest.mark.parametrize("dim", [64, 192])
def test_search_host_equals_the_ivf_restatement_over_the_candidate_lists(dim):
    X, Q = _rows(150, dim, 6), _rows(7, dim, 7)
    codes, qcodes = B.pack_host(X), B.pack_host(Q)
    mask = np.random.RandomState(8).rand(150) < 0.6
    for allow in (None, mask):
        for k, R in ((1, 1), (10, 10), (10, 40), (32, 256)):
            s, i, n = B.search_host(X, codes, qcodes, Q, k, R, allow)
            cand, _, count = B.candidates_host(codes, qcodes, R, allow)
            start = np.arange(Q.shape[0] + 1, dtype=np.int64) * R
            ws, wi, wn = I.search_host(X, cand.reshape(-1), start, np.arange(Q.shape[0], dtype=np.int32)[:, None], Q, k)
            assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(i, wi) and np.array_equal(n, wn) and np.array_equal(n, count)
    # every row a candidate: the exact ranking
    s, i, _ = B.search_host(X, codes, qcodes, Q, 10, 256)
    sc = Q.astype(np.float64) @ X.astype(np.float64).T           # small integers: exact in f32 and in f64
    for q in range(Q.shape[0]):
        best = np.lexsort((np.arange(150), -sc[q]))[:10]
        assert i[q].tolist() == best.tolist() and np.array_equal(s[q].astype(np.float64), sc[q, best])


def test_python_side_refusals():
    B.check_args(32, 256, 8192)
    B.check_args(None, 1, 64)
    for R in (0, 257, 2.0, None, True):
        with pytest.raises(ValueError, match="n_candidates="):
            B.check_args(1, R)
    for k in (0, 33, 1.5, True):
        with pytest.raises(ValueError, match="k="):
            B.check_args(k, 40)
    with pytest.raises(ValueError, match="n_candidates=5 is below k=10"):
        B.check_args(10, 5)
    for dim in (0, 32, 96, 8256, 64.0):
        with pytest.raises(ValueError, match="dim="):
            B.check_args(1, 10, dim)
    assert B.check_centre("mean", 64) == "mean" and B.check_centre(None, 64) is None
    assert B.check_centre(np.ones(64, np.float64), 64).dtype == np.float32
    for bad in ("median", np.ones(65, np.float32), np.ones((1, 64), np.float32), np.ones(64, np.int32)):
        with pytest.raises(ValueError, match="centre"):
            B.check_centre(bad, 64)
    ok = dict(has_index=True, n_width=10)
    B.check_query_with_binary(40, **ok)
    for kw, part in ((dict(nprobe=4), "nprobe"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.1), "min_score"), (dict(per_query_filters=True), "per-query filter lists"), (dict(world=2), "world == 1"),
                     (dict(has_index=False), "build_binary"), (dict(n_width=33), "k=33")):
        with pytest.raises(ValueError, match=part):
            B.check_query_with_binary(40, **{**ok, **kw})
    for R in (0, 257, 1.5):
        with pytest.raises(ValueError, match="n_candidates="):
            B.check_query_with_binary(R, **ok)
    with pytest.raises(ValueError, match="n_candidates=5 is below k=10"):
        B.check_query_with_binary(5, **ok)


def test_the_front_ends_refuse_before_any_launch():
    """`retrieve`, `query` and `search_queries` raise from `check_query_with_binary` before they touch the index or the queries."""
    import torch
    from arxiv_rag_amd import generate_embeddings_parallel as G
    from arxiv_rag_amd.retrieval import retrieve
    from arxiv_rag_amd.store import HipCollection
    q = torch.zeros((2, 64), dtype=torch.float16)
    with pytest.raises(ValueError, match="build_binary"):
        retrieve(None, q, None, 10, binary_candidates=40)
    for kw, part in ((dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(nprobe=4, ivf=object()), "nprobe"), (dict(grouped=True), "group_by"),
                     (dict(min_score=0.2), "min_score"), (dict(where=[None, None]), "per-query filter lists"), (dict(world=2), "world == 1")):
        with pytest.raises(ValueError, match=part):
            retrieve(None, q, None, 10, binary_candidates=40, binary=object(), **kw)
    with pytest.raises(ValueError, match="is below k=10"):
        retrieve(None, q, None, 10, binary_candidates=5, binary=object())
    col = HipCollection.__new__(HipCollection)
    col.world, col._keep, col._deleted = 1, None, None
    e = np.zeros((1, 64), np.float32)
    with pytest.raises(ValueError, match="build_binary"):
        col.query(query_embeddings=e, binary_candidates=40)
    col.binary = object()
    for kw, part in ((dict(nprobe=4), "nprobe"), (dict(where=[None]), "per-query filter lists"), (dict(min_score=0.5), "min_score"),
                     (dict(n_results=20, binary_candidates=10), "below k=20"), (dict(binary_candidates=300), "n_candidates=300")):
        with pytest.raises(ValueError, match=part):
            col.query(query_embeddings=e, **{"binary_candidates": 40, **kw})
    col.world = 2
    with pytest.raises(ValueError, match="build_binary needs world == 1"):
        col.build_binary()
    with pytest.raises(ValueError, match="nprobe"):
        G.search_queries(None, [], None, ["q"], binary_candidates=40, nprobe=4, ivf_lists=8)
    with pytest.raises(ValueError, match="binary_centre"):
        G.search_queries(None, [], None, ["q"], binary_candidates=40, binary_centre="median")


def test_cli_flags_and_refusals(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as G
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    p = G.build_parser()
    a = p.parse_args(["in", "--queries", "q.txt", "--binary-candidates", "128", "--binary-centre", "none"])
    assert (a.binary_candidates, a.binary_centre) == (128, "none") and G.check_binary_args(a) is None
    d = p.parse_args(["in"])
    assert (d.binary_candidates, d.binary_centre) == (None, "mean") and G.check_binary_args(d) is None
    for extra, part in ((["--binary-candidates", "0"], "--binary-candidates 0"), (["--binary-candidates", "257"], "--binary-candidates 257"),
                        (["--binary-candidates", "40", "--ivf-lists", "64", "--nprobe", "4"], "--nprobe"),
                        (["--binary-candidates", "40", "--hybrid-alpha", "0.5"], "--hybrid-alpha"),
                        (["--binary-candidates", "40", "--group-by-paper"], "--group-by-paper"),
                        (["--binary-candidates", "40", "--min-score", "0.3"], "--min-score")):
        msg = G.check_binary_args(p.parse_args(["in", "--queries", "q.txt"] + extra))
        assert msg is not None and part in msg, (extra, msg)
    assert "--queries" in G.check_binary_args(p.parse_args(["in", "--binary-candidates", "40"]))
    a.where_filters = [None]
    assert "--where-file" in G.check_binary_args(a)
    a.where_filters = None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in G.check_binary_args(a)
    assert G.main(["in", "--queries", "q.txt", "--binary-candidates", "999"]) == 2      # refused before the input directory is looked at


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
        proto = re.search(rf"^int(?:32|64)_t {name}\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        assert len(proto.split(",")) == n_args, name
    ws = lib.arx_binary_workspace_bytes
    ws.restype, ws.argtypes = _lib.EXPORTS["arx_binary_workspace_bytes"]
    assert ws(1000, 70, 64, 10) > 0 and ws(0, 1, 64, 1) > 0 and ws(2 ** 31 - 1, 1, 8192, 256) > 0
    assert ws(10 ** 7, 10 ** 6, 768, 256) <= 64 << 20           # bounded whatever the shard and the batch
    bad = [ws(1000, 70, 64, 0), ws(1000, 70, 64, 257), ws(1000, 70, 96, 10), ws(1000, 70, 0, 10), ws(1000, 70, 8256, 10),
           ws(-1, 70, 64, 10), ws(1 << 31, 70, 64, 10), ws(1000, 0, 64, 10)]
    assert bad == [-1] * len(bad)
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert " binary " in build and "$BLD/binary.o" in build
