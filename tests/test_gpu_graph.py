"""arx_graph_search (csrc/graph.hip) against its numpy restatement `graph.search_host` on the device (-m gpu; INTEGRATION.md "Graph
search").  Every comparison is exact: score bits, ids, rows scored, iterations run."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import graph as G
from arxiv_rag_amd.topics import exact_scores_host
from arxiv_rag_amd.where import pack_bitmap
from tests.graph_cases import ring as _ring

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NQ, I32_MAX = 1000, 70, np.iinfo(np.int32).max


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def words(mask):
    return dev(pack_bitmap(mask).view(np.int64))


def unit_rows(n, dim, seed):
    X = np.random.RandomState(seed).randn(n, dim)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


_worlds = {}


def world(dim):
    """X [N, dim] (row 500 a copy of row 10), Q [70, dim] (query 0 = row 10), every pair's exact score, computed once per dim."""
    if dim not in _worlds:
        X, Q = unit_rows(N, dim, 1), unit_rows(NQ, dim, 2)
        X[500] = X[10]
        Q[0] = X[10]
        _worlds[dim] = (X, Q, exact_scores_host(X, Q), dev(X), dev(Q))
    return _worlds[dim]


def random_graph(degree, seed, n=N):
    """a random graph with about 5 % of its edges bad: -1, n, INT32_MAX, a self-loop or a repeat of the row's first edge"""
    rs = np.random.RandomState(seed)
    nb = rs.randint(0, n, (n, degree)).astype(np.int32)
    kind = rs.randint(0, 100, (n, degree))
    nb[kind == 0], nb[kind == 1], nb[kind == 2] = -1, min(n, I32_MAX), I32_MAX
    nb = np.where(kind == 3, np.arange(n, dtype=np.int32)[:, None], nb)
    nb[:, 1:] = np.where(kind[:, 1:] == 4, nb[:, :1], nb[:, 1:])
    return nb


def random_entries(n_entries, seed, n=N, nq=NQ):
    """entries with repeats and values outside [0, n); query 3's are all invalid"""
    rs = np.random.RandomState(seed)
    ent = rs.randint(-2, n + 2, (nq, n_entries)).astype(np.int32)
    if n_entries > 1:
        ent[:, -1] = ent[:, 0]
    if nq > 3:
        ent[3] = [(-1, n, I32_MAX)[j % 3] for j in range(n_entries)]
    return ent


def same(got, want):
    s, i, scored, expanded = (t.cpu().numpy() for t in got)
    assert np.array_equal(i, want[1])
    assert np.array_equal(bits(s), bits(want[0]))
    assert np.array_equal(scored, want[2]) and np.array_equal(expanded, want[3])


@pytest.mark.parametrize("dim,degree,k,ef,n_entries,max_iters", [
    (64, 8, 1, 1, 1, 64), (64, 32, 10, 64, 8, 64), (64, 64, 32, 512, 64, 127), (64, 8, 10, 512, 8, 200), (64, 32, 32, 32, 64, 7),
    (768, 32, 10, 10, 8, 64), (768, 64, 10, 64, 1, 40), (768, 8, 32, 64, 64, 1), (768, 32, 1, 512, 8, 100)])
def test_kernel_equals_the_restatement_bit_for_bit(dim, degree, k, ef, n_entries, max_iters):
    X, Q, S, Xd, Qd = world(dim)
    nb, ent = random_graph(degree, degree), random_entries(n_entries, n_entries + k)
    mask = np.random.RandomState(ef).rand(N) < 0.3
    for allow in (None, mask):
        want = G.search_host(X, nb, Q, ent, k, ef, max_iters, allow=allow, pair_scores=S)
        got = G.graph_search(Xd, dev(nb), Qd, dev(ent), k, ef, max_iters, allow=None if allow is None else words(allow))
        same(got, want)
        assert want[2][3] == 0 and np.all(want[1][3] == -1) and np.all(want[0][3] == -np.inf)      # the query without a valid entry
    if n_entries == 8 and degree == 32 and ef == 64:
        assert want[3].max() > 1 and want[2].max() > 64            # the walk walked


def test_every_launch_shape_and_every_batch_gives_the_same_bits():
    X, Q, S, Xd, Qd = world(768)
    nb, ent = dev(random_graph(32, 5)), dev(random_entries(8, 6))
    allow = words(np.random.RandomState(7).rand(N) < 0.3)
    for a in (None, allow):
        base = G.graph_search(Xd, nb, Qd, ent, 10, 64, 64, allow=a)
        for threads in (64, 128, 256):
            got = G.graph_search(Xd, nb, Qd, ent, 10, 64, 64, allow=a, threads=threads)
            assert all(torch.equal(x, y) for x, y in zip(got, base)), threads
        alone = [G.graph_search(Xd, nb, Qd[q:q + 1], ent[q:q + 1], 10, 64, 64, allow=a) for q in range(NQ)]
        for j in range(4):
            assert torch.equal(torch.cat([r[j] for r in alone]), base[j]), j
    with pytest.raises(Exception, match="threads=96"):
        G.graph_search(Xd, nb, Qd, ent, 10, 64, 64, threads=96)


def test_fully_walked_ring_equals_the_exact_search():
    from arxiv_rag_amd.index import ShardIndex
    X, Q, _, _, Qd = world(64)
    n = 400                                                      # ef = 512 >= n: every row stays in the beam and gets expanded
    Xd = dev(X[:n])
    idx = ShardIndex(Xd)
    nb, ent = dev(_ring(0, n, n)), dev(np.full((NQ, 1), 7, np.int32))
    s, i, scored, expanded = G.graph_search(Xd, nb, Qd, ent, 10, 512, n)
    es, ei = idx.search(Qd, 10)
    assert torch.equal(i, ei) and torch.equal(s.view(torch.int32), es.view(torch.int32))
    assert scored.tolist() == [n] * NQ and expanded.tolist() == [n] * NQ
    assert i[0, :1].tolist() == [10]                             # query 0 is row 10
    mask = np.random.RandomState(3).rand(n) < 0.3
    s, i, scored, _ = G.graph_search(Xd, nb, Qd, ent, 10, 512, n, allow=words(mask))
    es, ei = idx.search(Qd, 10, allow=words(mask))
    assert torch.equal(i, ei) and torch.equal(s.view(torch.int32), es.view(torch.int32)) and scored.tolist() == [n] * NQ


def test_identical_rows_tie_by_row_and_idx_base_offsets_the_ids():
    X, Q, S, Xd, Qd = world(64)
    nb, ent = _ring(0, N, N), np.full((NQ, 2), 8, np.int32)
    want = G.search_host(X, nb, Q, ent, 10, 64, 64, pair_scores=S)
    got = G.graph_search(Xd, dev(nb), Qd, dev(ent), 10, 64, 64, idx_base=1 << 33)
    same((got[0], torch.where(got[1] >= 0, got[1] - (1 << 33), got[1]), got[2], got[3]), want)
    nb2 = nb.copy()
    nb2[8, 0] = 500                                              # a shortcut: both copies are found, the lower row first
    want = G.search_host(X, nb2, Q[:1], ent[:1], 10, 64, 64, pair_scores=S[:, :1])
    assert want[1][0, :2].tolist() == [10, 500] and bits(want[0][0, 0]) == bits(want[0][0, 1])
    same(G.graph_search(Xd, dev(nb2), Qd[:1], dev(ent[:1]), 10, 64, 64), want)


def test_a_shape_over_the_visited_table_is_refused_before_launch():
    from arxiv_rag_amd import _lib
    X, Q, S, Xd, Qd = world(64)
    nb, ent = dev(random_graph(32, 5)), dev(random_entries(8, 6))
    lib = _lib.load()
    assert lib.arx_graph_workspace_bytes(N, NQ, 64, 32, 10, 256, 256, 8) < 0 < lib.arx_graph_workspace_bytes(N, NQ, 64, 32, 10, 256, 255, 8)
    with pytest.raises(_lib.ArxError, match="unsupported shape"):
        G.graph_search(Xd, nb, Qd, ent, 10, 256, 256)
    out_s = torch.full((NQ, 10), 7.0, device=DEV)
    out_i = torch.full((NQ, 10), 7, dtype=torch.int64, device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    for kw, part in ((dict(max_iters=256), "visited table"), (dict(ef=9), "ef=9"), (dict(k=33), "k=33"), (dict(degree=12), "degree=12"),
                     (dict(n_entries=65), "n_entries=65"), (dict(dim=96), "dim=96"), (dict(ws_bytes=8), "workspace too small")):
        a = {**dict(dim=64, degree=32, n_entries=8, k=10, ef=256, max_iters=255, ws_bytes=256), **kw}
        rc = lib.arx_graph_search(Xd.data_ptr(), N, a["dim"], nb.data_ptr(), a["degree"], Qd.data_ptr(), NQ, ent.data_ptr(), a["n_entries"], None,
                                  a["k"], a["ef"], a["max_iters"], out_s.data_ptr(), out_i.data_ptr(), None, None, 0, ws.data_ptr(), a["ws_bytes"], None)
        assert rc != 0 and part in lib.arx_last_error().decode(), (kw, lib.arx_last_error())
    torch.cuda.synchronize()
    assert bool((out_s == 7.0).all()) and bool((out_i == 7).all())                      # nothing was launched


def test_no_query_one_row_and_dim_8192():
    X, Q, S, Xd, Qd = world(64)
    nb, ent = dev(random_graph(32, 5)), dev(random_entries(8, 6))
    got = G.graph_search(Xd, nb, Qd[:0], ent[:0], 10, 64, 64)
    assert [tuple(t.shape) for t in got] == [(0, 10), (0, 10), (0,), (0,)]
    one, nb1, ent1 = X[:1], np.zeros((1, 8), np.int32), np.zeros((2, 3), np.int32)
    same(G.graph_search(dev(one), dev(nb1), Qd[:2], dev(ent1), 4, 8, 8), G.search_host(one, nb1, Q[:2], ent1, 4, 8, 8))
    Xw, Qw = unit_rows(256, 8192, 3), unit_rows(3, 8192, 4)
    nbw, entw = random_graph(16, 9, 256), random_entries(4, 10, 256, 3)
    want = G.search_host(Xw, nbw, Qw, entw, 10, 32, 20)
    same(G.graph_search(dev(Xw), dev(nbw), dev(Qw), dev(entw), 10, 32, 20), want)
    assert want[2].max() > 32


def test_nan_and_inf_rows_have_the_restatements_places():
    X, Q, _, _, Qd = world(64)
    X = X[:200].copy()
    X[20], X[21], X[22, 5] = np.nan, np.inf, -np.inf
    with np.errstate(all="ignore"):
        S = exact_scores_host(X, Q[:8])
        nb, ent = _ring(0, 200, 200), np.full((8, 1), 19, np.int32)
        for k, ef, mask in ((32, 512, None), (10, 16, None), (32, 512, np.arange(200) % 2 == 0)):
            want = G.search_host(X, nb, Q[:8], ent, k, ef, 200, allow=mask, pair_scores=S)
            same(G.graph_search(dev(X), dev(nb), Qd[:8], dev(ent), k, ef, 200, allow=None if mask is None else words(mask)), want)
        want = G.search_host(X[:32], _ring(0, 32, 32), Q[:8], ent, 32, 32, 32, pair_scores=S[:32])
    assert np.isnan(want[0][:, -1]).all() and (bits(want[0][:, -1]) == 0x7FC00000).all()   # NaN scores rank last, by row
    same(G.graph_search(dev(X[:32]), dev(_ring(0, 32, 32)), Qd[:8], dev(ent), 32, 32, 32), want)
