"""The two pieces the row-selecting modes share on the device, against their numpy restatements (-m gpu): `codes.rescore_candidates`
against `codes.rescore_host`, bit for bit, and a collection with all four derived indexes attached (`build_ivf`, `build_binary`,
`build_pq`, `build_graph`) followed through add, delete, compact and add: after every step each index's device state is what its
restatement gives from the previous state, and each mode's `query` is its `*_host` search.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import binary as B
from arxiv_rag_amd import codes as C
from arxiv_rag_amd import graph as G
from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import pq as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, DIM, BASE = 300, 64, 7

_state = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clustered(n: int, seed: int, clusters: int = 8) -> np.ndarray:
    """fp16 [n, 64]: unit rows around `clusters` random directions (the cluster centres depend on `clusters` alone)"""
    centres = np.random.RandomState(clusters).randn(clusters, DIM)
    rs = np.random.RandomState(seed)
    x = centres[rs.randint(0, clusters, n)] + 0.6 * rs.randn(n, DIM)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


def shard():
    """300 clustered rows of dim 64 under idx_base = 7 with a BinaryIndex and a PqIndex over them, and 1025 queries; built once"""
    if not _state:
        from arxiv_rag_amd.index import ShardIndex
        X, Q = torch.from_numpy(clustered(N, 5)).to(DEV), torch.from_numpy(clustered(1025, 6)).to(DEV)
        index = ShardIndex(X, idx_base=BASE)
        _state.update(X=X, Xh=X.cpu().numpy(), Q=Q, Qh=Q.cpu().numpy(), index=index, bi=B.BinaryIndex.build(index),
                      pi=P.PqIndex.build(index, dsub=8, iters=2))
    return _state


def hand_made_lists(nq: int, R: int, k: int, seed: int):
    """(cand int32 [nq, R], count int64 [nq]): distinct rows per list, -1 behind `count[q]`; query 0 has fewer than k rows (where k > 1),
    query 1 none, queries 2 and 3 share their first row, the rest have 0..R rows."""
    rs = np.random.RandomState(seed)
    cand, count = np.full((nq, R), -1, np.int32), rs.randint(0, R + 1, nq).astype(np.int64)
    count[:4] = (k - 1, 0, R, R)[:min(nq, 4)]
    for q in range(nq):
        cand[q, :count[q]] = rs.permutation(N)[:count[q]]
    if nq >= 4:
        cand[3, 0] = cand[2, 0]
        cand[3, 1:] = [r for r in rs.permutation(N) if r != cand[2, 0]][:R - 1]
    return cand, count


@pytest.mark.parametrize("nq,R,k", [(nq, R, k) for nq in (0, 1) for R in (1, 33, 256) for k in (1, 32) if k <= R] + [(1025, 33, 32), (5, 256, 32)])
def test_rescore_candidates_is_rescore_host_through_both_indexes(nq, R, k):
    st = shard()
    cand, count = hand_made_lists(nq, R, k, seed=R * 100 + k)
    want_s, want_i, _ = C.rescore_host(st["Xh"], st["Qh"][:nq], cand, count, k)
    want_i = np.where(want_i >= 0, want_i + BASE, want_i)
    q16, cand_d, count_d = st["Q"][:nq].contiguous(), torch.from_numpy(cand).to(DEV), torch.from_numpy(count).to(DEV)
    for owner in (st["bi"], st["pi"]):
        s, i, c = C.rescore_candidates(owner.index, q16, cand_d, count_d, k, owner)
        assert c is count_d and s.shape == (nq, k) and i.dtype == torch.int64
        assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(bits(s.cpu().numpy()), bits(want_s)), type(owner).__name__
    if nq:                                                       # each index keeps its own workspace, and keeps it when it is large enough
        ws_b, ws_p = st["bi"]._ws_ivf, st["pi"]._ws_ivf
        assert ws_b is not None and ws_p is not None and ws_b.data_ptr() != ws_p.data_ptr()
        C.rescore_candidates(st["bi"].index, q16, cand_d, count_d, k, st["bi"])
        assert st["bi"]._ws_ivf is ws_b and st["pi"]._ws_ivf is ws_p


def test_search_of_both_indexes_is_candidates_then_the_one_rescore():
    st = shard()
    q16 = st["Q"][:9].contiguous()
    for owner in (st["bi"], st["pi"]):
        cand, _, count = owner.candidates(q16, 40)
        want = C.rescore_candidates(owner.index, q16, cand, count, 10, owner)
        got = owner.search(q16, 10, 40)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and type(owner).search is C.CodeIndex.search


def test_rescore_on_an_empty_index_returns_the_padding():
    from arxiv_rag_amd.index import ShardIndex
    st = shard()
    empty = B.BinaryIndex.build(ShardIndex(st["X"][:0].contiguous(), idx_base=BASE))
    cand, count = torch.full((3, 33), -1, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    s, i, c = C.rescore_candidates(empty.index, st["Q"][:3].contiguous(), cand, count, 32, empty)
    assert (s == float("-inf")).all() and (i == -1).all() and s.shape == i.shape == (3, 32) and c is count and empty._ws_ivf is None
    s, i, c = empty.search(st["Q"][:3].contiguous(), 32, 33)
    assert (s == float("-inf")).all() and (i == -1).all() and (c == 0).all()


# ---- all four indexes through a lifecycle ----------------------------------------------------------------------------------------------
def _meta(rows):
    return [{"chunk_id": f"c{r}", "text": f"text {r}"} for r in rows]


class Lifecycle:
    """A collection of 600 of 750 clustered rows (dim 64, capacity 1024) with the four indexes, and the host's picture of it: `rows`
    (which rows of `Xh` the collection holds, in order), `keep` (None or the rows not deleted) and `nb` (the graph's lists)."""

    def __init__(self, maintain: bool):
        from arxiv_rag_amd.store import HipCollection
        self.Xh, self.qe = clustered(750, 3), clustered(4, 4)
        self.q16 = torch.from_numpy(self.qe).to(DEV)
        self.col = col = HipCollection(self.Xh[:600], _meta(range(600)), capacity=1024)
        col.build_ivf(8, iters=3)
        col.build_binary()
        col.build_pq(dsub=8, iters=2)
        col.build_graph(degree=8, iters=2, maintain=maintain)
        self.rows, self.keep, self.nb = np.arange(600), None, col.graph.neighbors.cpu().numpy()
        self.centroids, self.centre_b = col.ivf.centroids_f16.clone(), col.binary.centre.cpu().numpy()
        self.codebooks, self.centre_p = col.pq.codebooks.cpu().numpy(), col.pq.centre.cpu().numpy()

    def check_state(self, graph: bool = True):
        col, X = self.col, self.Xh[self.rows]
        n = X.shape[0]
        assert col.ivf.index is col.binary.index is col.pq.index is col.index and int(col.index.n_rows) == n
        assert torch.equal(col.ivf.centroids_f16, self.centroids)
        assert torch.equal(col.ivf.labels, I.label_rows(torch.from_numpy(X).to(DEV), self.centroids)) and col.ivf.labels.shape[0] == n
        assert np.array_equal(col.binary.centre.cpu().numpy(), self.centre_b) and np.array_equal(col.pq.codebooks.cpu().numpy(), self.codebooks)
        assert np.array_equal(col.binary.codes.cpu().numpy().view(np.uint64), B.pack_host(X, self.centre_b))
        assert np.array_equal(col.pq.codes.cpu().numpy(), P.encode_host(X, self.codebooks, self.centre_p))
        if graph:
            assert np.array_equal(col.graph.neighbors.cpu().numpy(), self.nb) and col.graph.n_rows == n and not col.graph.stale
            assert col.graph.index is col.index

    def same(self, hit, want, counter):
        s, i, n = want[:3]
        assert hit[counter] == n.tolist(), counter
        for qi in range(4):
            assert hit["indices"][qi] == i[qi][i[qi] >= 0].tolist() and np.array_equal(bits(hit["scores"][qi]), bits(s[qi][i[qi] >= 0])), (counter, qi)

    def check_queries(self, graph: bool = True):
        col, X, qe, q16, keep = self.col, self.Xh[self.rows], self.qe, self.q16, self.keep
        probes = col.ivf.probe(q16, 8).cpu().numpy()
        self.same(col.query(query_embeddings=qe, n_results=5, nprobe=8),
                  I.search_host(X, col.ivf.order.cpu().numpy(), col.ivf.start.cpu().numpy(), probes, qe, 5, allow=keep), "ivf_scanned")
        self.same(col.query(query_embeddings=qe, n_results=5, binary_candidates=64),
                  B.search_host(X, B.pack_host(X, self.centre_b), B.pack_host(qe, self.centre_b), qe, 5, 64, allow=keep), "binary_count")
        self.same(col.query(query_embeddings=qe, n_results=5, pq_candidates=64),
                  P.search_host(X, P.encode_host(X, self.codebooks, self.centre_p), P.lut_host(qe, self.codebooks), qe, 5, 64, allow=keep), "pq_count")
        if graph:
            ent = col.graph.entries(q16, 8).cpu().numpy()
            self.same(col.query(query_embeddings=qe, n_results=5, graph_ef=64), G.search_host(X, self.nb, qe, ent, 5, 64, 64, allow=keep), "graph_scored")

    def add(self, new, graph: bool = True):
        lo = self.rows.shape[0]
        self.col.add(self.Xh[new], _meta(new))
        self.rows = np.concatenate([self.rows, new])
        if self.keep is not None:
            self.keep = np.concatenate([self.keep, np.ones(new.shape[0], bool)])
        if graph:
            ent = self.col.graph.entries(torch.from_numpy(self.Xh[new]).to(DEV), 8).cpu().numpy()
            self.nb, _ = G.insert_host(self.Xh[self.rows], self.nb, lo, lo + new.shape[0], ent, insert_ef=self.col.graph.insert_ef)

    def delete(self, gone):
        assert self.col.delete(ids=[f"c{r}" for r in self.rows[gone]]) == len(gone)
        self.keep = np.ones(self.rows.shape[0], bool)
        self.keep[gone] = False

    def compact(self, graph: bool = True):
        mapping = self.col.compact()
        assert np.array_equal(mapping >= 0, self.keep)
        if graph:
            self.nb = G.remap_host(self.nb[self.keep], self.keep)
        self.rows, self.keep = self.rows[self.keep], None


def test_four_indexes_follow_add_delete_compact_and_add():
    life = Lifecycle(maintain=True)
    assert life.col.graph.maintain and life.col.graph.insert_ef == 64
    gone = sorted(set(range(0, 700, 5)) | {r for r in range(641, 653) if r % 5})                 # 150 rows
    steps = (lambda: None, lambda: life.add(np.arange(600, 700)), lambda: life.delete(gone), life.compact, lambda: life.add(np.arange(700, 750)))
    for step in steps:
        step()
        life.check_state()
        life.check_queries()
    assert life.rows.shape[0] == life.col.count() == 600


def test_without_maintain_the_graph_goes_stale_and_the_other_three_follow():
    life = Lifecycle(maintain=False)
    life.check_state()
    life.add(np.arange(600, 700), graph=False)
    assert life.col.graph.stale and life.col.graph.n_rows == 600
    with pytest.raises(ValueError) as err:
        life.col.query(query_embeddings=life.qe, n_results=5, graph_ef=64)
    assert str(err.value) == ("the graph index is stale: rows were added or compacted since build_graph(); run build_graph() again "
                              "(build_graph(maintain=True) keeps the graph usable across add and compact)")
    life.check_state(graph=False)
    life.check_queries(graph=False)
    life.col.build_graph(degree=8, iters=2)
    life.nb = life.col.graph.neighbors.cpu().numpy()
    life.check_state()
    life.check_queries()
