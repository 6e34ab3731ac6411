"""The numpy restatement of the IVF probe search with a filter and a threshold per query (`ivf.search_many_host`), the switches of
`ivf.check_query_with_nprobe` and the exports of `arx_ivf_search_multi` (no GPU; INTEGRATION.md "IVF probe search")."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.where import pack_bitmap

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_ivf_multi_workspace_bytes": 6, "arx_ivf_search_multi": 25, "arx_ivf_search_multi_tuned": 26}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _world(dim=64, n=400, n_lists=9, nq=12, seed=0):
    """Integer-valued halves: every dot product is exact in f32, ties are real ties."""
    rs = np.random.RandomState(seed)
    X = rs.randint(-4, 5, (n, dim)).astype(np.float16)
    Q = rs.randint(-4, 5, (nq, dim)).astype(np.float16)
    labels = rs.randint(0, n_lists, n).astype(np.int32)
    order, start, _ = T.members_host(labels, n_lists)
    probes = rs.randint(-1, n_lists + 1, (nq, 4)).astype(np.int32)      # some invalid, some repeated
    masks = np.stack([np.ones(n, bool), np.zeros(n, bool), rs.rand(n) < 0.5, rs.rand(n) < 0.05])
    return X, Q, labels, order, start, probes, masks


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
    old, new = lib.arx_ivf_workspace_bytes, lib.arx_ivf_multi_workspace_bytes
    old.restype, old.argtypes = _lib.EXPORTS["arx_ivf_workspace_bytes"]
    new.restype, new.argtypes = _lib.EXPORTS["arx_ivf_multi_workspace_bytes"]
    for shape, slots in (((1000, 7, 70, 3, 64, 10), 16 * 70), ((0, 1, 1, 1, 64, 1), 1), ((10 ** 7, 4096, 1024, 128, 768, 32), 1 << 17)):
        assert new(*shape) == old(*shape) + (slots * 4 + 255) // 256 * 256       # the old layout and part_m [slots] behind it
    assert old(1000, 7, 70, 3, 64, 10) == 256 * (5 + 4 + 175 + 350 + 18)        # arx_ivf_workspace_bytes keeps its numbers
    assert new(1000, 7, 70, 3, 64, 33) == -1 and new(1000, 7, 70, 129, 64, 10) == -1 and new(1000, 7, 0, 3, 64, 10) == -1
    src = (ROOT / "arxiv_rag_amd" / "csrc" / "ivf.hip").read_text()
    assert len(re.findall(r"void ivf_scan_kernel\(", src)) == 1 and "atomicAdd(float" not in src      # one scan, no float atomics


def test_search_many_host_is_search_host_per_filter():
    X, Q, labels, order, start, probes, masks = _world()
    nq = Q.shape[0]
    fo = np.random.RandomState(1).randint(0, 4, nq)
    for k in (1, 10, 32):
        for allows in (masks, np.stack([pack_bitmap(m).view(np.int64) for m in masks])):
            s, i, n, h = I.search_many_host(X, order, start, probes, Q, k, allows=allows, filter_of=fo)
            assert s.dtype == np.float32 and i.dtype == n.dtype == h.dtype == np.int64 and np.array_equal(n, h)
            for q in range(nq):
                ws, wi, wn = I.search_host(X, order, start, probes[q:q + 1], Q[q:q + 1], k, allow=masks[fo[q]])
                assert np.array_equal(bits(s[q]), bits(ws[0])) and np.array_equal(i[q], wi[0]) and n[q] == wn[0]
        plain = I.search_many_host(X, order, start, probes, Q, k)                 # no filter: filter_of is not looked at
        want = I.search_host(X, order, start, probes, Q, k)
        assert all(np.array_equal(a, b) for a, b in zip(plain[:3], want)) and np.array_equal(plain[3], want[2])


def test_search_many_host_on_hand_built_lists():
    X, Q, labels, order, start, probes, masks = _world()
    nq = Q.shape[0]
    fo = np.arange(nq) % 4
    # a filter_of outside the range gives nothing
    bad = fo.copy()
    bad[[0, 5]] = (-1, 4)
    s, i, n, h = I.search_many_host(X, order, start, probes, Q, 10, allows=masks, filter_of=bad)
    good = I.search_many_host(X, order, start, probes, Q, 10, allows=masks, filter_of=fo)
    for q in range(nq):
        if q in (0, 5):
            assert n[q] == h[q] == 0 and (i[q] == -1).all() and np.isneginf(s[q]).all()
        else:
            assert all(np.array_equal(a[q], b[q]) for a, b in zip((s, i, n, h), good))
    # a NaN threshold gives nothing, +inf neither; scanned still counts the visible rows
    for thr in (np.nan, np.inf):
        s, i, n, h = I.search_many_host(X, order, start, probes, Q, 10, allows=masks, filter_of=fo, min_score=thr)
        assert np.array_equal(n, good[2]) and (h == 0).all() and (i == -1).all() and np.isneginf(s).all()
    # -inf gives the unfiltered answer with hits == scanned on finite rows
    s, i, n, h = I.search_many_host(X, order, start, probes, Q, 10, min_score=-np.inf)
    want = I.search_host(X, order, start, probes, Q, 10)
    assert np.array_equal(bits(s), bits(want[0])) and np.array_equal(i, want[1]) and np.array_equal(n, want[2]) and np.array_equal(h, n)
    # a threshold per query: ties at the threshold are kept, hits counts every qualifying row
    full = I.search_host(X, order, start, probes, Q, 400)
    thr = np.where(full[2] >= 3, full[0][:, 2], np.float32(0)).astype(np.float32)
    s, i, n, h = I.search_many_host(X, order, start, probes, Q, 5, min_score=thr)
    for q in range(nq):
        m = int(((full[1][q] >= 0) & (full[0][q] >= thr[q])).sum())
        assert h[q] == m and n[q] == full[2][q]
        assert np.array_equal(i[q, :min(m, 5)], full[1][q, :min(m, 5)]) and (i[q, min(m, 5):] == -1).all()
        assert (s[q][i[q] >= 0] >= thr[q]).all()
    assert (h >= 3).any() and (h < full[2]).any()
    # a repeated probe counts once
    rep = I.search_many_host(X, order, start, np.array([[2, 2, 5, 2]]), Q[:1], 8, allows=masks, filter_of=[2], min_score=-2000.0)
    ded = I.search_many_host(X, order, start, np.array([[2, 5]]), Q[:1], 8, allows=masks, filter_of=[2], min_score=-2000.0)
    assert all(np.array_equal(a, b) for a, b in zip(rep, ded)) and rep[3][0] == rep[2][0] == int((masks[2] & np.isin(labels, (2, 5))).sum())
    with pytest.raises(ValueError, match="min_score has shape"):
        I.search_many_host(X, order, start, probes, Q, 5, min_score=[0.1, 0.2])


def test_the_relaxed_refusals_pass_and_the_kept_ones_raise_their_old_messages():
    ok = dict(has_index=True, n_lists=16)
    I.check_query_with_nprobe(4, per_query_filters=True, allow_per_query_filters=True, **ok)
    I.check_query_with_nprobe(4, min_score=0.3, allow_min_score=True, **ok)
    I.check_query_with_nprobe(4, per_query_filters=True, min_score=0.3, allow_per_query_filters=True, allow_min_score=True, **ok)
    on = dict(allow_per_query_filters=True, allow_min_score=True)
    for kw, text in ((dict(per_query_filters=True, allow_min_score=True), "nprobe cannot be combined with per-query filter lists: the IVF search takes one bitmap per call"),
                     (dict(min_score=0.1, allow_per_query_filters=True), "nprobe cannot be combined with min_score: the range search reads every row"),
                     (dict(hybrid_alpha=0.5, **on), "nprobe cannot be combined with hybrid_alpha: the BM25 keyword search has no inverted lists of topics"),
                     (dict(group_by=True, **on), "nprobe cannot be combined with group_by: the grouped search reads every row"),
                     (dict(world=2, **on), "nprobe needs world == 1: more than one rank is out of scope"),
                     (dict(has_index=False, **on), "nprobe needs an IVF index: call build_ivf(n_lists) first"),
                     (dict(n_lists=3, **on), "nprobe=4 exceeds the index's n_lists=3"),
                     (dict(n_width=33, min_score=0.2, **on), "k=33 must be an integer in [1, 32] (the search's k limit)")):
        with pytest.raises(ValueError) as e:
            I.check_query_with_nprobe(4, **{**ok, **kw})
        assert str(e.value) == text


class _FakeIvf:
    """Records what `retrieve` asks of the index; returns empty lists."""
    n_lists = 16

    def __init__(self):
        self.calls = []

    def _out(self, q, k, extra):
        import torch
        nq = q.shape[0]
        return (torch.full((nq, k), float("-inf")), torch.full((nq, k), -1, dtype=torch.int64), torch.full((nq,), 7, dtype=torch.int64)) + extra

    def search(self, q, k, nprobe, allow=None):
        self.calls.append(("search", k, nprobe, allow))
        return self._out(q, k, ())

    def search_many(self, q, k, nprobe, allows=None, filter_of=None, min_score=None):
        import torch
        self.calls.append(("search_many", k, nprobe, allows, filter_of, min_score))
        return self._out(q, k, (torch.tensor([0, 40, 11][:q.shape[0]], dtype=torch.int64),))


class _FakeFilters:
    def allow_of(self, where, where_document=None):
        import torch
        return (None, None) if where is None else (torch.tensor([5, 6], dtype=torch.int64), 3)

    def per_query(self, nq, where, where_document=None):
        import torch
        return [torch.tensor([1, 2], dtype=torch.int64), torch.tensor([3, 4], dtype=torch.int64)], [0, 1, 0][:nq], [None, None]


def test_retrieve_routes_filter_lists_and_thresholds_through_search_many():
    import torch
    from arxiv_rag_amd.retrieval import retrieve
    q = torch.zeros((3, 64), dtype=torch.float16)
    ivf = _FakeIvf()
    hit = retrieve(None, q, _FakeFilters(), 10, nprobe=4, ivf=ivf, where=[{"a": 1}, None, {"a": 1}])       # a list: one call, a bitmap per filter
    name, k, nprobe, allows, fo, ms = ivf.calls[-1]
    assert (name, k, nprobe, ms) == ("search_many", 10, 4, None) and allows.tolist() == [[1, 2], [3, 4]] and fo.tolist() == [0, 1, 0]
    assert fo.dtype == torch.int32 and hit.ivf_scanned.tolist() == [7, 7, 7] and hit.ivf_hits.tolist() == [0, 40, 11] and hit.truncated is None
    hit = retrieve(None, q, _FakeFilters(), 10, nprobe=4, ivf=ivf, where={"a": 1}, min_score=0.25)          # one dict and a floor
    name, k, nprobe, allows, fo, ms = ivf.calls[-1]
    assert name == "search_many" and allows.tolist() == [[5, 6]] and fo.tolist() == [0, 0, 0]
    assert ms.dtype == np.float32 and ms.tolist() == [0.25] * 3 and hit.truncated == [False, True, True]
    hit = retrieve(None, q, _FakeFilters(), 10, nprobe=4, ivf=ivf, min_score=[0.1, 0.2, 0.3], n_candidates=32, reranked=True)
    name, k, nprobe, allows, fo, ms = ivf.calls[-1]
    assert (name, k, allows, fo) == ("search_many", 32, None, None) and np.array_equal(ms, np.float32([0.1, 0.2, 0.3]))
    assert hit.truncated == [False, True, False]
    hit = retrieve(None, q, _FakeFilters(), 10, nprobe=4, ivf=ivf, where={"a": 1})                          # neither: `IvfIndex.search`, as before
    assert ivf.calls[-1][0] == "search" and hit.ivf_hits is None and hit.truncated is None and hit.ivf_scanned.tolist() == [7, 7, 7]
    n = len(ivf.calls)
    for kw, text in ((dict(min_score=0.2, hybrid_alpha=0.5), "nprobe cannot be combined with hybrid_alpha"), (dict(where=[None] * 3, grouped=True), "group_by"),
                     (dict(min_score=0.2, world=2), "world == 1"), (dict(min_score=[0.1, 0.2]), "min_score has shape")):
        with pytest.raises(ValueError, match=text):
            retrieve(None, q, _FakeFilters(), 10, nprobe=4, ivf=ivf, **kw)
    with pytest.raises(ValueError, match="k=33"):
        retrieve(None, q, _FakeFilters(), 33, nprobe=4, ivf=ivf, min_score=0.2)
    with pytest.raises(ValueError, match="build_ivf"):
        retrieve(None, q, _FakeFilters(), 10, nprobe=4, where=[None] * 3)
    assert len(ivf.calls) == n                                                                              # refused before any search


def test_search_queries_and_the_front_ends_that_keep_their_refusals():
    """`search_queries` lets a `where` list and `min_score` through with `nprobe` (its later refusals show it got past them); the
    collection's `query` and the command line's `check_ivf_args` keep theirs."""
    from arxiv_rag_amd import generate_embeddings_parallel as G
    from arxiv_rag_amd.store import HipCollection

    class Shard:
        rows = np.zeros((100, 64), np.float16)
    with pytest.raises(ValueError, match="n_clusters"):                  # past the nprobe refusals, at the build's own check
        G.search_queries(None, [], Shard, ["q"], nprobe=4, ivf_lists=5000, where=[None], min_score=0.3)
    with pytest.raises(ValueError, match=r"k=33 must be an integer in \[1, 32\]"):
        G.search_queries(None, [], Shard, ["q"], top_k=33, nprobe=4, ivf_lists=16, min_score=0.3)
    with pytest.raises(ValueError, match="min_score cannot be combined with per-query filter lists"):        # without nprobe: as ever
        G.search_queries(None, [], Shard, ["q"], where=[None], min_score=0.3)
    with pytest.raises(ValueError, match="nprobe cannot be combined with hybrid_alpha"):
        G.search_queries(None, [], Shard, ["q"], nprobe=4, ivf_lists=16, where=[None], hybrid_alpha=0.5, hybrid_filters=True)
    a = G.build_parser().parse_args(["in", "--queries", "q.txt", "--ivf-lists", "64", "--nprobe", "8", "--min-score", "0.3"])
    assert "--min-score" in G.check_ivf_args(a)
    col = HipCollection.__new__(HipCollection)
    col.world, col._keep, col._deleted, col.ivf = 1, None, None, _FakeIvf()
    with pytest.raises(ValueError, match="per-query filter lists"):
        col.query(query_embeddings=np.zeros((1, 64), np.float32), nprobe=4, where=[None])
    with pytest.raises(ValueError, match="nprobe cannot be combined with min_score"):
        col.query(query_embeddings=np.zeros((1, 64), np.float32), nprobe=4, min_score=0.2)
