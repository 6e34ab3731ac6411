"""The numpy restatement of the IVF probe search (`ivf.probe_bitmaps_host`, `ivf.search_host`), every Python-side refusal, the CLI
flags and the exports of `arx_ivf_search` (no GPU; INTEGRATION.md "IVF probe search")."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T
from arxiv_rag_amd.mutation import unpack_rows

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_ivf_workspace_bytes": 6, "arx_ivf_search": 21, "arx_ivf_search_tuned": 22}


def _world(dim=64, n=400, n_lists=9, nq=12, seed=0):
    """Well-separated rows: integer-valued halves, so every dot product is exact in f32 and in float64 and ties are real ties."""
    rs = np.random.RandomState(seed)
    X = rs.randint(-4, 5, (n, dim)).astype(np.float16)
    Q = rs.randint(-4, 5, (nq, dim)).astype(np.float16)
    labels = rs.randint(0, n_lists, n).astype(np.int32)
    order, start, _ = T.members_host(labels, n_lists)
    probes = rs.randint(-1, n_lists + 1, (nq, 4)).astype(np.int32)      # some invalid, some repeated
    return X, Q, labels, order, start, probes


def _brute(X, Q, labels, probes, k, mask=None):
    """float64 ranking of the rows whose label is a valid probe of the query: (score desc, row asc)."""
    n_lists = int(labels.max()) + 1
    sc = Q.astype(np.float64) @ X.astype(np.float64).T
    out_s, out_i, out_n = [], [], []
    for q in range(Q.shape[0]):
        vis = np.isin(labels, [c for c in probes[q] if 0 <= c < n_lists])
        if mask is not None:
            vis &= mask
        rows = np.nonzero(vis)[0]
        best = rows[np.lexsort((rows, -sc[q, rows]))][:k]
        out_s.append(sc[q, best]); out_i.append(best); out_n.append(rows.shape[0])
    return out_s, out_i, out_n


@pytest.mark.parametrize("dim", [64, 192])
def test_search_host_against_a_float64_ranking(dim):
    X, Q, labels, order, start, probes = _world(dim)
    assert labels.max() == 8
    mask = np.random.RandomState(3).rand(X.shape[0]) < 0.4
    from arxiv_rag_amd.where import pack_bitmap
    for allow, m in ((None, None), (mask, mask), (pack_bitmap(mask).view(np.int64), mask), (np.zeros(X.shape[0], bool), np.zeros(X.shape[0], bool))):
        for k in (1, 10, 32):
            s, i, n = I.search_host(X, order, start, probes, Q, k, allow=allow)
            bs, bi, bn = _brute(X, Q, labels, probes, k, m)
            assert s.dtype == np.float32 and i.dtype == np.int64 and n.tolist() == bn
            for q in range(Q.shape[0]):
                m_ = len(bi[q])
                assert i[q, :m_].tolist() == bi[q].tolist() and np.array_equal(s[q, :m_].astype(np.float64), bs[q])
                assert (i[q, m_:] == -1).all() and np.isneginf(s[q, m_:]).all()


def test_probe_bitmaps_host_and_the_clamps():
    X, Q, labels, order, start, probes = _world()
    maps = I.probe_bitmaps_host(order, start, probes, X.shape[0])
    assert maps.dtype == np.int64 and maps.shape == (probes.shape[0], 7)
    for q in range(probes.shape[0]):
        assert np.array_equal(unpack_rows(maps[q], X.shape[0]), np.isin(labels, [c for c in probes[q] if 0 <= c < 9]))
    # bad data: entries outside [0, n_rows) are dropped in place, start is read through clamp_starts
    bad_order = order.copy()
    bad_order[[3, 77]] = (-5, X.shape[0] + 3)
    bad_start = start.copy()
    bad_start[3], bad_start[5], bad_start[9] = -4, 10, 10 ** 6
    s = T.clamp_starts(bad_start, order.shape[0])
    assert (np.diff(s) >= 0).all() and s[-1] == order.shape[0]
    got = I.search_host(X, bad_order, bad_start, probes, Q, 5)
    keep = (bad_order >= 0) & (bad_order < X.shape[0])
    for q in range(probes.shape[0]):
        rows = np.concatenate([bad_order[s[c]:s[c + 1]][keep[s[c]:s[c + 1]]] for c in dict.fromkeys(probes[q].tolist()) if 0 <= c < 9] + [np.zeros(0, np.int32)])
        assert got[2][q] == rows.shape[0] and set(got[1][q][got[1][q] >= 0]) <= set(rows.tolist())
    repeated = I.search_host(X, order, start, np.array([[2, 2, 5, 2]]), Q[:1], 8)
    deduped = I.search_host(X, order, start, np.array([[2, 5]]), Q[:1], 8)
    assert all(np.array_equal(a, b) for a, b in zip(repeated, deduped))
    none = I.search_host(X, order, start, np.array([[-1, 9, 2 ** 31 - 1]]), Q[:1], 3)
    assert none[2].tolist() == [0] and (none[1] == -1).all() and np.isneginf(none[0]).all()


def test_max_list_rows_cuts_every_list_at_its_first_entries():
    """`max_list_rows` (the library's argument of that name) in the restatement: the answer is that of the lists rebuilt from the first
    `cut` entries of each, without the parameter; None and a cut at the longest list change nothing; a cut of 0 leaves nothing; a bad
    `order` entry keeps its place inside the cut (it is dropped after the cut, and no later entry moves up)."""
    X, Q, labels, order, start, probes = _world()
    n, sizes = X.shape[0], np.diff(start)
    mask = np.random.RandomState(4).rand(n) < 0.6
    fo = np.arange(Q.shape[0]) % 3 - 1                                    # -1 (no row), 0, 1
    kw = dict(allows=np.stack([mask, ~mask]), filter_of=fo, min_score=0.0)
    whole = I.search_many_host(X, order, start, probes, Q, 10, **kw)
    for cut in (None, int(sizes.max()), n):
        assert all(np.array_equal(a, b) for a, b in zip(I.search_many_host(X, order, start, probes, Q, 10, max_list_rows=cut, **kw), whole))
    assert 1 < 7 < sizes.min() and sizes.max() > 40
    for cut in (1, 7, 40, int(sizes.max()) - 1):
        kept = np.minimum(sizes, cut)
        cut_order = np.concatenate([order[start[c]:start[c] + kept[c]] for c in range(9)])
        cut_start = np.concatenate([[0], np.cumsum(kept)])
        got = I.search_many_host(X, order, start, probes, Q, 10, max_list_rows=cut, **kw)
        want = I.search_many_host(X, cut_order, cut_start, probes, Q, 10, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), cut
        assert (got[3] <= got[2]).all() and (cut > 7 or got[2].sum() < whole[2].sum() // 4) and (got[2][fo < 0] == 0).all()
        one = I.search_host(X, order, start, probes, Q, 10, allow=mask, max_list_rows=cut)
        assert all(np.array_equal(a, b) for a, b in zip(one, I.search_host(X, cut_order, cut_start, probes, Q, 10, allow=mask)))
        maps = I.probe_bitmaps_host(order, start, probes, n, max_list_rows=cut)
        assert np.array_equal(maps, I.probe_bitmaps_host(cut_order, cut_start, probes, n))
        plain = I.search_host(X, order, start, probes, Q, 10, max_list_rows=cut)
        assert plain[2].tolist() == [int(unpack_rows(m, n).sum()) for m in maps]
    none = I.search_many_host(X, order, start, probes, Q, 10, max_list_rows=0, **kw)
    assert (none[2] == 0).all() and (none[3] == 0).all() and (none[1] == -1).all() and np.isneginf(none[0]).all()
    assert not I.probe_bitmaps_host(order, start, probes, n, max_list_rows=0).any()
    # a bad entry at place 2 of list 4, a cut of 3: places 0 and 1 are seen, the bad entry takes the third, place 3 stays outside
    bad = order.copy()
    a = int(start[4])
    for value in (-5, n + 3):
        bad[a + 2] = value
        s, i, scanned = I.search_host(X, bad, start, np.array([[4]]), Q[:1], 10, max_list_rows=3)
        assert scanned.tolist() == [2] and sorted(i[0][i[0] >= 0].tolist()) == sorted(order[a:a + 2].tolist())
        assert I._visible_rows(bad, start, [4], n, 3).tolist() == order[a:a + 2].tolist()
        assert I._visible_rows(bad, start, [4], n, 4).tolist() == order[[a, a + 1, a + 3]].tolist()
        assert unpack_rows(I.probe_bitmaps_host(bad, start, np.array([[4, 4]]), n, max_list_rows=3)[0], n).sum() == 2
    # ... and a cut meets clamped starts: the cut counts from the clamped start of the list
    bad_start = start.copy()
    bad_start[3], bad_start[5] = -4, 10                                    # lists 2 and 4 become empty, 3 and 5 grow (clamp_starts)
    s_ = T.clamp_starts(bad_start, order.shape[0])
    assert s_[3] == s_[2] and s_[5] == s_[4] and s_[4] - s_[3] > sizes[3]
    assert I._visible_rows(order, bad_start, [3, 2, 5], n, 6).tolist() == np.concatenate([order[s_[3]:s_[3] + 6], order[s_[5]:s_[5] + 6]]).tolist()


def test_python_side_refusals():
    for k in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="k="):
            I.check_probe_args(k, 4, 16)
    for nprobe in (0, 129, 1.5, None, True):
        with pytest.raises(ValueError, match="nprobe="):
            I.check_probe_args(10, nprobe, 4096)
    with pytest.raises(ValueError, match="nprobe=17 exceeds the index's n_lists=16"):
        I.check_probe_args(10, 17, 16)
    I.check_probe_args(32, 128, 128)
    assert I.check_build_args(100000, 768, 64, 10, None) == 16384 and I.check_build_args(1000, 64, 64, 1, None) == 1000
    assert I.check_build_args(1000, 64, 8, 3, 500) == 500
    for args, part in (((1000, 96, 8, 10, None), "dim"), ((1000, 64, 0, 10, None), "n_clusters"), ((1000, 64, 4097, 10, None), "n_clusters"),
                       ((1000, 64, 8, 0, None), "iters"), ((1000, 64, 8, 10, 7), "train_rows"), ((1000, 64, 8, 10, 1001), "train_rows"),
                       ((1 << 31, 64, 8, 10, None), "n_rows")):
        with pytest.raises(ValueError, match=part):
            I.check_build_args(*args)
    ok = dict(has_index=True, n_lists=16)
    I.check_query_with_nprobe(4, **ok)
    for kw, part in ((dict(per_query_filters=True), "per-query filter lists"), (dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by=True), "group_by"),
                     (dict(min_score=0.1), "min_score"), (dict(world=2), "world == 1"), (dict(has_index=False), "build_ivf"), (dict(n_lists=3), "n_lists=3")):
        with pytest.raises(ValueError, match=part):
            I.check_query_with_nprobe(4, **{**ok, **kw})


def test_retrieve_and_the_collection_refuse_before_any_launch():
    """`retrieve` and `query` raise from `check_query_with_nprobe` before they touch the index or the queries (None here)."""
    from arxiv_rag_amd.retrieval import retrieve
    from arxiv_rag_amd.store import HipCollection
    import torch
    q = torch.zeros((2, 64), dtype=torch.float16)
    with pytest.raises(ValueError, match="build_ivf"):
        retrieve(None, q, None, 10, nprobe=4)
    with pytest.raises(ValueError, match="hybrid_alpha"):
        retrieve(None, q, None, 10, nprobe=4, ivf=object(), hybrid_alpha=0.5)
    col = HipCollection.__new__(HipCollection)
    col.world, col._keep, col._deleted = 1, None, None
    with pytest.raises(ValueError, match="build_ivf"):
        col.query(query_embeddings=np.zeros((1, 64), np.float32), nprobe=4)
    with pytest.raises(ValueError, match="per-query filter lists"):
        col.query(query_embeddings=np.zeros((1, 64), np.float32), nprobe=4, where=[None])
    col.world = 2
    with pytest.raises(ValueError, match="build_ivf needs world == 1"):
        col.build_ivf(8)


def test_a_query_without_nprobe_never_touches_ivf(monkeypatch):
    """Without `nprobe` the retrieval pipeline does not import the module: a poisoned entry in sys.modules would raise."""
    from arxiv_rag_amd import retrieval
    from arxiv_rag_amd.store import HipCollection
    monkeypatch.setitem(sys.modules, "arxiv_rag_amd.ivf", None)             # `from .ivf import ...` now raises ImportError
    col = HipCollection.__new__(HipCollection)
    col.world, col._keep, col._deleted = 1, None, None
    with pytest.raises(ValueError, match="pass query_embeddings"):         # the refusal after every check: nothing imported ivf
        col.query()
    with pytest.raises(ImportError):
        col.query(nprobe=4)

    class Index:
        def search_distributed(self, q, k, allow=None, n_allowed=None):
            import torch
            return torch.zeros((q.shape[0], k)), torch.zeros((q.shape[0], k), dtype=torch.int64)

    class Filters:
        def allow_of(self, where, where_document=None):
            return None, None
    import torch
    hit = retrieval.retrieve(Index(), torch.zeros((2, 64), dtype=torch.float16), Filters(), 5)
    assert hit.ids.shape == (2, 5) and hit.ivf_scanned is None


def test_cli_flags_and_refusals(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as G
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    p = G.build_parser()
    a = p.parse_args(["in", "--queries", "q.txt", "--ivf-lists", "64", "--nprobe", "8", "--ivf-iters", "5", "--ivf-seed", "3"])
    assert (a.ivf_lists, a.nprobe, a.ivf_iters, a.ivf_seed) == (64, 8, 5, 3) and G.check_ivf_args(a) is None
    d = p.parse_args(["in"])
    assert (d.ivf_lists, d.nprobe, d.ivf_iters, d.ivf_seed) == (None, None, 10, 0) and G.check_ivf_args(d) is None
    for extra, part in ((["--ivf-lists", "64"], "go together"), (["--nprobe", "4"], "go together"),
                        (["--ivf-lists", "4097", "--nprobe", "4"], "--ivf-lists 4097"), (["--ivf-lists", "0", "--nprobe", "1"], "--ivf-lists 0"),
                        (["--ivf-lists", "64", "--nprobe", "65"], "--nprobe 65"), (["--ivf-lists", "4096", "--nprobe", "129"], "--nprobe 129"),
                        (["--ivf-lists", "64", "--nprobe", "0"], "--nprobe 0"), (["--ivf-lists", "64", "--nprobe", "4", "--ivf-iters", "0"], "--ivf-iters 0"),
                        (["--ivf-lists", "64", "--nprobe", "4", "--hybrid-alpha", "0.5"], "--hybrid-alpha"),
                        (["--ivf-lists", "64", "--nprobe", "4", "--group-by-paper"], "--group-by-paper"),
                        (["--ivf-lists", "64", "--nprobe", "4", "--min-score", "0.3"], "--min-score")):
        msg = G.check_ivf_args(p.parse_args(["in", "--queries", "q.txt"] + extra))
        assert msg is not None and part in msg, (extra, msg)
    assert "--queries" in G.check_ivf_args(p.parse_args(["in", "--ivf-lists", "64", "--nprobe", "4"]))
    a.where_filters = [None]
    assert "--where-file" in G.check_ivf_args(a)
    a.where_filters = None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in G.check_ivf_args(a)
    assert G.main(["in", "--queries", "q.txt", "--nprobe", "4"]) == 2        # refused before the input directory is looked at
    with pytest.raises(ValueError, match="go together"):
        G.search_queries(None, [], None, ["q"], nprobe=4)


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
    ws = lib.arx_ivf_workspace_bytes
    ws.restype, ws.argtypes = _lib.EXPORTS["arx_ivf_workspace_bytes"]
    assert ws(1000, 7, 70, 3, 64, 10) > 0 and ws(0, 1, 1, 1, 64, 1) > 0
    assert ws(10 ** 7, 4096, 1024, 128, 768, 32) <= 64 << 20     # bounded whatever the shard: about 50 MB
    bad = [ws(1000, 7, 70, 3, 64, 33), ws(1000, 7, 70, 3, 64, 0), ws(1000, 7, 70, 129, 64, 10), ws(1000, 7, 70, 0, 64, 10),
           ws(1000, 7, 70, 3, 96, 10), ws(1000, 7, 70, 3, 8256, 10), ws(1000, 0, 70, 3, 64, 10), ws(1000, 4097, 70, 3, 64, 10),
           ws(1 << 31, 7, 70, 3, 64, 10), ws(-1, 7, 70, 3, 64, 10), ws(1000, 7, 0, 3, 64, 10)]
    assert bad == [-1] * len(bad)
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert " ivf;" in build and "ivf.o" in build
    csrc = ROOT / "arxiv_rag_amd" / "csrc"
    assert "exact_row_score(" in (csrc / "ivf.hip").read_text()
    assert sum(len(re.findall(r"float exact_row_score\(", p.read_text())) for p in csrc.iterdir() if p.is_file()) == 1
