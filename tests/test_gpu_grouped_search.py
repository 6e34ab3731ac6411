"""Grouped exact search (`ShardIndex.search_grouped`, arx_topk_search_grouped; csrc/grouped.hip) on the GPU.

The oracle is not the code under test: a dense score table per query built from the EXISTING `arx_topk_search_filtered`, called with
bitmaps of 32 rows at a time and k = 32 (every row of the bitmap comes back, so the table holds the search's own bits of every
(query, row)), folded in numpy by the definition (INTEGRATION.md "Grouped results").  The new call's scores, ids and groups must equal
the folded table bit for bit, on every path; its scores are also held to float64 with the pass-B budget of tests/helpers.py
(`pass_b_budget`, as `check_topk_fp64` does)."""
import json

import numpy as np
import pytest

from tests.helpers import pass_b_budget, scores_fp64

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BASE = 1 << 33
NQ = 5


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _rows(n, d, seed):
    """Unit rows in loose clusters (so that papers compete) as fp16, and NQ queries near some of them."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    cent = torch.nn.functional.normalize(torch.randn((max(2, n // 40), d), generator=g, device="cuda"), dim=1)
    pick = torch.randint(cent.shape[0], (n,), generator=g, device="cuda")
    C_ = torch.nn.functional.normalize(cent[pick] + 0.5 * torch.randn((n, d), generator=g, device="cuda"), dim=1).half().contiguous()
    src = torch.randint(n, (NQ,), generator=g, device="cuda")
    Q_ = torch.nn.functional.normalize(C_[src].float() + 0.3 * torch.randn((NQ, d), generator=g, device="cuda"), dim=1).half().contiguous()
    return C_, Q_


def _group_of(lengths, n):
    """Runs of the given lengths (cycled until n rows), with values that are not dense: run j is 3 j + 5."""
    out, j = [], 0
    while len(out) < n:
        out += [3 * j + 5] * lengths[j % len(lengths)]
        j += 1
    return np.array(out[:n], np.int32)


def _pack(mask):
    from arxiv_rag_amd.where import pack_bitmap
    return torch.from_numpy(pack_bitmap(np.asarray(mask, bool)).view(np.int64)).cuda()


def _score_table(C_, Q_):
    """float32 [nq, n]: the bits the existing filtered search gives every (query, row), 32 rows of the shard at a time."""
    from arxiv_rag_amd.index import ShardIndex
    n, nq = C_.shape[0], Q_.shape[0]
    idx = ShardIndex(C_, idx_base=BASE)
    T = torch.full((nq, n), float("nan"), dtype=torch.float32, device="cuda")
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    for a in range(0, n, 32):
        cnt = min(32, n - a)
        bits = ((1 << cnt) - 1) << (a & 63)
        words[a >> 6] = bits - (1 << 64) if bits >= (1 << 63) else bits
        s, i = idx.search(Q_, 32, allow=words, n_allowed=cnt)
        assert (i[:, :cnt] >= BASE + a).all() and (i[:, :cnt] < BASE + a + cnt).all() and (i[:, cnt:] == -1).all()
        T.scatter_(1, i[:, :cnt] - BASE, s[:, :cnt])
        words[a >> 6] = 0
    assert not torch.isnan(T).any()
    return T.cpu().numpy()


def _fold(T, group_of, visible, P, m, base):
    """The definition, in numpy: per query the P best groups by (best visible score desc, its row asc), of each the m best visible rows
    by (score desc, row asc); (-inf, -1) / -1 padding."""
    nq = T.shape[0]
    S = np.full((nq, P, m), -np.inf, np.float32); I = np.full((nq, P, m), -1, np.int64); G = np.full((nq, P), -1, np.int32)
    rows = np.flatnonzero(visible)
    for q in range(nq):
        if rows.size == 0:
            continue
        order = rows[np.lexsort((rows, -T[q, rows].astype(np.float64)))]
        gs = group_of[order]
        uniq, first = np.unique(gs, return_index=True)
        for p, gv in enumerate(uniq[np.argsort(first)][:P]):
            mine = order[gs == gv][:m]
            G[q, p] = gv
            S[q, p, :mine.size] = T[q, mine]
            I[q, p, :mine.size] = mine + base
    return S, I, G


def _same(got, want, what):
    s, i, g = (t.cpu().numpy() for t in got)
    assert np.array_equal(i, want[1]), (what, "ids", i.tolist()[:1], want[1].tolist()[:1])
    assert np.array_equal(g, want[2]), (what, "groups")
    assert np.array_equal(s.view(np.int32), want[0].view(np.int32)), (what, "score bits")


def _check_fp64(C_, Q_, got, what):
    """Every returned score within B(D) |q| |c| (1 + 1e-3) of the float64 dot product: the manner of check_topk_fp64's pass-B test."""
    s, i, _ = got
    e = scores_fp64(Q_, C_)
    valid = i >= 0
    loc = (i - BASE).clamp(min=0).reshape(Q_.shape[0], -1)
    ej = e.gather(1, loc).reshape(i.shape)
    bound = pass_b_budget(C_.shape[1]) * Q_.double().norm(dim=1)[:, None, None] * C_.double().norm(dim=1)[loc].reshape(i.shape) * (1 + 1e-3)
    err = (s.double() - ej).abs()
    assert (err[valid] <= bound[valid]).all(), (what, "score outside B(D)")
    assert (torch.isinf(s[~valid]) & (s[~valid] < 0)).all(), (what, "padding")


def _index(C_, group_of):
    from arxiv_rag_amd.index import ShardIndex
    return ShardIndex(C_, idx_base=BASE).set_groups(group_of)


CASES = [
    dict(id="n1", d=64, n=1, runs=[1]),
    dict(id="n63-single-rows", d=64, n=63, runs=[1]),
    dict(id="n64-single-rows", d=128, n=64, runs=[1]),
    dict(id="n65-single-rows", d=64, n=65, runs=[1]),
    dict(id="one-paper-is-the-shard", d=64, n=700, runs=[700]),
    dict(id="runs-1-to-7", d=128, n=1500, runs=[1, 2, 3, 4, 5, 6, 7]),
    dict(id="runs-64-offset-0", d=64, n=64 * 9 + 3, runs=[64]),
    dict(id="runs-64-offset-32", d=64, n=64 * 9 + 3, runs=[32] + [64] * 40),
    dict(id="run-200-across-a-tile-edge", d=128, n=900, runs=[156, 200, 3, 41, 200, 7]),
    dict(id="mixed-12805", d=64, n=64 * 200 + 5, runs=[1, 9, 64, 2, 130, 5, 33, 200, 1, 1, 17]),
]
SHAPES = [(1, 1), (10, 3), (32, 8), (3, 8), (32, 1)]


@pytest.fixture(scope="module")
def tables():
    """The score table of every case, built once and left unchanged."""
    cache = {}

    def get(case):
        if case["id"] not in cache:
            C_, Q_ = _rows(case["n"], case["d"], 1000 + len(cache))
            cache[case["id"]] = (C_, Q_, _group_of(case["runs"], case["n"]), _score_table(C_, Q_))
        return cache[case["id"]]
    return get


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_grouped_search_equals_the_folded_score_table_on_every_path(hip, tables, case):
    """Per case, per (P, m) and per mask - none, all ones, half the rows, the best chunk of query 0's best paper hidden, that whole paper
    hidden, nothing visible - the library's choice, the scan, the exhaustive path and the scan with a one-entry candidate list return
    the folded table's bits.  P = 32 on the small shards is "fewer than P visible papers", m = 8 "papers with fewer than m visible rows"."""
    C_, Q_, group_of, T = tables(case)
    n = case["n"]
    idx = _index(C_, group_of)
    runs = np.diff(np.flatnonzero(np.r_[True, group_of[1:] != group_of[:-1], True]))
    assert idx.max_run_rows == runs.max() and idx.n_runs == runs.size
    rs = np.random.RandomState(n)
    everything = np.ones(n, bool)
    _, I0, G0 = _fold(T, group_of, everything, 1, 1, 0)
    hide_chunk = everything.copy(); hide_chunk[I0[0, 0, 0]] = False
    hide_paper = group_of != G0[0, 0]
    masks = [("none", None), ("ones", everything), ("rand50", rs.rand(n) < 0.5), ("best chunk hidden", hide_chunk),
             ("best paper hidden", hide_paper), ("zero", np.zeros(n, bool))]
    for P, m in SHAPES:
        for name, mask in masks:
            visible = everything if mask is None else mask
            want = _fold(T, group_of, visible, P, m, BASE)
            allow = None if mask is None else _pack(mask)
            for kw in (dict(), dict(path=1), dict(path=2), dict(path=1, cand_cap=1), dict(n_allowed=int(visible.sum()))):
                if (P, m) != (10, 3) and kw and kw != dict(path=2):
                    continue                                 # every path at (10, 3); elsewhere the library's choice and the exhaustive path
                got = idx.search_grouped(Q_, P, m, allow=allow, **kw)
                _same(got, want, (case["id"], P, m, name, kw))
            if name in ("none", "rand50") and (P, m) == (10, 3):
                _check_fp64(C_, Q_, got, (case["id"], name))
    # the masks do what their names say (query 0)
    if n > 1:
        s, i, g = idx.search_grouped(Q_[:1], 1, 1, allow=_pack(hide_chunk))
        assert int(i[0, 0, 0]) != I0[0, 0, 0] + BASE
        s, i, g = idx.search_grouped(Q_[:1], 32, 1, allow=_pack(hide_paper))
        assert G0[0, 0] not in g.cpu().numpy()


def test_exact_duplicate_rows_in_two_papers_tie_to_the_lower_row(hip):
    """Rows 10 and 300 (two papers) and rows 301 and 303 (inside the second paper) are copies of one row, which is also the query: both
    papers score the same bits, the paper of row 10 comes first; inside the second paper row 300 comes before 301 before 303."""
    C_, Q_ = _rows(640, 64, 7)
    C_[300] = C_[10]; C_[301] = C_[10]; C_[303] = C_[10]
    Q_ = C_[10:11].clone()
    group_of = _group_of([8], 640)
    T = _score_table(C_, Q_)
    assert T[0, 10].view(np.int32) == T[0, 300].view(np.int32) == T[0, 301].view(np.int32) == T[0, 303].view(np.int32) == T[0].max().view(np.int32)
    idx = _index(C_, group_of)
    for kw in (dict(), dict(path=2), dict(path=1, cand_cap=1)):
        got = idx.search_grouped(Q_, 4, 3, **kw)
        _same(got, _fold(T, group_of, np.ones(640, bool), 4, 3, BASE), kw)
        s, i, g = (t.cpu().numpy() for t in got)
        assert i[0, 0, 0] == BASE + 10 and g[0, 0] == group_of[10] and g[0, 1] == group_of[300]
        assert i[0, 1].tolist() == [BASE + 300, BASE + 301, BASE + 303]


def test_k_512_takes_the_scan_and_k_513_the_exhaustive_path_with_the_same_bits(hip, tables):
    """K = P S with S = floor((R + 62) / 64) + 1 (arxiv_rag_amd.grouping.select_count).  P = 32, R = 961: K = 512, the scan runs (it
    lists candidate groups).  P = 27, R = 1090: K = 513, the whole call is exhaustive (no candidate group is listed).  Both are a
    `max_run_rows` larger than the true one (200), as is 10^12: same bits as the folded table."""
    from arxiv_rag_amd.grouping import select_count
    C_, Q_, group_of, T = tables(CASES[-1])
    idx = _index(C_, group_of)
    everything = np.ones(C_.shape[0], bool)
    assert select_count(32, 961) == 512 and select_count(27, 1090) == 513 and idx.max_run_rows == 200
    for P, R, scan in ((32, 961, True), (27, 1090, False), (10, 10 ** 12, False), (10, 201, True)):
        got = idx.search_grouped(Q_, P, 2, max_run_rows=R)
        _same(got, _fold(T, group_of, everything, P, 2, BASE), (P, R))
        overflowed, cands = idx.grouped_stats()
        print(f"P={P} max_run_rows={R}: K={select_count(P, R)} overflowed={overflowed} candidate groups={cands}")
        assert overflowed == 0 and (cands > 0) == scan, (P, R, cands)
    want = _fold(T, group_of, everything, 10, 2, BASE)
    _same(idx.search_grouped(Q_, 10, 2, path=1), want, "path 1")
    _same(idx.search_grouped(Q_, 10, 2, path=2), want, "path 2")


def test_a_small_candidate_list_overflows_into_the_exhaustive_path_with_the_same_bits(hip):
    """48 copies of one row, one in each of 48 different 64-row groups, and that row as the query.  Runs of 5 rows: S = 2, P = 4, K = 8.
    On the host first: the copies' bits are the table's maximum in 48 > cand_cap = 16 groups and K <= 48, so the K-th largest group
    maximum is the copies' score and all 48 groups lie within 2 tau of it - the list must overflow."""
    from arxiv_rag_amd.grouping import select_count
    n, cap, P = 64 * 60 + 9, 16, 4
    C_, Q_ = _rows(n, 128, 11)
    at = np.arange(48) * 64 + (np.arange(48) * 13) % 64
    C_[torch.from_numpy(at).cuda()] = C_[7].clone()
    Q_ = torch.cat([C_[7:8], Q_[:2]]).contiguous()
    group_of = _group_of([5], n)
    T = _score_table(C_, Q_)
    gmax = np.array([T[0, a:a + 64].max() for a in range(0, n, 64)])
    top_groups = int((gmax.view(np.int32) == T[0].max().view(np.int32)).sum())
    K = select_count(P, 5)
    assert K == 8 and top_groups >= 48 > cap and K <= top_groups
    idx = _index(C_, group_of)
    want = _fold(T, group_of, np.ones(n, bool), P, 3, BASE)
    _same(idx.search_grouped(Q_, P, 3, path=1, cand_cap=cap), want, "overflow")
    overflowed, cands = idx.grouped_stats()
    print(f"cand_cap={cap}: overflowed queries={overflowed} candidate groups={cands}")
    assert overflowed >= 1
    _same(idx.search_grouped(Q_, P, 3), want, "default cap")
    assert idx.grouped_stats()[0] == 0


def test_a_query_gets_the_same_bits_alone_and_anywhere_in_a_batch_of_70_and_of_1100(hip, tables):
    C_, Q_, group_of, T = tables(CASES[5])
    idx = _index(C_, group_of)
    n = C_.shape[0]
    allow = _pack(np.random.RandomState(3).rand(n) < 0.7)
    alone = [tuple(t.cpu().numpy() for t in idx.search_grouped(Q_[b:b + 1], 10, 3, allow=allow)) for b in range(NQ)]
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    for nq in (70, 1100):
        batch = torch.nn.functional.normalize(torch.randn((nq, C_.shape[1]), generator=g, device="cuda"), dim=1).half()
        where = torch.randperm(nq, generator=g, device="cuda")[:NQ].cpu().tolist()
        for b, pos in enumerate(where):
            batch[pos] = Q_[b]
        for kw in (dict(), dict(path=2)):
            s, i, gr = (t.cpu().numpy() for t in idx.search_grouped(batch.contiguous(), 10, 3, allow=allow, **kw))
            for b, pos in enumerate(where):
                assert np.array_equal(i[pos], alone[b][1][0]) and np.array_equal(gr[pos], alone[b][2][0]), (nq, b, kw)
                assert np.array_equal(s[pos].view(np.int32), alone[b][0][0].view(np.int32)), (nq, b, kw)


def test_group_runs_info_and_set_groups(hip):
    from arxiv_rag_amd.index import ShardIndex
    lib = hip.load()

    def info(values):
        g = torch.tensor(values, dtype=torch.int32, device="cuda")
        out = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        hip.check(lib.arx_group_runs_info(g.data_ptr(), g.shape[0], out.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_group_runs_info")
        return out.tolist()
    assert info([0, 0, 1, 1, 1, 4, 9, 9]) == [3, 4]
    assert info([5] * 1000) == [1000, 1]
    assert info([7]) == [1, 1]
    assert info(list(range(0, 3000, 3))) == [1, 1000]
    assert info([0] * 100 + [1] * 70000 + [2] * 5) == [70000, 3]
    assert info([0, 0, 1, 0])[0] == -1                            # unsorted
    assert info([2, 2, 1])[0] == -1
    assert info([-1, 0, 0])[0] == -1                              # negative
    assert info([0] * 300 + [-5])[0] == -1
    idx = ShardIndex(_rows(8, 64, 1)[0])
    for bad in ([0, 0, 1, 0, 2, 2, 2, 2], [-1, 0, 0, 0, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match="non-decreasing"):
            idx.set_groups(np.array(bad, np.int32))
    with pytest.raises(ValueError, match="shape"):
        idx.set_groups(np.zeros(7, np.int32))
    with pytest.raises(ValueError, match="set_groups"):
        idx.search_grouped(_rows(8, 64, 1)[1], 2)
    idx.set_groups([0, 0, 0, 4, 4, 9, 9, 9])
    assert (idx.max_run_rows, idx.n_runs) == (3, 3)


def test_bad_arguments_are_refused_before_any_launch_with_the_field_and_its_value(hip):
    lib = hip.load()
    C_, Q_ = _rows(100, 64, 2)
    g = torch.zeros(100, dtype=torch.int32, device="cuda")
    need = lib.arx_topk_grouped_workspace_bytes(100, NQ, 64, 4, 2)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = torch.empty((NQ, 4, 2), dtype=torch.float32, device="cuda"); i = torch.empty((NQ, 4, 2), dtype=torch.int64, device="cuda")
    gr = torch.empty((NQ, 4), dtype=torch.int32, device="cuda")

    def call(**over):
        a = dict(corpus=C_.data_ptr(), n_rows=100, group_of=g.data_ptr(), max_run_rows=100, allow=None, n_allowed=-1, queries=Q_.data_ptr(),
                 nq=NQ, dim=64, P=4, m=2, s=s.data_ptr(), i=i.data_ptr(), g=gr.data_ptr(), base=0, norm=0.0, ws=ws.data_ptr(), ws_bytes=need,
                 path=0, cand_cap=0)
        a.update(over)
        rc = lib.arx_topk_search_grouped_tuned(*a.values(), None)
        return rc, lib.arx_last_error().decode()
    assert call()[0] == 0
    for over, text in ((dict(P=0), "n_groups=0"), (dict(P=33), "n_groups=33"), (dict(m=0), "chunks_per_group=0"), (dict(m=9), "chunks_per_group=9"),
                       (dict(max_run_rows=0), "max_run_rows=0"), (dict(dim=96), "dim=96"), (dict(group_of=None), "null pointer"),
                       (dict(g=None), "null pointer"), (dict(corpus=None), "null pointer"), (dict(path=3), "path=3"),
                       (dict(cand_cap=9000), "cand_cap=9000"), (dict(ws_bytes=need - 1), "workspace too small")):
        rc, msg = call(**over)
        assert rc == -1 and text in msg, (over, rc, msg)
    rc = lib.arx_group_runs_info(None, 5, s.data_ptr(), None)
    assert rc == -1 and "null pointer" in lib.arx_last_error().decode()


# ---- HipCollection.query and the CLI ---------------------------------------------------------------------------------------------------------
def _score_bits(lists):
    return [np.array(s, np.float32).view(np.int32).tolist() for s in lists]


def test_collection_query_group_by(hip):
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.where import compile_where, evaluate, pack_bitmap
    from oracle import search_oracle as SO
    from tests.test_gpu_filtered_search import _collection
    emb, meta = _collection(n=420)
    coll = HipCollection(emb, meta, group_key="paper_id")
    plain = HipCollection(emb, meta)
    q = SO.unit_rows_f16(6, 128, 9)
    qd = torch.from_numpy(q).cuda()
    # without group_by nothing changes, with or without group_key
    assert coll.query(query_embeddings=q, n_results=10, group_by=None) == plain.query(query_embeddings=q, n_results=10)
    assert coll.query(query_embeddings=q, n_results=10, group_by=False) == plain.query(query_embeddings=q, n_results=10)
    assert coll.index.max_run_rows == 7 and coll.group_keys == [f"0704.{p:04d}" for p in range(60)]

    def check(out, s, i, g, mask=None):
        s, i, g = s.cpu().numpy(), i.cpu().numpy(), g.cpu().numpy()
        for b in range(q.shape[0]):
            keep = i[b] >= 0
            assert out["indices"][b] == i[b][keep].tolist()
            assert _score_bits([out["scores"][b]]) == [s[b][keep].view(np.int32).tolist()]
            assert out["group_keys"][b] == [f"0704.{v:04d}" for v in g[b] if v >= 0]
            assert out["group_sizes"][b] == [int(k.sum()) for k, v in zip(keep, g[b]) if v >= 0]
            assert sum(out["group_sizes"][b]) == len(out["indices"][b]) == len(out["ids"][b]) == len(out["documents"][b])
            pos = 0
            for key, size in zip(out["group_keys"][b], out["group_sizes"][b]):      # paper by paper
                assert all(meta[r]["paper_id"] == key for r in out["indices"][b][pos:pos + size])
                pos += size
            assert len(set(out["group_keys"][b])) == len(out["group_keys"][b])
            if mask is not None:
                assert all(mask[r] for r in out["indices"][b])
    out = coll.query(query_embeddings=q, n_results=10, group_by=True, chunks_per_group=3)
    check(out, *coll.index.search_grouped(qd, 10, 3))
    assert all(len(k) == 10 and sz == [3] * 10 for k, sz in zip(out["group_keys"], out["group_sizes"]))
    where = {"section": {"$ne": "Methods"}}
    mask = evaluate(compile_where(where), meta)
    out = coll.query(query_embeddings=q, n_results=8, group_by=True, chunks_per_group=8, where=where)
    allow = torch.from_numpy(pack_bitmap(mask).view(np.int64)).cuda()
    check(out, *coll.index.search_grouped(qd, 8, 8, allow=allow), mask=mask)
    assert any(sz < 7 for sizes in out["group_sizes"] for sz in sizes)
    # a dedup collection: flagged rows never come back
    emb2 = emb.copy(); emb2[200] = emb2[3]; emb2[201] = emb2[3]
    dd = HipCollection(emb2, meta, group_key="paper_id", dedup_threshold=0.99)
    assert {e["index"] for e in dd.duplicates} == {200, 201}
    out = dd.query(query_embeddings=emb2[3:4].astype(np.float16), n_results=5, group_by=True, chunks_per_group=7)
    assert out["indices"][0][0] == 3 and not {200, 201} & set(out["indices"][0])
    with pytest.raises(ValueError, match="group_key"):
        plain.query(query_embeddings=q, group_by=True)
    with pytest.raises(ValueError, match="mmr_lambda"):
        coll.query(query_embeddings=q, group_by=True, mmr_lambda=0.5)


def test_cli_group_by_paper_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script with --queries --group-by-paper --top-k 4 --chunks-per-paper 2: the hits are, in order, what
    `ShardIndex.search_grouped` returns on the rows the script wrote, each with `paper_rank` and `paper_id`."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.grouping import runs_from_keys
    from arxiv_rag_amd.index import ShardIndex
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=40, chunks_per_file=6, seed=2, words=words)
    (tmp_path / "queries.txt").write_text("\n".join(" ".join(words[i:i + 6]) for i in range(0, 24, 6)) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    qs = (tmp_path / "queries.txt").read_text().split("\n")[:-1]
    GEN._model, GEN._model_name = None, None
    assert GEN.main([str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
                     "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"), "--top-k", "4", "--group-by-paper",
                     "--chunks-per-paper", "2"]) == 0
    res = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
    kept = GEN.load_chunks_parallel(tmp_path / "in", 0.9, 4)
    arr = np.load(tmp_path / "embeddings_saved" / "embeddings.npy")
    qd = torch.empty((len(qs), 384), dtype=torch.float16, device="cuda")
    GEN._model.encode(qs, normalize_embeddings=True, device_f16_out=qd, low_latency=True)
    group_of, keys = runs_from_keys([c["metadata"]["paper_id"] for c in kept])
    s, i, g = (t.cpu().numpy() for t in ShardIndex(torch.from_numpy(arr.astype(np.float16)).cuda()).set_groups(group_of).search_grouped(qd, 4, 2))
    for qi, r in enumerate(res):
        assert r["query"] == qs[qi]
        want = [(p + 1, keys[g[qi, p]], int(i[qi, p, c]), float(s[qi, p, c])) for p in range(4) for c in range(2) if i[qi, p, c] >= 0]
        assert [(h["paper_rank"], h["paper_id"], h["index"], h["score"]) for h in r["results"]] == want, qi
        assert [h["rank"] for h in r["results"]] == list(range(1, len(want) + 1))
        assert all(kept[h["index"]]["chunk_id"] == h["chunk_id"] and kept[h["index"]]["metadata"]["paper_id"] == h["paper_id"] for h in r["results"])
        assert len({h["paper_id"] for h in r["results"]}) == 4
    GEN._model.encoder.close()
    GEN._model, GEN._model_name = None, None
