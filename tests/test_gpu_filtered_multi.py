"""Filtered exact top-k with a different filter per query in one call (`ShardIndex.search_filtered_many`, arx_topk_search_filtered_multi;
csrc/filter_multi.hip) on the GPU.  The reference of every query is `search(allow=...)` (arx_topk_search_filtered) called with that query
ALONE and its own bitmap: the multi call must return its bits.  Beside that: float64 (tests/helpers.py check_topk_fp64, the helper's own
tolerance) over the rows each query's bitmap allows, no id outside a query's own filter, every path (1 masked scan, 2 exhaustive, 0 the
library's choice), the overflow fallback, permutations of the batch and of the filter numbering, out-of-range filter indices, a shard
beyond the tail's register boundary, the argument checks, `HipCollection.query` with lists and the CLI's --where-file."""
import ctypes as C
import json
import zlib

import numpy as np
import pytest

from tests.test_gpu_filtered_search import BASE, _bits_equal, _check_fp64, _collection
from tests.test_gpu_search_fp64 import _case_data, _gen, _unit

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ("all", "none", "one", "block", "rand1", "rand50", "complement")


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _masks(F, n, g, first=0):
    """bool [F, n]: the seven kinds in turn from `first` on (all rows, no rows, one single row, contiguous 12.5 % not aligned to 64, random
    1 %, random 50 %, the exact complement of the filter before it: with F = 2 a random 50 % filter and its complement)."""
    out = []
    for f in range(F):
        kind = KINDS[(first + f) % len(KINDS)] if F != 2 else ("rand50", "complement")[f]
        m = torch.zeros(n, dtype=torch.bool, device="cuda")
        if kind == "all":
            m[:] = True
        elif kind == "one":
            m[int(torch.randint(n, (1,), generator=g, device="cuda"))] = True
        elif kind == "block":
            a = int(torch.randint(n - n // 8, (1,), generator=g, device="cuda"))
            m[a:a + n // 8] = True
        elif kind == "rand1":
            m = torch.rand(n, generator=g, device="cuda") < 0.01
        elif kind == "rand50":
            m = torch.rand(n, generator=g, device="cuda") < 0.5
        elif kind == "complement":
            m = ~out[-1] if out else torch.rand(n, generator=g, device="cuda") >= 0.5
        out.append(m)
    return torch.stack(out)


def _pack_many(masks, garbage=True):
    """bool [F, n] (device) -> int64 [F, ceil(n / 64)] (device); `garbage`: every bitmap's bits beyond n are SET."""
    from arxiv_rag_amd.where import pack_bitmap
    n = masks.shape[1]
    rows = []
    for m in masks.cpu().numpy():
        words = pack_bitmap(m)
        if garbage and n % 64:
            words[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
        rows.append(words.view(np.int64))
    return torch.from_numpy(np.stack(rows)).cuda()


def _interleaved(nq, F):
    """filter_of: every filter in turn with a stride coprime to 2, 7 and 64, so that no query tile is sorted or uniform."""
    return ((torch.arange(nq, device="cuda") * 5 + 3) % F).to(torch.int32)


def _alone(idx, Q_, allows, fo, k, **kw):
    """The reference: every query by itself through the single-filter search with its own bitmap."""
    s = torch.empty((Q_.shape[0], k), dtype=torch.float32, device="cuda")
    i = torch.empty((Q_.shape[0], k), dtype=torch.int64, device="cuda")
    for q, f in enumerate(fo.tolist()):
        idx.search(Q_[q:q + 1], k, allow=allows[f], out=(s[q:q + 1], i[q:q + 1]), **kw)
    return s, i


def _no_leak(i, masks, fo, what):
    """No returned id lies outside the query's own filter."""
    n = masks.shape[1]
    loc = i - BASE
    valid = i >= 0
    assert ((loc[valid] >= 0) & (loc[valid] < n)).all(), (what, "id outside the shard")
    own = masks[fo.long()].gather(1, loc.clamp(0, n - 1))
    assert own[valid].all(), (what, "a row outside the query's own filter was returned")


_DATA = {}


def _data(n, d):
    """One corpus (every row family of the fp64 search tests) and 257 queries per (n, d), shared by the cases and left unchanged."""
    if (n, d) not in _DATA:
        _DATA[(n, d)] = _case_data(dict(id=f"multi-{n}-{d}", d=d, n=n, nq=257, rows="mixed"))
    return _DATA[(n, d)]


@pytest.mark.parametrize("F", [1, 2, 7, 64])
@pytest.mark.parametrize("nq", [1, 65, 130, 257])
@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("n", [1037, 4133])
def test_every_query_gets_the_bits_of_the_single_filter_search_alone(hip, n, d, k, nq, F):
    from arxiv_rag_amd.index import ShardIndex
    C_, Qall = _data(n, d)
    Q_ = Qall[:nq].contiguous()
    what = f"n{n}-d{d}-k{k}-q{nq}-F{F}"
    seed = zlib.crc32(what.encode())
    masks = _masks(F, n, _gen(seed), first=seed % len(KINDS))
    allows, fo = _pack_many(masks), _interleaved(nq, F)
    counts = masks.sum(1).tolist()
    idx = ShardIndex(C_, idx_base=BASE)
    ref = _alone(idx, Q_, allows, fo, k)
    for f in sorted(set(fo.tolist())):
        qs = torch.nonzero(fo == f).flatten()
        _check_fp64(C_, Q_[qs].contiguous(), ref[0][qs].contiguous(), ref[1][qs].contiguous(), torch.nonzero(masks[f]).flatten(), k, (what, f))
    for path in (1, 2, 0):
        got = idx.search_filtered_many(Q_, allows, fo, k, n_allowed=counts if path == 0 else None, path=path)
        assert _bits_equal(got, ref), (what, path, "differs from the single-filter search of each query alone")
        _no_leak(got[1], masks, fo, (what, path))


def test_tiles_empty_for_one_filter_and_not_for_the_other(hip):
    """Two filters over disjoint row ranges (rows < 512, rows >= 3 072 of 4 133) alternate inside one query tile: every 256-row tile is
    empty for one of them and not for the other.  Then every query of the tile on the low range: whatever the rows from 512 on hold (here
    copies of the queries, score 1), the answers are those over a shard where they are zero."""
    from arxiv_rag_amd.index import ShardIndex
    n, d, k = 4133, 64, 10
    C_, Qall = _data(n, d)
    masks = torch.zeros((2, n), dtype=torch.bool, device="cuda")
    masks[0, :512] = True
    masks[1, 3072:] = True
    allows = _pack_many(masks)
    idx = ShardIndex(C_, idx_base=BASE)
    for nq in (64, 130, 257):
        Q_ = Qall[:nq].contiguous()
        fo = (torch.arange(nq, device="cuda") % 2).to(torch.int32)
        ref = _alone(idx, Q_, allows, fo, k)
        for path in (1, 2, 0):
            got = idx.search_filtered_many(Q_, allows, fo, k, path=path)
            assert _bits_equal(got, ref), (nq, path)
            _no_leak(got[1], masks, fo, (nq, path))
        low = torch.zeros(nq, dtype=torch.int32, device="cuda")
        P_ = C_.clone(); P_[512:] = Q_[torch.arange(n - 512, device="cuda") % nq]
        Z_ = C_.clone(); Z_[512:] = 0
        a = ShardIndex(P_.contiguous(), idx_base=BASE).search_filtered_many(Q_, allows, low, k, path=1)
        b = ShardIndex(Z_.contiguous(), idx_base=BASE).search_filtered_many(Q_, allows, low, k, path=1)
        assert _bits_equal(a, b), (nq, "rows of tiles no query of the tile may see changed the answer")
        _no_leak(a[1], masks, low, (nq, "low"))


def test_a_one_entry_candidate_list_sends_every_query_to_the_exhaustive_path(hip):
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(91)
    n, d, nq, k = 4133, 768, 130, 10
    C_ = _unit(n, d, g).half().contiguous()
    Q_ = _unit(nq, d, g).half().contiguous()
    masks = _masks(2, n, g)
    allows, fo = _pack_many(masks), _interleaved(nq, 2)
    idx = ShardIndex(C_, idx_base=BASE)
    ref = _alone(idx, Q_, allows, fo, k)
    a = idx.search_filtered_many(Q_, allows, fo, k, path=1)
    over, groups = idx.filtered_many_stats()
    print(f"default candidate list: overflowed {over}, candidate groups per query {groups / nq:.1f}")
    assert over == 0 and groups >= nq * k and _bits_equal(a, ref)
    b = idx.search_filtered_many(Q_, allows, fo, k, path=1, cand_cap=1)
    assert idx.filtered_many_stats()[0] == nq                     # k groups at or above the k-th maximum: more than the list holds
    assert _bits_equal(b, ref)
    idx.search_filtered_many(Q_, allows, fo, k, path=2)
    assert idx.filtered_many_stats() == (0, 0)


def test_permuting_the_batch_or_renumbering_the_filters(hip):
    from arxiv_rag_amd.index import ShardIndex
    n, d, nq, k, F = 4133, 64, 257, 10, 7
    C_, Q_ = _data(n, d)
    g = _gen(92)
    masks = _masks(F, n, g)
    allows, fo = _pack_many(masks), _interleaved(nq, F)
    idx = ShardIndex(C_, idx_base=BASE)
    for path in (1, 2):
        s, i = idx.search_filtered_many(Q_, allows, fo, k, path=path)
        perm = torch.randperm(nq, generator=g, device="cuda")
        got = idx.search_filtered_many(Q_[perm].contiguous(), allows, fo[perm].contiguous(), k, path=path)
        assert _bits_equal(got, (s[perm], i[perm])), (path, "shuffling the queries with filter_of")
        order = torch.randperm(F, generator=g, device="cuda")          # new filter j = old filter order[j]
        new_of = torch.empty(F, dtype=torch.int32, device="cuda")
        new_of[order] = torch.arange(F, dtype=torch.int32, device="cuda")
        got = idx.search_filtered_many(Q_, allows[order].contiguous(), new_of[fo.long()].contiguous(), k, path=path)
        assert _bits_equal(got, (s, i)), (path, "renumbering the filters")


def test_a_filter_index_out_of_range_sees_no_row(hip):
    from arxiv_rag_amd.index import ShardIndex
    n, d, k, F = 4133, 64, 10, 7
    C_, Qall = _data(n, d)
    masks = _masks(F, n, _gen(93))
    allows = _pack_many(masks)
    idx = ShardIndex(C_, idx_base=BASE)
    for nq in (65, 257):
        Q_ = Qall[:nq].contiguous()
        fo = _interleaved(nq, F)
        bad = fo.clone()
        bad[1::4] = -1
        bad[2::4] = F
        bad[3::64] = 1 << 30
        out = (bad < 0) | (bad >= F)
        for path in (1, 2, 0):
            s, i = idx.search_filtered_many(Q_, allows, fo, k, path=path)
            sb, ib = idx.search_filtered_many(Q_, allows, bad, k, path=path)
            assert (ib[out] == -1).all() and torch.isinf(sb[out]).all() and (sb[out] < 0).all(), (nq, path)
            assert _bits_equal((sb[~out], ib[~out]), (s[~out], i[~out])), (nq, path, "the other queries changed")
        # a tile in which NO query names a filter
        sb, ib = idx.search_filtered_many(Q_, allows, torch.full((nq,), -1, dtype=torch.int32, device="cuda"), k)
        assert (ib == -1).all() and torch.isinf(sb).all()


def test_a_shard_beyond_the_tails_register_boundary(hip):
    """n_rows = 2^20 + 300: more than 16 x 1 024 groups, so the tail reads its last group maxima from memory."""
    from arxiv_rag_amd.index import ShardIndex
    n, d, k = (1 << 20) + 300, 64, 10
    g = _gen(94)
    C_ = _unit(n, d, g).half().contiguous()
    Q_ = _unit(5, d, g).half().contiguous()
    masks = torch.stack([torch.rand(n, generator=g, device="cuda") < 0.5, torch.zeros(n, dtype=torch.bool, device="cuda"),
                         torch.rand(n, generator=g, device="cuda") < 0.01])
    masks[1, (1 << 20) - 100:] = True                                    # only rows around the boundary and in the last, partial group
    allows = _pack_many(masks)
    fo = torch.tensor([2, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
    idx = ShardIndex(C_, idx_base=BASE)
    ref = _alone(idx, Q_, allows, fo, k)
    for path in (1, 2, 0):
        got = idx.search_filtered_many(Q_, allows, fo, k, path=path)
        assert _bits_equal(got, ref), path
        _no_leak(got[1], masks, fo, path)


def test_argument_checks(hip):
    from arxiv_rag_amd.index import ShardIndex
    lib = hip.load()
    n, d, k = 1037, 64, 5
    C_, Qall = _data(n, d)
    Q_ = Qall[:4].contiguous()
    allows = _pack_many(_masks(2, n, _gen(95)))
    fo = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device="cuda")
    idx = ShardIndex(C_)
    with pytest.raises(ValueError):
        idx.search_filtered_many(Q_, allows[:0], fo, k)
    with pytest.raises(ValueError):
        idx.search_filtered_many(Q_, allows[:1].expand(65, -1).contiguous(), fo, k)
    with pytest.raises(ValueError):
        idx.search_filtered_many(Q_, allows, fo, k, n_allowed=[1, 2, 3])
    with pytest.raises(AssertionError):
        idx.search_filtered_many(Q_, allows[:, :-1].contiguous(), fo, k)
    with pytest.raises(AssertionError):
        idx.search_filtered_many(Q_, allows, fo.long(), k)
    with pytest.raises(TypeError):
        idx.search_filtered_many(Q_, allows, fo, k, tau_mult=2.0)
    with pytest.raises(hip.ArxError):
        idx.search_filtered_many(Q_, allows, fo, k, path=3)
    with pytest.raises(ValueError):
        idx.search_distributed(Q_, k, allows=allows)
    # the C ABI: ARX_ERR_ARG (-1), and the outputs keep what they held
    assert lib.arx_topk_filtered_multi_workspace_bytes(n, 4, 0, d, k) == -1
    assert lib.arx_topk_filtered_multi_workspace_bytes(n, 4, 65, d, k) == -1
    need = lib.arx_topk_filtered_multi_workspace_bytes(n, 4, 2, d, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = torch.full((4, k), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((4, k), 7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n_filters=2, fo_ptr=fo.data_ptr(), allow_ptr=allows.data_ptr(), ws_bytes=need):
        return lib.arx_topk_search_filtered_multi(C_.data_ptr(), n, allow_ptr, n_filters, None, fo_ptr, Q_.data_ptr(), 4, d, k, s.data_ptr(),
                                                  i.data_ptr(), 0, 0.0, ws.data_ptr(), ws_bytes, st)
    for kw in (dict(n_filters=0), dict(n_filters=65), dict(fo_ptr=None), dict(allow_ptr=None), dict(ws_bytes=need - 1)):
        assert call(**kw) == -1, kw
        torch.cuda.synchronize()
        assert (s == 7.0).all() and (i == 7).all(), (kw, "something was launched")
    bad = (C.c_int64 * 2)(n + 1, 0)
    assert lib.arx_topk_search_filtered_multi(C_.data_ptr(), n, allows.data_ptr(), 2, bad, fo.data_ptr(), Q_.data_ptr(), 4, d, k, s.data_ptr(),
                                              i.data_ptr(), 0, 0.0, ws.data_ptr(), need, st) == -1
    assert call() == 0
    assert _bits_equal((s, i), idx.search_filtered_many(Q_, allows, fo, k))


# ---- HipCollection.query with one filter per query, and the CLI ------------------------------------------------------------------------
WHERES = [{"section": "abstract"}, {"quality_score": {"$gte": 0.95}, "section": "Results"}, {"paper_id": {"$in": ["0704.0003", "0704.0100", "0704.0399"]}},
          {"$and": [{"section": {"$ne": "Methods"}}, {"chunk_index": {"$lt": 2}}]}]


class _LengthReranker:                                           # anything with HipCrossEncoder's `predict`
    def predict(self, pairs, **kw):
        return np.array([len(doc) for _, doc in pairs], np.float32)


def _same_rows(out, qi, single, keys):
    for key in keys:
        assert out[key][qi] == single[key][0], (qi, key)


def test_collection_query_with_one_filter_per_query(hip):
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    emb, meta = _collection()
    coll = HipCollection(emb, meta)
    q = SO.unit_rows_f16(12, 128, 9)
    wheres = [WHERES[0], None, WHERES[1], dict(reversed(list(WHERES[1].items()))), WHERES[2], WHERES[3], None, WHERES[0], WHERES[3],
              WHERES[2], WHERES[1], {"section": "abstract"}]
    texts = ["alpha beta"] * 12
    keys = ("indices", "ids", "scores", "distances", "documents", "metadatas")
    for kw, extra in ((dict(n_results=10), ()), (dict(n_results=5, n_candidates=20, reranker=_LengthReranker(), query_texts=texts), ("rerank_scores",)),
                      (dict(n_results=5, n_candidates=20, mmr_lambda=0.6), ("mmr_scores",))):
        out = coll.query(query_embeddings=q, where=wheres, **kw)
        assert set(out) == set(keys + extra)
        for qi in range(12):
            single = coll.query(query_embeddings=q[qi:qi + 1], where=wheres[qi],
                                **{**kw, **({"query_texts": texts[:1]} if "query_texts" in kw else {})})
            _same_rows(out, qi, single, keys + extra)
    assert out["indices"][1] != out["indices"][0]                 # (the filters do differ)
    with pytest.raises(ValueError, match="12 queries"):
        coll.query(query_embeddings=q, where=wheres[:-1])
    with pytest.raises(ValueError, match="hybrid_alpha"):
        coll.query(query_embeddings=q, query_texts=texts, where=wheres, hybrid_alpha=0.5)
    with pytest.raises(ValueError, match="documents=True"):
        coll.query(query_embeddings=q, where_document=[{"$contains": "alpha"}] * 12)


def test_collection_query_with_more_than_64_distinct_filters(hip):
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    emb, meta = _collection()
    coll = HipCollection(emb, meta, documents=True)
    q = SO.unit_rows_f16(75, 128, 10)
    wheres = [{"paper_id": {"$in": [f"0704.{p:04d}" for p in range(j, j + 40)]}} for j in range(70)] + [None, WHERES[0]] + \
             [{"paper_id": {"$in": [f"0704.{p:04d}" for p in range(j, j + 40)]}} for j in (3, 69, 0)]
    docs = [{"$contains": "alpha"} if j % 3 == 0 else None for j in range(75)]
    out = coll.query(query_embeddings=q, where=wheres, where_document=docs, n_results=10)
    for qi in range(75):
        single = coll.query(query_embeddings=q[qi:qi + 1], where=wheres[qi], where_document=docs[qi], n_results=10)
        _same_rows(out, qi, single, ("indices", "scores"))
        if qi % 3 == 0:
            assert all("alpha" in meta[r]["text"] for r in out["indices"][qi])


def test_cli_where_file_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script with --where-file: the results of every query are those of a run with --where and that query's filter."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=30, chunks_per_file=10, seed=2, words=words)
    qs = [" ".join(words[i:i + 6]) for i in range(0, 24, 6)]
    (tmp_path / "queries.txt").write_text("\n".join(qs) + "\n")
    filters = [{"section": "Methods"}, None, {"quality_score": {"$gte": 0.93}}, {"section": "Methods"}]
    (tmp_path / "filters.jsonl").write_text("\n".join(json.dumps(f) for f in filters) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
              "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    results = tmp_path / "embeddings_saved" / "search_results.json"
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--where-file", str(tmp_path / "filters.jsonl")]) == 0
    many = json.loads(results.read_text())
    assert [r["query"] for r in many] == qs
    everything = {"quality_score": {"$gte": 0.0}}                 # (null = no filter: the same rows as a filter every chunk satisfies)
    for f in (filters[0], filters[1], filters[2]):
        GEN._model, GEN._model_name = None, None
        assert GEN.main(common + ["--where", json.dumps(everything if f is None else f)]) == 0
        single = json.loads(results.read_text())
        for qi, fq in enumerate(filters):
            if fq == f:
                assert many[qi] == single[qi], (qi, f)
    assert many[0]["results"] != many[1]["results"]
    (tmp_path / "filters.jsonl").write_text("\n".join(json.dumps(f) for f in filters[:3]) + "\n")
    assert GEN.main(common + ["--where-file", str(tmp_path / "filters.jsonl")]) == 2
    GEN._model, GEN._model_name = None, None
