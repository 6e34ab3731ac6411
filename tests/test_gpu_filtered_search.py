"""Filtered exact top-k search (`ShardIndex.search(allow=...)`, arx_topk_search_filtered; csrc/filter.hip) on the GPU: against float64 with
the certificate's own budget (tests/helpers.py: pass_b_budget), bit for bit against the existing search of the compacted rows, both
device paths and the overflow fallback against each other, and through `HipCollection.query(where=...)` and the CLI.

Figures printed by the tests: the counters of `filtered_stats` (queries answered by the exhaustive fallback, candidate groups)."""
import json
import zlib

import numpy as np
import pytest

from tests.helpers import check_topk_fp64
from tests.test_gpu_search_fp64 import _case_data, _gen, _unit

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BASE = 1 << 33


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _pack(mask, garbage=False):
    """bool [n] (device) -> int64 words (device), bit r & 63 of word r >> 6; `garbage`: the last word's bits beyond n are SET."""
    from arxiv_rag_amd.where import pack_bitmap
    m = mask.cpu().numpy()
    words = pack_bitmap(m)
    n = m.shape[0]
    if garbage and n % 64:
        words[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
    return torch.from_numpy(words.view(np.int64)).cuda()


def _mask(kind, n, k, g):
    m = torch.zeros(n, dtype=torch.bool, device="cuda")
    if kind in ("all", "garbage"):
        m[:] = True
    elif kind == "none":
        pass
    elif kind == "one":
        m[int(torch.randint(n, (1,), generator=g, device="cuda"))] = True
    elif kind == "k-1":
        m[torch.randperm(n, generator=g, device="cuda")[:k - 1]] = True
    elif kind == "rand50":
        m = torch.rand(n, generator=g, device="cuda") < 0.5
    elif kind == "rand1":
        m = torch.rand(n, generator=g, device="cuda") < 0.01
    elif kind == "block":                                       # contiguous, not aligned to 64 at either end
        a = min(n - 1, 37 + 64 * (n // 640))
        m[a:min(n, a + max(3, n // 8) + 11)] = True
    elif kind == "every64":
        m[5 % n::64] = True
    elif kind == "lastgroup":                                   # only rows of the last, partial group
        m[(n - 1) // 64 * 64:] = True
    else:
        raise AssertionError(kind)
    return m


def _check_fp64(C_, Q_, s, i, rows, k, what):
    """The filtered answer is the exact top-k of the sub-corpus C_[rows]: every id lies in `rows`; mapped to positions in `rows` the
    answer passes check_topk_fp64 over C_[rows]."""
    n = C_.shape[0]
    pos = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    pos[rows] = torch.arange(rows.shape[0], device="cuda")
    loc = i - BASE
    valid = i >= 0
    assert ((loc[valid] >= 0) & (loc[valid] < n)).all(), (what, "id outside the shard")
    sub = torch.where(valid, pos[loc.clamp(0, n - 1)], torch.full_like(i, -1))
    assert (sub[valid] >= 0).all(), (what, "a row outside the mask was returned")
    if rows.shape[0] == 0:
        assert (i == -1).all() and torch.isinf(s).all() and (s < 0).all(), (what, "padding")
        return
    check_topk_fp64(C_[rows].contiguous(), Q_, s, sub, k, idx_base=0, what=what)


def _bits_equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


CASES = [
    dict(id="n1-all", d=64, n=1, nq=1, k=1, rows="unit", mask="all"),
    dict(id="n63-rand50", d=64, n=63, nq=64, k=10, rows="unit", mask="rand50"),
    dict(id="n64-k-1", d=128, n=64, nq=257, k=32, rows="mixed", mask="k-1"),
    dict(id="n65-lastgroup", d=128, n=65, nq=1, k=10, rows="unit", mask="lastgroup"),
    dict(id="320-block", d=320, n=256 * 5 + 1, nq=64, k=10, rows="mixed", mask="block"),
    dict(id="320-every64", d=320, n=256 * 5 + 1, nq=257, k=32, rows="mixed", mask="every64"),
    dict(id="768-rand50", d=768, n=256 * 40 + 1, nq=64, k=10, rows="mixed", mask="rand50"),
    dict(id="768-one", d=768, n=256 * 40 + 1, nq=1, k=1, rows="unit", mask="one"),
    dict(id="768-none", d=768, n=256 * 8 + 1, nq=64, k=10, rows="unit", mask="none"),
    dict(id="768-ties-rand50", d=768, n=64 * 200 + 5, nq=64, k=10, rows="ties", mask="rand50"),
    dict(id="1024-ties-garbage", d=1024, n=64 * 200 + 5, nq=7, k=32, rows="ties", mask="garbage"),
    dict(id="1024-rand1-1030q", d=1024, n=256 * 8 + 1, nq=1030, k=10, rows="unit", mask="rand1"),
    dict(id="1024-all-257q", d=1024, n=256 * 4 + 1, nq=257, k=1, rows="mixed", mask="all"),
    dict(id="320-ties-lastgroup", d=320, n=64 * 130 + 37, nq=64, k=10, rows="ties", mask="lastgroup"),
    dict(id="64-200k-rand50-1030q", d=64, n=200001, nq=1030, k=10, rows="unit", mask="rand50"),
    dict(id="128-200k-rand1", d=128, n=200001, nq=64, k=32, rows="unit", mask="rand1"),
    dict(id="768-200k-block", d=768, n=200001, nq=64, k=10, rows="unit", mask="block"),
]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_filtered_search_fp64_paths_and_bitwise_equal_to_the_search_of_the_compacted_rows(hip, case):
    """Per case: the library's choice, the masked scan, the exhaustive path and the masked scan with a one-entry candidate list (every
    query with two candidate groups overflows into the exhaustive path) return the same bits; that answer passes the float64 check over
    the allowed rows and equals, scores and ids, what the existing search returns on an index of the allowed rows alone."""
    from arxiv_rag_amd.index import ShardIndex
    c = case
    C_, Q_ = _case_data(c)
    n, k = C_.shape[0], c["k"]
    g = _gen(zlib.crc32(("mask" + c["id"]).encode()))
    m = _mask(c["mask"], n, k, g)
    rows = torch.nonzero(m).flatten()
    allow = _pack(m, garbage=c["mask"] == "garbage")
    idx = ShardIndex(C_, idx_base=BASE)
    ref = idx.search(Q_, k, allow=allow, n_allowed=int(rows.shape[0]))
    _check_fp64(C_, Q_, ref[0], ref[1], rows, k, c["id"])
    stats = {}
    for name, kw in (("unknown-count", dict()), ("scan", dict(path=1)), ("exhaustive", dict(path=2)), ("cap1", dict(path=1, cand_cap=1))):
        got = idx.search(Q_, k, allow=allow, n_allowed=None if name == "unknown-count" else int(rows.shape[0]), **kw)
        stats[name] = idx.filtered_stats()
        assert _bits_equal(got, ref), (c["id"], name, "differs from the library's choice")
    print(f"{c['id']}: allowed {rows.shape[0]} of {n}; (overflowed queries, candidate groups) = {stats}")
    assert stats["exhaustive"] == (0, 0)
    # the existing search over the allowed rows alone (fp16 pass, the parent's behaviour), ids mapped back through `rows`
    if rows.shape[0]:
        s2, i2 = ShardIndex(C_[rows].contiguous()).search(Q_, k)
        i2 = torch.where(i2 >= 0, rows[i2.clamp_min(0)] + BASE, i2)
        assert _bits_equal((s2, i2), ref), (c["id"], "differs from the unfiltered search of the compacted rows")
    if c["mask"] in ("all", "garbage"):
        assert _bits_equal(idx.search(Q_, k), ref), (c["id"], "all-rows mask differs from the unfiltered search")


def test_unit_rows_never_take_the_fallback_and_a_one_entry_list_always_does(hip):
    """On unit rows and unit queries no query may overflow the default candidate list (so the fallback cannot hide a broken scan); with
    cand_cap = 1 every query does, the counter says so, and the bits are the same."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(77)
    C_ = _unit(64 * 900 + 3, 768, g).half().contiguous()
    Q_ = _unit(300, 768, g).half().contiguous()
    idx = ShardIndex(C_, idx_base=BASE)
    for frac in (1.0, 0.5, 0.1):
        m = torch.rand(C_.shape[0], generator=g, device="cuda") < frac
        allow = _pack(m)
        for k in (1, 10, 32):
            a = idx.search(Q_, k, allow=allow, path=1)
            over, groups = idx.filtered_stats()
            print(f"unit rows, {frac:.0%} allowed, k = {k}: overflowed {over}, candidate groups per query {groups / 300:.1f}")
            assert over == 0 and groups >= 300 * k
            b = idx.search(Q_, k, allow=allow, path=1, cand_cap=1)
            over1, _ = idx.filtered_stats()
            assert _bits_equal(a, b)
            if k > 1:
                assert over1 == 300                               # k groups at or above the k-th maximum: more than the list holds
            assert _bits_equal(idx.search(Q_, k, allow=allow, path=2), a)


def test_disallowed_rows_cannot_leak(hip):
    """Disallowed rows are copies of the queries (score 1, above every allowed row) and rows of norm 50: no id outside the mask comes
    back on either path, and the results equal, bit for bit, those with the disallowed rows zeroed."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(78)
    d, n, nq, k = 256, 64 * 70 + 9, 40, 10
    C_ = _unit(n, d, g).half()
    Q_ = _unit(nq, d, g).half().contiguous()
    m = torch.rand(n, generator=g, device="cuda") < 0.6
    m[64 * 3:64 * 5] = False                                     # two groups with no allowed row at all
    bad = torch.nonzero(~m).flatten()
    C_[bad[0::2]] = Q_[torch.arange(bad[0::2].shape[0], device="cuda") % nq]
    C_[bad[1::2]] = (C_[bad[1::2]].float() * 50.0).half()
    C_ = C_.contiguous()
    Z_ = C_.clone(); Z_[bad] = 0
    allow, rows = _pack(m), torch.nonzero(m).flatten()
    idx, idz = ShardIndex(C_, idx_base=BASE), ShardIndex(Z_, idx_base=BASE)
    assert idx.max_row_norm() > 49
    for kw in (dict(), dict(path=1), dict(path=2), dict(path=1, cand_cap=1)):
        s, i = idx.search(Q_, k, allow=allow, **kw)
        assert m[(i - BASE).flatten()].all(), kw
        _check_fp64(C_, Q_, s, i, rows, k, kw)
        assert _bits_equal(idz.search(Q_, k, allow=allow, **kw), (s, i)), kw
    # (the same shard unfiltered does return the copies: the mask is what keeps them out)
    s, i = idx.search(Q_, k)
    assert (~m[(i[:, 0] - BASE)]).all()


def test_the_fp64_check_fails_for_a_mask_shifted_by_one_row(hip):
    """The check used above can fail: the answer for mask M does not pass it against M shifted by one row."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(79)
    C_ = _unit(64 * 40 + 1, 128, g).half().contiguous()
    Q_ = _unit(64, 128, g).half().contiguous()
    m = torch.rand(C_.shape[0], generator=g, device="cuda") < 0.5
    s, i = ShardIndex(C_, idx_base=BASE).search(Q_, 10, allow=_pack(m))
    _check_fp64(C_, Q_, s, i, torch.nonzero(m).flatten(), 10, "mask")
    shifted = torch.roll(m, 1)
    with pytest.raises(AssertionError):
        _check_fp64(C_, Q_, s, i, torch.nonzero(shifted).flatten(), 10, "shifted mask")
    # and a block mask shifted by one: the ids mostly stay inside, the float64 completeness / membership test still objects
    mb = torch.zeros_like(m); mb[100:140] = True
    s, i = ShardIndex(C_, idx_base=BASE).search(Q_, 32, allow=_pack(mb))
    _check_fp64(C_, Q_, s, i, torch.nonzero(mb).flatten(), 32, "block")
    with pytest.raises(AssertionError):
        _check_fp64(C_, Q_, s, i, torch.nonzero(torch.roll(mb, 1)).flatten(), 32, "shifted block")


def test_a_query_gets_the_same_bits_alone_and_inside_a_257_query_batch(hip):
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(80)
    C_ = _unit(64 * 300 + 17, 320, g).half().contiguous()
    Q_ = _unit(257, 320, g).half().contiguous()
    m = torch.rand(C_.shape[0], generator=g, device="cuda") < 0.3
    allow = _pack(m)
    idx = ShardIndex(C_, idx_base=BASE)
    for kw in (dict(), dict(path=1), dict(path=2)):
        s, i = idx.search(Q_, 10, allow=allow, **kw)
        for qi in (0, 63, 64, 200, 256):
            s1, i1 = idx.search(Q_[qi:qi + 1].contiguous(), 10, allow=allow, **kw)
            assert _bits_equal((s1, i1), (s[qi:qi + 1], i[qi:qi + 1])), (kw, qi)


def test_search_allow_argument_checks(hip):
    from arxiv_rag_amd.index import ShardIndex
    C_ = _unit(200, 128, _gen(1)).half().contiguous()
    q = _unit(2, 128, _gen(2)).half().contiguous()
    idx = ShardIndex(C_)
    allow = _pack(torch.ones(200, dtype=torch.bool, device="cuda"))
    with pytest.raises(TypeError):
        idx.search(q, 5, allow=allow, tau_mult=2.0)
    with pytest.raises(AssertionError):
        idx.search(q, 5, allow=allow[:-1].contiguous())
    with pytest.raises(hip.ArxError):
        idx.search(q, 5, allow=allow, path=3)
    s, i = idx.search(q, 5, allow=allow, n_allowed=200)
    assert _bits_equal(idx.search(q, 5), (s, i))


# ---- HipCollection.query(where=...) and the CLI ----------------------------------------------------------------------------------------
def _collection(n=3000, d=128, seed=3):
    from oracle import search_oracle as SO
    rs = np.random.RandomState(seed)
    emb = SO.unit_rows_f16(n, d, seed).astype(np.float32)
    meta = [{"chunk_id": f"0704.{r // 7:04d}_chunk_{r % 7}", "paper_id": f"0704.{r // 7:04d}", "chunk_index": r % 7,
             "section": ["abstract", "Introduction", "Methods", "Results"][rs.randint(4)], "quality_score": float(np.round(rs.uniform(0.8, 1.0), 2)),
             "text": " ".join(rs.choice(["alpha", "beta", "gamma", "delta"], size=rs.randint(2, 9)))} for r in range(n)]
    return emb, meta


def test_collection_query_where(hip):
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.where import compile_where, evaluate
    from oracle import search_oracle as SO
    emb, meta = _collection()
    coll = HipCollection(emb, meta)
    q = SO.unit_rows_f16(12, 128, 9)
    for where, n_results in (({"section": "abstract"}, 10), ({"quality_score": {"$gte": 0.95}}, 10),
                             ({"paper_id": {"$in": ["0704.0003", "0704.0100", "0704.0399"]}}, 10),
                             ({"$and": [{"section": {"$ne": "Methods"}}, {"chunk_index": {"$lt": 2}}]}, 32),
                             ({"paper_id": "0704.0007"}, 10), ({"paper_id": "none such"}, 5)):
        out = coll.query(query_embeddings=q, n_results=n_results, where=where)
        rows = np.nonzero(evaluate(compile_where(where), meta))[0]
        want_n = min(n_results, rows.shape[0])
        sub = emb[rows].astype(np.float16)
        if rows.shape[0]:
            rs_, ri_ = SO.topk_search(sub, q, want_n)
        for qi in range(q.shape[0]):
            assert len(out["indices"][qi]) == want_n, (where, "list length")          # short lists when few rows satisfy the filter
            for md, r in zip(out["metadatas"][qi], out["indices"][qi]):
                assert r in set(rows.tolist()) and md["paper_id"] == meta[r]["paper_id"] and md["section"] == meta[r]["section"], where
            if rows.shape[0]:
                assert out["indices"][qi] == rows[ri_[qi]].tolist(), (where, qi)
                assert np.abs(np.array(out["scores"][qi]) - rs_[qi]).max() < 1e-5
    with pytest.raises(ValueError, match="hybrid_alpha"):
        coll.query(query_embeddings=q, query_texts=["a"] * 12, where={"section": "abstract"}, hybrid_alpha=0.5)
    with pytest.raises(ValueError, match="\\$like"):
        coll.query(query_embeddings=q, where={"section": {"$like": "a"}})

    class LengthReranker:                                        # anything with HipCrossEncoder's `predict`
        def predict(self, pairs, **kw):
            return np.array([len(doc) for _, doc in pairs], np.float32)
    out = coll.query(query_embeddings=q, query_texts=["alpha beta"] * 12, n_results=5, n_candidates=20, reranker=LengthReranker(),
                     where={"section": "Results"})
    cand = coll.query(query_embeddings=q, n_results=20, where={"section": "Results"})
    for qi in range(12):
        assert all(meta[r]["section"] == "Results" for r in out["indices"][qi]) and len(out["indices"][qi]) == 5
        assert set(out["indices"][qi]) <= set(cand["indices"][qi])                   # the cross-encoder saw the filtered candidates
        assert out["rerank_scores"][qi] == sorted(out["rerank_scores"][qi], reverse=True)


def test_cli_where_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script with --queries and --where: every hit satisfies the filter and the lists are the top-10 of the satisfying
    rows (the fp16 rows the script wrote, the queries as it encoded them)."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from oracle import search_oracle as SO
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=60, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text("\n".join(" ".join(words[i:i + 6]) for i in range(0, 48, 6)) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    GEN._model, GEN._model_name = None, None
    where = {"$and": [{"section": "Methods"}, {"quality_score": {"$gte": 0.93}}]}
    rc = GEN.main([str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
                   "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"), "--where", json.dumps(where)])
    assert rc == 0
    kept = GEN.load_chunks_parallel(tmp_path / "in", 0.9, 4)
    ok = np.array([c["metadata"]["section"] == "Methods" and c["metadata"]["quality_score"] >= 0.93 for c in kept])
    assert 10 < ok.sum() < len(kept)
    res = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
    qs = (tmp_path / "queries.txt").read_text().split("\n")[:-1]
    assert [r["query"] for r in res] == qs
    arr = np.load(tmp_path / "embeddings_saved" / "embeddings.npy")
    qd = torch.empty((len(qs), 384), dtype=torch.float16, device="cuda")
    GEN._model.encode(qs, normalize_embeddings=True, device_f16_out=qd, low_latency=True)
    rows = np.nonzero(ok)[0]
    rs2, ri2 = SO.topk_search(arr[rows].astype(np.float16), qd.cpu().numpy(), 11)
    for qi, r in enumerate(res):
        got = [h["index"] for h in r["results"]]
        assert len(got) == 10 and all(ok[j] for j in got), "a hit outside the filter"
        assert [h["chunk_id"] for h in r["results"]] == [kept[j]["chunk_id"] for j in got]
        assert all(set(h) == {"rank", "score", "index", "chunk_id"} for h in r["results"])       # search_results.json keeps its shape
        if set(got) != set(rows[ri2[qi, :10]].tolist()):
            assert rs2[qi, 9] - rs2[qi, 10] < 1e-6
    GEN._model, GEN._model_name = None, None
