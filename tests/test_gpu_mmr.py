"""MMR retrieval on the device (-m gpu): `arx_gather_rows` and `arx_mmr_select` through the C ABI against the float64 definition
(`mmr.mmr_reference_f64`), then `HipCollection.query(mmr_lambda=...)`, the CLI flags and the path under a one-rank RCCL group."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd.mmr import cosines_f64, mmr_reference_f64
from tests.mmr_cases import certify, cluster_case, eps_of, ladder_case, step_gaps_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _f32(lam):
    """The lambda the kernel receives: the C ABI takes a float, so the float64 reference is evaluated at that value."""
    return float(np.float32(lam))


def _select(hip, q, cand, ids, m, lam):
    """arx_mmr_select through the C ABI on numpy inputs (q fp16 [Q, D], cand fp16 [Q, n, D], ids int64 [Q, n]) -> (order, mmr) numpy; the
    output buffers are poisoned before the call."""
    qd, cd, idd = torch.from_numpy(q.copy()).cuda(), torch.from_numpy(cand.copy()).cuda(), torch.from_numpy(ids.copy()).cuda()
    nq, n, dim = cand.shape
    order = torch.full((nq, m), -77, dtype=torch.int32, device="cuda")
    val = torch.full((nq, m), float("nan"), dtype=torch.float32, device="cuda")
    rc = hip.load().arx_mmr_select(qd.data_ptr(), cd.data_ptr(), idd.data_ptr(), nq, n, dim, m, lam, order.data_ptr(), val.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    hip.check(rc, "arx_mmr_select")
    torch.cuda.synchronize()
    return order.cpu().numpy(), val.cpu().numpy()


def _unit(rs, shape):
    x = rs.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 768, 8])
def test_gather_rows_equals_indexing_and_overwrites_every_byte(hip, dim):
    rs = np.random.RandomState(dim)
    n_rows, base = 1000, 1 << 33
    shard = rs.standard_normal((n_rows, dim)).astype(np.float16)
    shard[shard == 0] = np.float16(1.0)                         # no zero element: an all-zero output row can only be a written one
    ids = base + rs.randint(0, n_rows, size=(7, 32)).astype(np.int64)
    ids[0, :5] = -1
    ids[1, 3] = base - 1                                        # just below the shard
    ids[1, 4] = base + n_rows                                   # just beyond it
    ids[2, 0] = 5                                               # a row of a rank far below
    ids[2, 1] = (1 << 40) + 3
    ids[3, :2] = [base, base + n_rows - 1]                      # the shard's first and last row
    sd, idd = torch.from_numpy(shard).cuda(), torch.from_numpy(ids).cuda()
    inside = (ids >= base) & (ids < base + n_rows)
    want = np.where(inside[..., None], shard[np.clip(ids - base, 0, n_rows - 1)], np.float16(0))
    assert (~inside).sum() == 9
    for poison in (0xFF, 0x3C):
        out = torch.full((7, 32, dim * 2), poison, dtype=torch.uint8, device="cuda")
        rc = hip.load().arx_gather_rows(sd.data_ptr(), n_rows, dim, base, idd.data_ptr(), ids.size, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        hip.check(rc, "arx_gather_rows")
        got = out.cpu().numpy().view(np.float16).reshape(7, 32, dim)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        assert not got[~inside].view(np.uint16).any()
    # the Python wrapper, and an empty shard (every slot zero)
    from arxiv_rag_amd.index import ShardIndex
    from arxiv_rag_amd.mmr import gather_rows
    if dim % 64 == 0:
        got = gather_rows(ShardIndex(sd, idx_base=base), idd).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    out = torch.full((4, dim), 7.0, dtype=torch.float16, device="cuda")
    hip.check(hip.load().arx_gather_rows(None, 0, dim, 0, idd.data_ptr(), 4, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_gather_rows")
    assert not out.cpu().numpy().any()


# ---- the float64 certificate ----------------------------------------------------------------------------------------------------------------
KINDS = ("unit", "mixed", "zeros", "duplicates", "trailing")
N_QUERIES = 4


def _case(kind, dim, n, seed):
    """N_QUERIES queries of one row kind -> (q fp16 [Q, D], cand fp16 [Q, n, D], ids int64 [Q, n])."""
    rs = np.random.RandomState(seed)
    q = _unit(rs, (N_QUERIES, dim))
    cand = _unit(rs, (N_QUERIES, n, dim))
    cand += 0.5 * q[:, None, :] * rs.uniform(0.0, 1.0, size=(N_QUERIES, n, 1))           # relevances spread over (0, 0.5)
    cand /= np.linalg.norm(cand, axis=-1, keepdims=True)
    ids = rs.randint(0, 1 << 40, size=(N_QUERIES, n)).astype(np.int64)
    if kind == "mixed":                                         # norms from 1/8 to 32, the queries' too
        cand *= 2.0 ** rs.randint(-3, 6, size=(N_QUERIES, n, 1))
        q *= 2.0 ** rs.randint(-3, 6, size=(N_QUERIES, 1))
    elif kind == "zeros":                                       # all-zero candidate rows under valid ids; one all-zero query
        cand[rs.uniform(size=(N_QUERIES, n)) < 0.4] = 0.0
        cand[0, 0] = 0.0
        q[N_QUERIES - 1] = 0.0
    elif kind == "duplicates":                                  # every row one of at most 3 distinct rows, bit for bit
        src = rs.randint(0, min(3, n), size=(N_QUERIES, n))
        cand = np.take_along_axis(cand, src[..., None], axis=1)
    q, cand = q.astype(np.float16), cand.astype(np.float16)
    if kind == "trailing":                                      # the list ends in -1 slots (their rows hold anything); one query has no valid slot
        for b in range(N_QUERIES):
            ids[b, n - rs.randint(1, n + 1):] = -1
        ids[1, :] = -1
        ids[0, n - 1] = -1
    return q, cand, ids


@pytest.mark.parametrize("dim", [64, 320, 768, 1024, 8192])
def test_certificate_against_float64(hip, dim):
    """Every pick of the kernel is certified in float64 on the fp16 inputs (tests/mmr_cases.certify): given the kernel's own earlier
    picks, the pick is a valid unpicked slot with obj_t(pick) >= max_i obj_t(i) - 2 eps, and the returned value is within eps of obj_t.

    eps is derived, not measured.  A product of two fp16 values is exact in f32.  An f32 sum of D such products, in any order, differs
    from the exact sum by at most gamma_D |a| |b| with gamma_D ~ D 2^-24.  A cosine dot / sqrt(nn' nn'') takes three such dots: the
    numerator's error is D 2^-24 in cosine units, each of the two squared norms has relative error D 2^-24 and enters under a square
    root (half of it each), together 2 D 2^-24; the multiply, the sqrt and the divide add one rounding of 2^-24 each, and the budget
    leaves 16 2^-24 for those and for the objective: a convex combination of two cosines (weights lambda, 1 - lambda: no larger an error
    than the cosines') plus the roundings of 1 - lambda, the two products and the sum.  Hence eps = (2 D + 16) 2^-24.  The reference
    is evaluated at the lambda the kernel receives (the C ABI takes a float).

    Cases: n in {1, 2, 17, 32}, m from 1 to n, lambda in {0, 0.3, 0.7, 1}, unit rows, rows of mixed norms, all-zero rows, duplicated
    rows and lists with trailing -1 slots.  None is skipped."""
    eps = eps_of(dim)
    checked = 0
    for n in (1, 2, 17, 32):
        for kind in KINDS:
            q, cand, ids = _case(kind, dim, n, seed=dim * 131 + n * 7 + KINDS.index(kind))
            for m in sorted({1, 2, (n + 1) // 2, n - 1, n} & set(range(1, n + 1))):
                for lam in (0.0, 0.3, 0.7, 1.0):
                    order, val = _select(hip, q, cand, ids, m, lam)
                    for b in range(N_QUERIES):
                        try:
                            certify(q[b], cand[b], ids[b], order[b], val[b], _f32(lam), eps)
                        except AssertionError as e:
                            raise AssertionError(f"dim={dim} n={n} m={m} lambda={lam} {kind} rows, query {b}: {e}") from None
                        checked += 1
    assert checked == sum(len({1, 2, (n + 1) // 2, n - 1, n} & set(range(1, n + 1))) for n in (1, 2, 17, 32)) * len(KINDS) * 4 * N_QUERIES


def test_the_certificate_is_not_vacuous(hip):
    dim, n, m, lam = 768, 32, 10, 0.5
    eps = eps_of(dim)
    q, cand, ids = _case("unit", dim, n, seed=5)
    order, val = _select(hip, q, cand, ids, m, lam)
    certify(q[0], cand[0], ids[0], order[0], val[0], _f32(lam), eps)
    # one pick swapped for a slot whose float64 objective at that step is more than 10 (2 eps) lower
    rel, sim = cosines_f64(q[0], cand[0])
    t = 3
    worst = sim[:, order[0, :t]].max(axis=1)
    obj = _f32(lam) * rel - (1.0 - _f32(lam)) * worst
    free = np.ones(n, bool)
    free[order[0, :t]] = False
    low = [i for i in np.nonzero(free)[0] if obj[i] < obj[order[0, t]] - 20 * eps]
    assert low, "no slot is clearly worse: the case proves nothing"
    bad = order[0].copy()
    bad[t] = low[0]
    bad[t + 1:] = [i for i in np.nonzero(free)[0] if i != low[0]][:m - t - 1]
    with pytest.raises(AssertionError, match=f"step {t}: slot {low[0]} has objective"):
        certify(q[0], cand[0], ids[0], bad, val[0], _f32(lam), eps)
    # a repeated pick
    rep = order[0].copy()
    rep[5] = rep[2]
    with pytest.raises(AssertionError, match="step 5: slot .* was picked before"):
        certify(q[0], cand[0], ids[0], rep, val[0], _f32(lam), eps)
    # an invalid slot picked
    ids2 = ids[0].copy()
    ids2[order[0, 4]] = -1
    with pytest.raises(AssertionError, match="step 4: slot .* is not a valid slot"):
        certify(q[0], cand[0], ids2, order[0], val[0], _f32(lam), eps)
    # a value off by 4 eps
    off = val[0].copy()
    off[6] += 4 * eps
    with pytest.raises(AssertionError, match="step 6: returned"):
        certify(q[0], cand[0], ids[0], order[0], off, _f32(lam), eps)


# ---- exact sequences ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,m,lams", [("cluster", 8, (0.5, 1.0)), ("ladder", 17, (0.3, 0.7, 1.0))])
def test_exact_sequence_on_constructed_inputs(hip, case, m, lams):
    """Constructed inputs at D = 768 on which every step's best objective leads the second best by more than 100 eps in float64 (asserted
    first): the kernel's sequence must then be the reference's, exactly."""
    dim = 768
    q, cand, ids = (cluster_case if case == "cluster" else ladder_case)(dim, np.float16)
    for lam in lams:
        want, _ = mmr_reference_f64(q, cand, ids, m, _f32(lam))
        gaps = step_gaps_f64(q, cand, ids, want[0], _f32(lam))
        assert min(gaps) > 100 * eps_of(dim), f"{case} lambda={lam}: a step's gap {min(gaps):.3e} is not above 100 eps = {100 * eps_of(dim):.3e}"
        order, val = _select(hip, q[None], cand[None], ids[None], m, lam)
        assert order[0].tolist() == want[0].tolist(), (case, lam)
        certify(q, cand, ids, order[0], val[0], _f32(lam), eps_of(dim))
    if case == "cluster":
        o5, _ = _select(hip, q[None], cand[None], ids[None], 8, 0.5)
        assert sorted((o5[0] // 4).tolist()) == list(range(8))          # one row of every group
        o1, _ = _select(hip, q[None], cand[None], ids[None], 8, 1.0)
        assert o1[0].tolist() == list(range(8))


def test_ties_go_to_the_lower_slot(hip):
    dim, n = 320, 20
    rs = np.random.RandomState(3)
    q = _unit(rs, (1, dim))
    cand = _unit(rs, (1, n, dim)) * 0.5
    twin = _unit(rs, (dim,)) + 2.0 * q[0]                       # by far the most relevant row, at slots 3, 7 and 15, bit for bit
    cand[0, [3, 7, 15]] = twin
    q, cand = q.astype(np.float16), cand.astype(np.float16)
    ids = np.arange(50, 50 + n, dtype=np.int64)[None]
    order, val = _select(hip, q, cand, ids, 5, 1.0)
    assert order[0, :3].tolist() == [3, 7, 15] and val[0, 0] == val[0, 1] == val[0, 2]
    order, _ = _select(hip, q, cand, ids, 3, 0.5)               # after the first twin the other two carry the full penalty
    assert order[0, 0] == 3 and 7 not in order[0].tolist() and 15 not in order[0].tolist()
    # lambda = 0: every first objective is 0 -> the lowest VALID slot
    ids2 = ids.copy()
    ids2[0, :2] = -1
    order, val = _select(hip, q, cand, ids2, 3, 0.0)
    assert order[0, 0] == 2 and val[0, 0] == 0.0
    # all rows identical: the order is the slot order
    same = np.repeat(cand[:, 3:4], n, axis=1)
    for lam in (0.0, 0.4, 1.0):
        order, _ = _select(hip, q, same, ids, n, lam)
        assert order[0].tolist() == list(range(n)), lam


def test_a_query_gets_the_same_bits_alone_and_anywhere_in_a_256_query_batch(hip):
    dim, n, m, lam = 768, 32, 10, 0.5
    rs = np.random.RandomState(9)
    q = _unit(rs, (257, dim)).astype(np.float16)
    cand = _unit(rs, (257, n, dim)).astype(np.float16)
    ids = rs.randint(0, 1 << 30, size=(257, n)).astype(np.int64)
    ids[0, 29:] = -1

    def bits(o, v):
        return o.tobytes() + v.tobytes()
    alone = _select(hip, q[:1], cand[:1], ids[:1], m, lam)
    first = _select(hip, q[:256], cand[:256], ids[:256], m, lam)
    perm = np.r_[np.arange(256, 0, -1)[:255], 0]                # other neighbours, the query last
    last = _select(hip, q[perm], cand[perm], ids[perm], m, lam)
    again = _select(hip, q[perm], cand[perm], ids[perm], m, lam)
    assert bits(alone[0][0], alone[1][0]) == bits(first[0][0], first[1][0]) == bits(last[0][255], last[1][255])
    assert bits(*last) == bits(*again)
    assert not np.array_equal(first[0][1], first[0][0])          # (the batch does hold different answers)


def test_argument_checks(hip):
    lib = hip.load()
    z = torch.zeros(32 * 8192, dtype=torch.float16, device="cuda")
    i64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    o32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(64, dtype=torch.float32, device="cuda")

    def call(n, dim, m, lam):
        return lib.arx_mmr_select(z.data_ptr(), z.data_ptr(), i64.data_ptr(), 1, n, dim, m, lam, o32.data_ptr(), f32.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert call(32, 64, 32, 0.5) == 0
    for args, word in (((32, 96, 8, 0.5), "multiple of 64"), ((4, 8256, 2, 0.5), "8192"), ((33, 64, 8, 0.5), "n=33"), ((8, 64, 9, 0.5), "m=9"),
                       ((8, 64, 0, 0.5), "m=0"), ((8, 64, 4, 1.5), "lambda"), ((8, 64, 4, -0.1), "lambda"), ((8, 64, 4, float("nan")), "lambda")):
        assert call(*args) == -1, args
        assert word in lib.arx_last_error().decode(), (args, lib.arx_last_error())
    assert lib.arx_gather_rows(z.data_ptr(), 10, 12, 0, i64.data_ptr(), 4, z.data_ptr(), None) == -1 and b"multiple of 8" in lib.arx_last_error()
    torch.cuda.synchronize()


# ---- HipCollection.query --------------------------------------------------------------------------------------------------------------------
def _score_bits(out, key="scores"):
    return [np.array(s, np.float32).view(np.int32).tolist() for s in out[key]]


def test_collection_query_mmr(hip):
    from arxiv_rag_amd.mmr import mmr_select
    from arxiv_rag_amd.store import HipCollection
    from arxiv_rag_amd.where import compile_where, evaluate
    from arxiv_rag_amd.where_document import compile_where_document, evaluate_host
    from oracle import search_oracle as SO
    from tests.test_gpu_filtered_search import _collection
    emb, meta = _collection()
    coll = HipCollection(emb, meta, documents=True)
    q = SO.unit_rows_f16(12, 128, 9)
    qd = torch.from_numpy(q).cuda()
    # without mmr_lambda nothing changes
    assert coll.query(query_embeddings=q, n_results=10, mmr_lambda=None) == coll.query(query_embeddings=q, n_results=10)
    assert "mmr_scores" not in coll.query(query_embeddings=q, n_results=10)
    # with it: ids[order] of a direct search + mmr_select, the search's scores of those rows
    for lam, n_results, n_cand in ((0.5, 10, 32), (0.2, 5, 16), (1.0, 8, 8), (0.0, 32, 32)):
        out = coll.query(query_embeddings=q, n_results=n_results, n_candidates=n_cand, mmr_lambda=lam)
        s, i = coll.index.search(qd, n_cand)
        order, val = mmr_select(coll.index, qd, i, n_results, lam)
        pos = order.long()
        assert (order >= 0).all()
        assert out["indices"] == i.gather(1, pos).cpu().tolist(), lam
        assert _score_bits(out) == s.gather(1, pos).cpu().numpy().view(np.int32).tolist()
        assert _score_bits(out, "mmr_scores") == val.cpu().numpy().view(np.int32).tolist()
        assert out["distances"] == [(2.0 - 2.0 * np.array(sc, np.float32)).tolist() for sc in out["scores"]]
        assert out["documents"] == [[meta[r]["text"] for r in rows] for rows in out["indices"]]
        eps = eps_of(128)
        cand = emb.astype(np.float16)[i.cpu().numpy()]
        for b in range(q.shape[0]):
            certify(q[b], cand[b], i[b].cpu().numpy(), order[b].cpu().numpy(), val[b].cpu().numpy(), _f32(lam), eps)
    top = coll.query(query_embeddings=q, n_results=8)              # lambda = 1 and no spare candidate: the same rows
    assert [sorted(r) for r in coll.query(query_embeddings=q, n_results=8, n_candidates=8, mmr_lambda=1.0)["indices"]] == [sorted(r) for r in top["indices"]]
    # with filters: no disallowed row, and MMR over the filtered search's candidates
    from arxiv_rag_amd.where import pack_bitmap
    where, wdoc = {"section": "abstract"}, {"$contains": "alpha beta"}
    m_where = evaluate(compile_where(where), meta)
    m_doc = evaluate_host(compile_where_document(wdoc), [m["text"] for m in meta])
    for kw, mask in (({"where": where}, m_where), ({"where_document": wdoc}, m_doc), ({"where": where, "where_document": wdoc}, m_where & m_doc)):
        assert 32 < mask.sum() < len(meta)
        out = coll.query(query_embeddings=q, n_results=10, n_candidates=24, mmr_lambda=0.5, **kw)
        allow = torch.from_numpy(pack_bitmap(mask).view(np.int64)).cuda()
        s, i = coll.index.search(qd, 24, allow=allow, n_allowed=int(mask.sum()))
        order, val = mmr_select(coll.index, qd, i, 10, 0.5)
        assert out["indices"] == i.gather(1, order.long()).cpu().tolist(), kw
        assert _score_bits(out) == s.gather(1, order.long()).cpu().numpy().view(np.int32).tolist()
        assert all(mask[r] for rows in out["indices"] for r in rows) and all(len(rows) == 10 for rows in out["indices"])
    # a filter that leaves fewer rows than n_results: short lists, no padding entries
    few = {"paper_id": "0704.0007"}
    out = coll.query(query_embeddings=q, n_results=10, n_candidates=20, mmr_lambda=0.5, where=few)
    n_few = int(evaluate(compile_where(few), meta).sum())
    assert 0 < n_few < 10 and all(len(rows) == n_few == len(ms) for rows, ms in zip(out["indices"], out["mmr_scores"]))
    assert all(meta[r]["paper_id"] == "0704.0007" for rows in out["indices"] for r in rows)
    # refusals

    class LengthReranker:
        def predict(self, pairs, **kw):
            return np.array([len(doc) for _, doc in pairs], np.float32)
    with pytest.raises(ValueError, match="reranker"):
        coll.query(query_embeddings=q, query_texts=["a"] * 12, reranker=LengthReranker(), mmr_lambda=0.5)
    with pytest.raises(ValueError, match="hybrid_alpha"):
        coll.query(query_embeddings=q, query_texts=["a"] * 12, hybrid_alpha=0.5, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="mmr_lambda"):
        coll.query(query_embeddings=q, mmr_lambda=1.5)
    with pytest.raises(ValueError, match="n_candidates"):
        coll.query(query_embeddings=q, n_candidates=33, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="n_candidates"):
        coll.query(query_embeddings=q, n_results=10, n_candidates=9, mmr_lambda=0.5)


def test_mmr_returns_distinct_originals_where_the_plain_query_returns_duplicates(hip):
    """A corpus that holds each chunk four times as near-duplicates (overlapping windows of one passage): the plain top 8 repeats
    originals, `mmr_lambda=0.5` returns 8 distinct ones."""
    from arxiv_rag_amd.store import HipCollection
    rs = np.random.RandomState(21)
    n_orig, dim = 500, 128
    base = _unit(rs, (n_orig, dim))
    rows = np.repeat(base, 4, axis=0) + 0.004 * rs.standard_normal((4 * n_orig, dim))      # copy c of original o is row 4 o + c
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    inside = np.einsum("ocd,oed->oce", rows.reshape(n_orig, 4, dim), rows.reshape(n_orig, 4, dim))
    assert inside.min() > 0.99
    meta = [{"chunk_id": f"c{r}", "text": f"t{r}"} for r in range(4 * n_orig)]
    coll = HipCollection(rows.astype(np.float32), meta)
    q = (base[rs.randint(0, n_orig, size=16)] + 0.6 * _unit(rs, (16, dim))).astype(np.float16)
    plain = coll.query(query_embeddings=q, n_results=8)
    div = coll.query(query_embeddings=q, n_results=8, n_candidates=32, mmr_lambda=0.5)
    for b in range(16):
        assert len({r // 4 for r in plain["indices"][b]}) < 8, "the plain top 8 holds no duplicate: the corpus proves nothing"
        assert len(div["indices"][b]) == 8 and len({r // 4 for r in div["indices"][b]}) == 8, (b, div["indices"][b])
        assert div["indices"][b][0] == plain["indices"][b][0]      # the first pick is the most relevant row


# ---- CLI and process group ------------------------------------------------------------------------------------------------------------------
def test_cli_mmr_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script with --queries --mmr-lambda 0.5 --mmr-fetch-k 16 --top-k 5: the hits are, in order, what the Python path
    (search of 16 + mmr_select on the rows the script wrote) picks, each with `mmr_score`; with --mmr-lambda 1.0 the set is the top 5."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.index import ShardIndex
    from arxiv_rag_amd.mmr import mmr_select
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=60, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text("\n".join(" ".join(words[i:i + 6]) for i in range(0, 48, 6)) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    qs = (tmp_path / "queries.txt").read_text().split("\n")[:-1]
    base = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
            "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt"), "--top-k", "5"]
    for lam in ("0.5", "1.0"):
        GEN._model, GEN._model_name = None, None
        assert GEN.main(base + ["--mmr-lambda", lam, "--mmr-fetch-k", "16"]) == 0
        res = json.loads((tmp_path / "embeddings_saved" / "search_results.json").read_text())
        assert [r["query"] for r in res] == qs
        kept = GEN.load_chunks_parallel(tmp_path / "in", 0.9, 4)
        arr = np.load(tmp_path / "embeddings_saved" / "embeddings.npy")
        qd = torch.empty((len(qs), 384), dtype=torch.float16, device="cuda")
        GEN._model.encode(qs, normalize_embeddings=True, device_f16_out=qd, low_latency=True)
        index = ShardIndex(torch.from_numpy(arr.astype(np.float16)).cuda())
        s, i = index.search(qd, 16)
        order, val = mmr_select(index, qd, i, 5, float(lam))
        want_i, want_s = i.gather(1, order.long()).cpu().numpy(), s.gather(1, order.long()).cpu().numpy()
        for qi, r in enumerate(res):
            assert [h["index"] for h in r["results"]] == want_i[qi].tolist(), (lam, qi)
            assert [h["rank"] for h in r["results"]] == [1, 2, 3, 4, 5]
            assert all(set(h) == {"rank", "score", "index", "chunk_id", "mmr_score"} for h in r["results"])
            assert [h["chunk_id"] for h in r["results"]] == [kept[j]["chunk_id"] for j in want_i[qi]]
            assert np.array_equal(np.array([h["score"] for h in r["results"]], np.float32), want_s[qi])
            assert np.array_equal(np.array([h["mmr_score"] for h in r["results"]], np.float32), val[qi].cpu().numpy())
            if lam == "1.0":
                assert {h["index"] for h in r["results"]} == set(i[qi, :5].tolist())
    GEN._model.encoder.close()
    GEN._model, GEN._model_name = None, None


def test_mmr_under_a_single_rank_rccl_group_equals_no_group(hip):
    """The path through `exchange_candidate_rows` (an RCCL all_reduce of the gathered rows) with a one-rank group: the same bits as
    without a group.  Multi-rank MMR has run at world size 1 on hardware only; the sum over two ranks is checked on CPU tensors over gloo
    (tests/test_mmr_host.py)."""
    import torch.distributed as dist
    from arxiv_rag_amd.index import ShardIndex
    from arxiv_rag_amd.mmr import exchange_candidate_rows, gather_rows, mmr_select
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    Cm, Q = SO.unit_rows_f16(5000, 128, 1), SO.unit_rows_f16(33, 128, 2)
    idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=7)
    qd = torch.from_numpy(Q).cuda()
    s0, i0 = idx.search(qd, 32)
    # without a group: gather + select through the C ABI, no exchange step at all
    rows0 = gather_rows(idx, i0)
    assert torch.equal(rows0.view(torch.int16), torch.from_numpy(Cm).cuda()[i0 - 7].view(torch.int16))
    o0, v0 = _select(hip, Q, rows0.cpu().numpy(), i0.cpu().numpy(), 10, 0.5)
    coll = HipCollection(Cm.astype(np.float32), [{"chunk_id": f"c{r}", "text": f"t{r}"} for r in range(5000)])
    created = not dist.is_initialized()
    out0 = coll.query(query_embeddings=Q, n_results=10, mmr_lambda=0.5) if created else None
    if created:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29537", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        summed = exchange_candidate_rows(rows0.clone())
        assert torch.equal(summed.view(torch.int16), rows0.view(torch.int16))
        s1, i1 = idx.search_distributed(qd, 32)
        o1, v1 = mmr_select(idx, qd, i1, 10, 0.5)
        torch.cuda.synchronize()
        out1 = coll.query(query_embeddings=Q, n_results=10, mmr_lambda=0.5)
    finally:
        if created:
            dist.destroy_process_group()
    assert torch.equal(i0, i1) and np.array_equal(o0, o1.cpu().numpy()) and np.array_equal(v0.view(np.int32), v1.cpu().numpy().view(np.int32))
    assert out1["indices"] == (i1.gather(1, o1.long()) - 7).cpu().tolist()          # (the collection numbers the same rows from 0, `idx` from 7)
    assert out0 is None or out0 == out1
