"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (ctypes), against the CPU oracle and
the committed golden vectors.  Tolerances: encoder per-vector cosine >= 1 - 1e-3 (BASELINE.json north_star;
bf16 weights/activations vs fp32 oracle); search top-10 set-equal, except where the oracle's own k-th /
(k+1)-th scores differ by < 1e-6 (two fp32 accumulation orders cannot rank such a pair reliably)."""
import os

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import seeded_state_dict
from oracle import encoder_oracle as EO
from oracle import search_oracle as SO
from tests.helpers import ATTN_KERNELS, attention_budget, attention_fp64, gemm_epilogue_budget, gemm_epilogue_fp64, need_dev, tiny_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1) + 1e-30)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from arxiv_rag_amd import _lib
    _lib.load()                                   # fails loudly if libarx_hip.so is missing
    return _lib


@pytest.mark.parametrize("name", ["tiny-mpnet", "tiny-bert", "tiny-bert-cls"])
def test_tiny_golden_all_layers(hip, golden_dir, name):
    from arxiv_rag_amd.encoder import HipEncoder
    g = np.load(golden_dir / f"{name}.npz")
    cfg = C.PRESETS[name]
    sd = tiny_weights(g, cfg)
    ids, lens = g["ids"], g["lens"]
    enc = HipEncoder(cfg, sd)
    valid = np.arange(ids.shape[1])[None] < lens[:, None]
    for layer in range(cfg.layers + 1):
        hid = enc.tap_hidden(ids, lens, layer)
        ref = g[f"hidden_{layer}"][valid]
        assert np.isfinite(hid).all()
        assert np.abs(hid - ref).max() < 0.08, (name, layer)          # bf16 activations, |x| ~ 4
        assert _cos(hid, ref).min() > 1 - 2e-4
    emb = enc.encode_tokens(ids, lens).cpu().numpy()
    assert _cos(emb, g["emb"]).min() > 1 - 1e-3
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5
    raw = enc.encode_tokens(ids, lens, normalize=False).cpu().numpy()
    assert _cos(raw, g["pooled"]).min() > 1 - 1e-3
    enc.close()


@pytest.mark.parametrize("name,key", [("all-mpnet-base-v2", "all-mpnet-base-v2:w05"),
                                      ("all-mpnet-base-v2", "all-mpnet-base-v2:hf02"),
                                      ("all-MiniLM-L6-v2", "all-MiniLM-L6-v2:w05"),
                                      ("all-MiniLM-L6-v2", "all-MiniLM-L6-v2:hf02"),
                                      ("BAAI/bge-large-en-v1.5", "BAAI_bge-large-en-v1.5:w05")])
def test_full_shape_golden(hip, golden_dir, name, key):
    """Full-size shapes: weights regenerated from (seed, stds); 16 ragged sequences (lens 1..256)."""
    from arxiv_rag_amd.encoder import HipEncoder
    g = np.load(golden_dir / "full_shapes.npz")
    cfg = C.PRESETS[name]
    seed, std, bstd, jit = g[key + ":wspec"]
    sd = seeded_state_dict(cfg, seed=int(seed), std=std, bias_std=bstd, ln_jitter=jit)
    ids, lens, ref = g[key + ":ids"], g[key + ":lens"], g[key + ":emb"]
    enc = HipEncoder(cfg, sd)
    emb = enc.encode_tokens(ids, lens).cpu().numpy()
    assert _cos(emb, ref).min() > 1 - 1e-3
    # order contract + batch-composition independence: ragged re-bucketing returns rows in input order
    seqs = [ids[r, :lens[r]].tolist() for r in range(len(lens))]
    emb2 = enc.encode_ragged(seqs, batch_size=5)
    assert _cos(emb2, ref).min() > 1 - 1e-3
    # bitwise: token-packed activations, fixed-order row statistics and a per-(sequence, head) attention block make a row
    # independent of what else is in the batch, of the padded width and of the forward's size
    assert np.array_equal(emb2, emb)
    solo = np.concatenate([enc.encode_ragged([sq]) for sq in seqs[:6]], 0)
    assert np.array_equal(solo, emb[:6])
    wide = np.full((len(lens), 384), cfg.pad_id, ids.dtype); wide[:, :ids.shape[1]] = ids
    assert np.array_equal(enc.encode_tokens(wide, lens).cpu().numpy(), emb)
    enc.close()


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("name", ["all-mpnet-base-v2", "all-MiniLM-L6-v2", "BAAI/bge-large-en-v1.5"])
def test_full_shape_adversarial_statistics(hip, golden_dir, name, fold):
    """The regime seeded N(0, sigma) weights never reach (VERDICT r1 / ADVICE): LayerNorm gamma log-uniform in [0.25, 4] with
    outlier channels at 10, beta with +-5 outliers, every pre-LN row offset by 4 (|mean| >> spread: the one-pass variance
    E[y^2] - mean^2 cancels, the bf16 pre-LN stream sits on a coarse grid), Student-t matrices.  Both the LN-fold schedule and
    the explicit-LayerNorm schedule must hold the north-star bar against the transformers outputs in full_shapes_adv.npz."""
    from arxiv_rag_amd.encoder import HipEncoder
    from arxiv_rag_amd.weights import adversarial_state_dict
    g = np.load(golden_dir / "full_shapes_adv.npz")
    cfg = C.PRESETS[name]
    key = name.replace("/", "_") + ":adv"
    seed, off = g[key + ":wspec"]
    sd = adversarial_state_dict(cfg, seed=int(seed), row_offset=float(off))
    ids, lens, ref = g[key + ":ids"], g[key + ":lens"], g[key + ":emb"]
    enc = HipEncoder(cfg, sd, ln_fold=(fold == "1"))
    emb = enc.encode_tokens(ids, lens).cpu().numpy()
    enc.close()
    c = _cos(emb, ref)
    print(f"adversarial {name} ln_fold={fold}: worst 1-cos = {1 - c.min():.2e}")
    assert np.isfinite(emb).all() and c.min() > 1 - 1e-3, (name, fold, 1 - c.min())


def test_encoder_vs_oracle_random_batch(hip):
    """Seeded inputs the golden files do not hold: MiniLM shape, 24 ragged rows incl. len 1, 2 and max 256."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.MINILM_L6
    sd = seeded_state_dict(cfg, seed=5, std=0.04, bias_std=0.03, ln_jitter=0.05)
    rs = np.random.RandomState(1)
    lens = np.array([256, 1, 2, 255, 31, 32, 33, 64, 65, 100, 128, 129, 3, 17, 200, 250, 96, 97, 7, 8, 9, 63, 127, 191], np.int64)
    ids = np.zeros((len(lens), 256), np.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(1, cfg.vocab_size, size=n)
    ref = EO.encode_tokens(sd, cfg, ids, lens)
    enc = HipEncoder(cfg, sd)
    emb = enc.encode_tokens(ids, lens).cpu().numpy()
    assert _cos(emb, ref).min() > 1 - 1e-3
    enc.close()


def test_encoder_rows_bitwise_independent_of_random_batch_compositions(hip):
    """The size-independent property behind the order contract (GEN:146-153 re-batches freely): a row is the same BITS whatever else is in
    its forward.  A short in-suite cut of tools/encode_soak.py (profiles/r04/encode_soak.txt: 7 765 random compositions of three models,
    365 M tokens): pool of ragged sequences on tile-edge lengths, random subsets / orders / batch sizes, f32 and fp16 outputs."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.MINILM_L6
    sd = seeded_state_dict(cfg, seed=21, std=0.04, bias_std=0.02, ln_jitter=0.05)
    rs = np.random.RandomState(4)
    edges = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]
    P = 400
    lens = np.where(rs.rand(P) < 0.4, rs.choice(edges, size=P), rs.randint(1, cfg.max_seq_length + 1, size=P))
    pool = [rs.randint(4, cfg.vocab_size - 1, size=int(n)).tolist() for n in lens]
    enc = HipEncoder(cfg, sd)
    ref16 = torch.zeros((P, cfg.hidden), dtype=torch.float16, device="cuda")
    ref = enc.encode_ragged(pool, batch_size=256, on_device=True, out_f16=ref16).clone()
    assert torch.isfinite(ref).all() and (ref.norm(dim=1) - 1).abs().max().item() < 1e-5
    for trial in range(30):
        n = int([1, rs.randint(1, 9), rs.randint(9, 120), rs.randint(120, P + 1)][trial % 4])
        pick = rs.choice(P, size=n, replace=(trial % 5 == 0))
        bs = int([1, rs.randint(1, 33), rs.randint(33, 257), 1024][(trial // 4) % 4]) if n <= 64 else int(rs.randint(5, 1025))
        o16 = torch.full((n, cfg.hidden + 8), 7.0, dtype=torch.float16, device="cuda")
        out = enc.encode_ragged([pool[i] for i in pick], batch_size=bs, on_device=True, out_f16=o16)
        pk = torch.from_numpy(pick).cuda()
        assert torch.equal(out, ref[pk]), (trial, n, bs)
        assert torch.equal(o16[:, :cfg.hidden], ref16[pk]) and (o16[:, cfg.hidden:] == 7.0).all(), (trial, n, bs)
    enc.close()


def test_encoder_empty_rows_and_pad_garbage(hip):
    """len 0 rows give zero vectors; ids beyond lens are ignored whatever they hold (GEN:169 zero-row contract)."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.TINY_MPNET
    sd = seeded_state_dict(cfg, seed=2, std=0.05)
    rs = np.random.RandomState(0)
    lens = np.array([10, 0, 64, 0, 5], np.int32)
    ids = rs.randint(4, cfg.vocab_size, size=(5, 64)).astype(np.int32)
    enc = HipEncoder(cfg, sd)
    a = enc.encode_tokens(ids, lens).cpu().numpy()
    ids2 = ids.copy()
    for r, n in enumerate(lens):
        ids2[r, n:] = cfg.pad_id
    b = enc.encode_tokens(ids2, lens).cpu().numpy()
    assert np.array_equal(a[[1, 3]], np.zeros((2, cfg.hidden), np.float32))
    assert np.array_equal(a, b)
    ref = EO.encode_tokens(sd, cfg, ids2.astype(np.int64)[[0, 2, 4]], lens[[0, 2, 4]].astype(np.int64))
    assert _cos(a[[0, 2, 4]], ref).min() > 1 - 1e-3
    enc.close()


def test_encoder_capacity_and_arg_errors(hip):
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.TINY_BERT
    enc = HipEncoder(cfg, seeded_state_dict(cfg, seed=1), max_tokens=64, max_seqs=2)
    ids = torch.zeros((2, 600), dtype=torch.int32, device="cuda")
    lens = torch.full((2,), 600, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.ArxError):
        enc.forward_tokens(ids, lens, 600, 1200)          # max_len > 512
    enc.close()


def _check_search(C_, Q_, k, idx_base=0, prefilter=None):
    from arxiv_rag_amd.index import ShardIndex
    s, i = ShardIndex(torch.from_numpy(C_).cuda(), idx_base=idx_base, prefilter=prefilter).search(torch.from_numpy(Q_).cuda(), k)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    # oracle with one extra candidate to measure the k-th / (k+1)-th gap
    rs, ri = SO.topk_search(C_, Q_, k + 1, idx_base=idx_base)
    fin = np.isfinite(rs[:, :k])
    assert np.abs(s[fin] - rs[:, :k][fin]).max() < 1e-5
    assert np.array_equal(np.isfinite(s), np.isfinite(rs[:, :k]))
    for q in range(Q_.shape[0]):
        if set(i[q].tolist()) != set(ri[q, :k].tolist()):
            gap = rs[q, k - 1] - rs[q, k]
            assert gap < 1e-6, (q, i[q], ri[q], gap)
    return s, i, rs[:, :k], ri[:, :k]


def test_search_golden_with_exact_ties(hip, golden_dir):
    g = np.load(golden_dir / "search_4096x768.npz")
    Cm = SO.unit_rows_f16(4096, 768, 7); Q = SO.unit_rows_f16(64, 768, 11)
    Cm[100] = Cm[17]; Cm[2000] = Cm[17]; Cm[3000] = Cm[17]; Q[0] = Cm[17]
    s, i, _, _ = _check_search(Cm, Q, 10)
    assert i[0, :4].tolist() == [17, 100, 2000, 3000]          # exact ties -> lower index first
    assert (i == g["ids"]).all(axis=1).mean() > 0.95


@pytest.mark.parametrize("n,nq,d,k", [(5000, 77, 768, 10), (130, 3, 128, 10), (7, 2, 64, 10), (70000, 200, 384, 10),
                                      (3000, 300, 1024, 5), (9000, 1500, 256, 10), (64, 1, 768, 1), (100000, 130, 768, 32)])
def test_search_vs_oracle_shapes(hip, n, nq, d, k):
    """ragged sizes: n not a multiple of 64/256, every query-tile variant (<=64, <=128, >128, >1024), k > n."""
    _check_search(SO.unit_rows_f16(n, d, 3), SO.unit_rows_f16(nq, d, 4), k, idx_base=12345)


@pytest.mark.parametrize("n,nq,d,k", [(5000, 77, 768, 10), (130, 3, 128, 10), (70000, 200, 384, 10), (3000, 300, 1024, 5),
                                      (9000, 1500, 256, 10), (64, 1, 768, 1), (100000, 130, 768, 32), (1, 5, 128, 3)])
def test_search_int8_prefilter_is_exact(hip, n, nq, d, k):
    """`ShardIndex(prefilter="int8")` (arx_topk_search_i8): the first pass runs over int8 rows and yields UPPER BOUNDS; the answer must be
    the oracle's exact top-k all the same — same shapes as the fp16 test (every query-tile variant, ragged row counts, k > n), and
    bit-identical scores and ids to the fp16 pass of the same index."""
    from arxiv_rag_amd.index import ShardIndex
    Cm, Q = SO.unit_rows_f16(n, d, 3), SO.unit_rows_f16(nq, d, 4)
    s8, i8, _, _ = _check_search(Cm, Q, k, idx_base=12345, prefilter="int8")
    s16, i16 = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=12345).search(torch.from_numpy(Q).cuda(), k)
    s16, i16 = s16.cpu().numpy(), i16.cpu().numpy()
    same = (i8 == i16).all(axis=1)
    assert same.mean() > 0.98                                  # (rows tied to 1e-6 may be taken in either order by the two selections)
    assert np.array_equal(s8[same], s16[same])                  # same rows -> the same fp32 rescoring, bit for bit


def test_search_int8_prefilter_adversarial_rows(hip):
    """Rows on which int8 quantisation is at its worst — one huge coordinate (scale set by an outlier: every other coordinate rounds to
    0 or +-1), near-duplicates of the query differing in a few low-order bits, rows of very different norms, all-zero rows — and
    the planted near-tie corpus of the certificate test.  The bound must hold on each: exact answers, checked row by row."""
    from arxiv_rag_amd.index import ShardIndex
    rs = np.random.RandomState(77)
    d, n = 256, 64 * 300
    Cm = SO.unit_rows_f16(n, d, 31).astype(np.float32); Q = SO.unit_rows_f16(8, d, 32).astype(np.float32)
    out = rs.choice(n, size=2000, replace=False)
    Cm[out[:700], rs.randint(d, size=700)] = 3.0 * np.sign(rs.standard_normal(700))          # outlier coordinate
    Cm[out[700:1000]] *= rs.uniform(0.01, 8.0, size=(300, 1))                                   # norms far from 1
    Cm[out[1000:1100]] = 0.0
    for j, r in enumerate(out[1100:1400]):                                                       # near-duplicates of queries
        v = Q[j % 8].copy(); c = rs.randint(d, size=3); v[c] *= (1 + 2.0 ** -9 * rs.choice([-1, 1], size=3)); Cm[r] = v
    Q[3, 5] = 2.5                                                                                # a query with an outlier coordinate too
    Cm, Q = Cm.astype(np.float16), Q.astype(np.float16)
    for k in (10, 32):
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), prefilter="int8")
        s, i = idx.search(torch.from_numpy(Q).cuda(), k)
        _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, tol=2e-6 * float(np.abs(Cm.astype(np.float32)).max()) ** 2 * 4)
    # the same rows under the wide query tiles (Qb = 256 and > 1024: the int8 pass is now the default at every batch size)
    for nq_big in (256, 1100):
        Qb = np.concatenate([Q, SO.unit_rows_f16(nq_big - len(Q), d, 33)])
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), prefilter="int8")
        s, i = idx.search(torch.from_numpy(Qb).cuda(), 10)
        _assert_topk_valid(Cm, Qb, s.cpu().numpy(), i.cpu().numpy(), 10, tol=2e-6 * float(np.abs(Cm.astype(np.float32)).max()) ** 2 * 4)
    Cn, Qn, planted = _near_tied_corpus(60)
    idx = ShardIndex(torch.from_numpy(Cn).cuda(), idx_base=7, prefilter="int8")
    s, i = idx.search(torch.from_numpy(Qn).cuda(), 10)
    _assert_topk_valid(Cn, Qn, s.cpu().numpy(), i.cpu().numpy(), 10, idx_base=7)
    assert set(i.cpu().numpy()[0].tolist()) <= {p + 7 for p in planted}


def test_search_int8_prefilter_overflow_falls_back_to_the_exhaustive_kernel(hip):
    """More candidate groups than the pre-filter's pair list holds (a corpus of 320 000 IDENTICAL rows: every one of the 5 000 groups
    reaches every query's threshold, and every row survives it): the candidate pipeline flags the queries and the exhaustive kernel
    answers them — ids 0..k-1 (ties -> lower row), and the counters say the slow path ran for every query."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = np.tile(SO.unit_rows_f16(1, 128, 1), (64 * 5000, 1)); Q = SO.unit_rows_f16(3, 128, 2)
    idx = ShardIndex(torch.from_numpy(Cm).cuda(), prefilter="int8")
    s, i = idx.search(torch.from_numpy(Q).cuda(), 10)
    flagged, _ = idx.certificate_stats()
    assert np.array_equal(i.cpu().numpy(), np.tile(np.arange(10), (3, 1)))
    ref = (Q.astype(np.float32) @ Cm[:1].astype(np.float32).T)
    assert np.abs(s.cpu().numpy() - ref).max() < 1e-5
    assert flagged >= 3
    # a mixed case: survivors overflow for ONE query only (300 exact copies of it among random rows), the others take the fast pipeline
    rs = np.random.RandomState(5)
    Cr = SO.unit_rows_f16(64 * 600, 256, 9); Qr = SO.unit_rows_f16(5, 256, 10)
    Cr[rs.choice(len(Cr), size=300, replace=False)] = Qr[2]
    idx = ShardIndex(torch.from_numpy(Cr).cuda(), idx_base=50, prefilter="int8")
    s, i = idx.search(torch.from_numpy(Qr).cuda(), 10)
    _assert_topk_valid(Cr, Qr, s.cpu().numpy(), i.cpu().numpy(), 10, idx_base=50)
    assert idx.certificate_stats()[0] >= 1
    # the same with 256 and 1 030 queries per call (wide query tiles, two internal passes): overflow stays per query
    for nq_big in (256, 1030):
        Qb = np.concatenate([Qr, SO.unit_rows_f16(nq_big - len(Qr), 256, 12)])
        s, i = idx.search(torch.from_numpy(Qb).cuda(), 10)
        _assert_topk_valid(Cr, Qb, s.cpu().numpy(), i.cpu().numpy(), 10, idx_base=50)
        flagged, _ = idx.certificate_stats()
        assert 1 <= flagged <= 3, flagged
    # every query of a 300-query batch overflowing: all go through the exhaustive kernel, all exact
    Q300 = SO.unit_rows_f16(300, 128, 2)
    idx = ShardIndex(torch.from_numpy(Cm).cuda(), prefilter="int8")
    s, i = idx.search(torch.from_numpy(Q300).cuda(), 10)
    assert np.array_equal(i.cpu().numpy(), np.tile(np.arange(10), (300, 1))) and idx.certificate_stats()[0] == 300


def test_search_duplicate_rows_everywhere(hip):
    """degenerate corpus (all rows equal, e.g. zero-vector fallback rows): ids must be 0..k-1."""
    Cm = np.tile(SO.unit_rows_f16(1, 128, 1), (1000, 1)); Q = SO.unit_rows_f16(5, 128, 2)
    s, i, rs, ri = _check_search(Cm, Q, 10)
    assert np.array_equal(i, np.tile(np.arange(10), (5, 1)))
    Z = np.zeros((500, 128), np.float16)
    s, i, _, _ = _check_search(Z, Q, 10)
    assert np.array_equal(i, np.tile(np.arange(10), (5, 1))) and (s == 0).all()


def _near_tied_corpus(n_groups_hit, d=256, n=64 * 400, seed=21):
    """A corpus in which MORE 64-row groups than the selection keeps hold a row tied (to the last bit) or nearly tied with the
    query's k-th best match: boilerplate / duplicated chunks.  One planted row per group, in `n_groups_hit` groups spread over
    the corpus, in DEcreasing group order of quality so that 'first K groups by position' is the wrong choice."""
    Cm = SO.unit_rows_f16(n, d, seed); Q = SO.unit_rows_f16(6, d, seed + 1)
    rs = np.random.RandomState(seed + 2)
    groups = rs.permutation(n // 64)[:n_groups_hit]
    planted = []
    for j, g in enumerate(groups):
        row = int(g) * 64 + int(rs.randint(64))
        v = Q[0].astype(np.float32).copy()
        if j % 3 == 1:                                        # near tie: one coordinate moved by one fp16 ulp
            c = int(rs.randint(d)); v[c] = np.nextafter(np.float16(v[c]), np.float16(0)).astype(np.float32)
        elif j % 3 == 2:
            c = int(rs.randint(d)); v[c] = np.nextafter(np.float16(v[c]), np.float16(2)).astype(np.float32)
        Cm[row] = v.astype(np.float16)
        planted.append(row)
    return Cm, Q, sorted(planted)


def _assert_same_topk_up_to_ties(corpus, Q, a, b, idx_base=0, tol=2e-6):
    """Two top-k answers (scores, ids) for the same queries must be the SAME rows, except where the exact fp32 scores of the rows
    that differ are equal within `tol` (near-ties, among which any choice is an exact answer).  Checked on the device against the
    fp32 dot products of the candidate rows themselves — no fraction of queries is let off."""
    (sa, ia), (sb, ib) = a, b
    diff = (~(ia == ib).all(dim=1)).nonzero().flatten()
    same = (ia == ib).all(dim=1)
    assert torch.equal(sa[same], sb[same])
    for q in diff.tolist():
        qv = Q[q].float()
        xa = (corpus[(ia[q] - idx_base)].float() @ qv).sort(descending=True).values
        xb = (corpus[(ib[q] - idx_base)].float() @ qv).sort(descending=True).values
        assert (xa - xb).abs().max().item() <= tol, (q, (xa - xb).abs().max().item())
        assert (sa[q] - xa).abs().max().item() < 1e-5 and (sb[q] - xb).abs().max().item() < 1e-5
    return len(diff)


def _assert_topk_valid(Cm, Q, s, i, k, idx_base=0, tol=1e-6):
    """A returned top-k list is right iff, by the oracle's own fp32 scores of EVERY row: the scores reported are those rows'
    scores, no row left out beats a row returned by more than `tol`, the list is in non-increasing order up to `tol`, and rows
    whose reported scores are equal to the last bit come in ascending id order.  (Two fp32 evaluation orders cannot rank rows
    that differ by less than ~1e-6; among such near-ties any choice is an exact answer.)"""
    full = Q.astype(np.float32) @ Cm.astype(np.float32).T
    for qi in range(Q.shape[0]):
        ids = i[qi] - idx_base
        assert len(set(ids.tolist())) == k and ids.min() >= 0 and ids.max() < Cm.shape[0]
        ref = full[qi, ids]
        assert np.abs(ref - s[qi]).max() < 1e-5
        rest = np.delete(full[qi], ids)
        assert rest.max() <= ref.min() + tol, (qi, rest.max() - ref.min())
        assert (ref[:-1] >= ref[1:] - tol).all()
        same = s[qi][:-1] == s[qi][1:]
        assert (ids[:-1][same] < ids[1:][same]).all()


@pytest.mark.parametrize("k", [10, 32])
def test_search_certificate_near_tied_groups(hip, k):
    """>= 17 (k = 10: 12 selected; k = 32: 36 selected) groups tied or nearly tied at the top: the first selection cannot be
    certified, the kernel must say so (flag counter) and still return exactly the oracle's rows, ties -> lower row."""
    from arxiv_rag_amd.index import ShardIndex
    Cm, Q, planted = _near_tied_corpus(60)
    idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=1000)
    s, i = idx.search(torch.from_numpy(Q).cuda(), k)
    flagged, extra = idx.certificate_stats()
    rs, ri = SO.topk_search(Cm, Q, k, idx_base=1000)
    _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=1000)
    assert np.array_equal(i.cpu().numpy()[1:], ri[1:])                    # the queries without planted near-ties: the oracle's rows
    assert set(i.cpu().numpy()[0].tolist()) <= {p + 1000 for p in planted}
    assert flagged >= 1 and extra >= 8                                    # query 0 went through the fallback (20 exact ties alone overflow nothing less)
    # a corpus with no such structure certifies at once
    Cr = SO.unit_rows_f16(64 * 400, 256, 5)
    idx2 = ShardIndex(torch.from_numpy(Cr).cuda())
    idx2.search(torch.from_numpy(Q).cuda(), k)
    assert idx2.certificate_stats()[0] <= 1


def test_search_certificate_recovers_a_missed_group(hip):
    """Test hook `drop_best=1` (arx_topk_options.debug_drop_best, per call) makes the selection forget its best group (as a rounding
    accident at the boundary would): without the certificate the top hit would be lost; with it the answer is the oracle's.
    tau_mult = 1e9 turns the fallback into an exhaustive exact scan: same answer again.  The hook can only WIDEN the tolerance: a
    multiplier below 1 is refused (a stray environment variable used to be able to shrink it).  The hooks are arguments of
    the call: the SAME index searched without them right afterwards certifies at once (no process-wide state)."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(30000, 384, 8); Q = SO.unit_rows_f16(40, 384, 9)
    rs, ri = SO.topk_search(Cm, Q, 11)
    base = ShardIndex(torch.from_numpy(Cm).cuda())
    qd = torch.from_numpy(Q).cuda()
    s0, i0 = base.search(qd, 10)
    assert base.certificate_stats()[0] <= 1
    with pytest.raises(hip.ArxError):
        base.search(qd, 10, tau_mult=0.5)
    for hook in (dict(drop_best=1), dict(tau_mult=1e9)):
        s, i = base.search(qd, 10, **hook)
        flagged, extra = base.certificate_stats()
        assert flagged == 40 and extra >= 40, (hook, flagged, extra)
        assert torch.equal(i, i0) and torch.equal(s, s0), hook
        s, i = base.search(qd, 10)
        assert base.certificate_stats()[0] <= 1 and torch.equal(i, i0) and torch.equal(s, s0)
    i0 = i0.cpu().numpy()
    for q in range(40):
        if set(i0[q].tolist()) != set(ri[q, :10].tolist()):
            assert rs[q, 9] - rs[q, 10] < 1e-6


def test_sharded_search_equals_global(hip):
    """The multi-GPU data path in one process: 3 row shards -> local top-k with global ids -> merge kernel."""
    from arxiv_rag_amd.index import ShardIndex, merge_partials, shard_bounds
    Cm = SO.unit_rows_f16(10001, 256, 5); Q = SO.unit_rows_f16(50, 256, 6)
    qd = torch.from_numpy(Q).cuda()
    parts = []
    for r in range(3):
        lo, hi = shard_bounds(10001, 3, r)
        parts.append(ShardIndex(torch.from_numpy(Cm[lo:hi].copy()).cuda(), idx_base=lo).search(qd, 10))
    ms, mi = merge_partials(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), 10)
    gs, gi = ShardIndex(torch.from_numpy(Cm).cuda()).search(qd, 10)
    assert torch.equal(mi, gi) and torch.equal(ms, gs)
    rs, ri = SO.topk_search(Cm, Q, 10)
    assert (mi.cpu().numpy() == ri).all(axis=1).mean() > 0.95


def test_search_many_two_batches_in_flight_equals_batch_by_batch(hip):
    """`ShardIndex.search_many`: a stream of query batches on two side streams (batch b + 1's pass A under batch b's select / rescore
    tail) returns exactly what `search` returns batch by batch — fp16 and int8 first passes, ragged last batch, results usable on the
    caller's stream right away."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(64 * 700 + 13, 256, 5); Q = SO.unit_rows_f16(9 * 64 + 17, 256, 6)
    qd = torch.from_numpy(Q).cuda()
    batches = [qd[a:a + 64] for a in range(0, len(Q), 64)]
    for pre in (None, "int8"):
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=100, prefilter=pre)
        want = [idx.search(b, 10) for b in batches]
        for _ in range(2):                                                     # second round: the lanes' workspaces are reused
            got = idx.search_many(batches, 10)
            tot = sum(float(s.sum()) for s, _ in got)                          # consumed on the caller's stream, no explicit sync
            assert np.isfinite(tot)
            for (s, i), (ws_, wi_) in zip(got, want):
                assert torch.equal(i, wi_) and torch.equal(s, ws_)
    rs, ri = SO.topk_search(Cm, Q, 10, idx_base=100)
    assert (torch.cat([i for _, i in got]).cpu().numpy() == ri).all(axis=1).mean() > 0.95



def test_search_rows_of_any_norm_stay_exact(hip):
    """the exactness certificate's rounding tolerance used to assume rows of norm <= 1 + 2^-9.  The index now measures
    the shard's largest row norm on the device (`arx_rows_max_norm_f16`) and passes it with every call (`arx_topk_options.max_row_norm`),
    so the answers are the exact top-k of the dot products for rows of norm 0.01 ... 8 — on the fp16 pass, with near-ties planted at
    the scale of the LONG rows' rounding error, where a unit-row tolerance would certify too early."""
    from arxiv_rag_amd.index import ShardIndex
    rs = np.random.RandomState(3)
    d, n = 256, 64 * 500
    Cm = SO.unit_rows_f16(n, d, 31).astype(np.float32)
    norms = np.exp(rs.uniform(np.log(0.01), np.log(8.0), size=n)).astype(np.float32)
    Q = SO.unit_rows_f16(12, d, 32)
    # 40 long rows nearly tied at the top of query 0, spread over 40 different groups: scores ~ 8 x 0.9, equal to ~1e-6 relative
    planted = rs.choice(n // 64, size=40, replace=False) * 64 + rs.randint(0, 64, size=40)
    for j, r in enumerate(planted):
        v = Q[0].astype(np.float32) * 0.9 + 0.02 * rs.standard_normal(d).astype(np.float32)
        Cm[r] = v / np.linalg.norm(v); norms[r] = 8.0
    Cm = (Cm * norms[:, None]).astype(np.float16)
    ct = torch.from_numpy(Cm).cuda()
    idx = ShardIndex(ct, idx_base=5)
    got = float(np.linalg.norm(Cm.astype(np.float32), axis=1).max())
    assert got <= idx.max_row_norm() <= got * 1.001
    for k in (10, 32):
        s, i = idx.search(torch.from_numpy(Q).cuda(), k)
        _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=5, tol=2e-6 * 8.0)
    assert set(i.cpu().numpy()[0].tolist()) <= {int(p) + 5 for p in planted}
    # the int8 first pass (bounds are rigorous whatever the norms) gives the same rows up to exact near-ties
    idx8 = ShardIndex(ct, idx_base=5, prefilter="int8")
    s8, i8 = idx8.search(torch.from_numpy(Q).cuda(), 10)
    _assert_topk_valid(Cm, Q, s8.cpu().numpy(), i8.cpu().numpy(), 10, idx_base=5, tol=2e-6 * 8.0)
    # a caller-given bound is taken at its word; a non-finite shard is refused
    assert ShardIndex(ct, max_row_norm=9.0).max_row_norm() == 9.0
    bad = ct.clone(); bad[77, 3] = float("inf")
    with pytest.raises(hip.ArxError):
        ShardIndex(bad).search(torch.from_numpy(Q).cuda(), 10)
    # rows written later are seen (the bound follows the tensor's version counter, like the int8 copy)
    ct[9] = ct[9] * 0 + 30.0
    assert idx.max_row_norm() >= 30.0 * np.sqrt(d) * 0.999
    # ... and rows written through a raw pointer (the encoder kernels, another library) after `invalidate()`
    from arxiv_rag_amd.index import fill_unit_rows
    lib = hip.load()
    hip.check(lib.arx_fill_unit_rows_f16_at(ct.data_ptr(), 128, d, 5, 0, torch.cuda.current_stream().cuda_stream), "fill")     # rows 0..127 unit again
    ct8 = ct.clone(); i9 = ShardIndex(ct8, prefilter="int8")
    assert i9.max_row_norm() > 8.0                                             # (measured and cached now)
    hip.check(lib.arx_fill_unit_rows_f16_at(ct8.data_ptr(), ct8.shape[0], d, 6, 0, torch.cuda.current_stream().cuda_stream), "fill")
    assert i9.max_row_norm() > 8.0                                             # stale: torch did not see the write
    i9.invalidate()
    assert i9.max_row_norm() < 1.01
    qn = fill_unit_rows(6, d, seed=77)
    s9, id9 = i9.search(qn, 10)
    _assert_topk_valid(ct8.cpu().numpy(), qn.cpu().numpy(), s9.cpu().numpy(), id9.cpu().numpy(), 10, tol=2e-6)


def test_two_indices_with_their_own_policies_from_two_host_threads(hip):
    """no process-wide search state.  Two `ShardIndex` objects over different shards, one with the int8 first pass
    at every batch size, one with `i8_max_queries=0` (never) and the certificate's test hook on every call, are searched from two host
    threads at once, each on its own stream and workspace; each gets ITS answers (bit-equal to a quiet single-threaded run) and ITS
    certificate counters.  A third thread searches the FIRST index concurrently with its own workspace."""
    import threading
    from arxiv_rag_amd.index import ShardIndex
    Ca = torch.from_numpy(SO.unit_rows_f16(64 * 900 + 5, 256, 41)).cuda(); Cb = torch.from_numpy(SO.unit_rows_f16(64 * 700, 256, 42)).cuda()
    Q = torch.from_numpy(SO.unit_rows_f16(96, 256, 43)).cuda()
    ia = ShardIndex(Ca, idx_base=10, prefilter="int8")
    ib = ShardIndex(Cb, idx_base=20, prefilter="int8", i8_max_queries=0)
    wa = ia.search(Q, 10); wb = ib.search(Q, 10, drop_best=1)
    assert ib.certificate_stats()[0] == 96                       # the hook ran for every query of THAT call ...
    ia.search(Q, 10); fa0 = ia.certificate_stats()
    assert fa0[0] <= 1                                           # ... while the int8 index's own call saw no hook
    torch.cuda.synchronize()
    res, errs = {}, []

    def run(tag, idx, kw, own_ws):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                ws = idx.alloc_workspace(96, 10) if own_ws else idx._workspace(96, 10)
                outs = [idx.search(Q, 10, ws=ws, **kw) for _ in range(25)]
                stats = idx.certificate_stats(ws)
            st.synchronize()
            res[tag] = (outs, stats)
        except Exception as e:                                   # noqa: BLE001
            errs.append((tag, repr(e)))
    ts = [threading.Thread(target=run, args=("a", ia, {}, False)), threading.Thread(target=run, args=("b", ib, {"drop_best": 1}, False)),
          threading.Thread(target=run, args=("a2", ia, {}, True))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    for s, i in res["a"][0] + res["a2"][0]:
        assert torch.equal(i, wa[1]) and torch.equal(s, wa[0])
    for s, i in res["b"][0]:
        assert torch.equal(i, wb[1]) and torch.equal(s, wb[0])
    assert res["b"][1][0] == 96 and res["a"][1] == fa0 and res["a2"][1] == fa0


def test_search_many_sees_rows_written_since_the_int8_copy(hip):
    """`search_many` dispatches batches to side streams; the int8 copy (and the norm bound) must be rebuilt from the
    current rows on the CALLER's stream before the first batch is enqueued, or a later batch could read a half-built copy.  A row is
    overwritten to match a query exactly; every batch of the stream must see it (it is in batch 2's and batch 3's queries)."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(64 * 800, 256, 3); Q = SO.unit_rows_f16(4 * 48, 256, 4)
    ct = torch.from_numpy(Cm).cuda(); qd = torch.from_numpy(Q).cuda()
    for tail in (0, 32):
        idx = ShardIndex(ct, prefilter="int8")
        batches = [qd[a:a + 48] for a in range(0, len(Q), 48)]
        idx.search_many(batches, 10, tail_cus=tail)
        row, j = 20000 + tail, (5 if tail == 0 else 9)                         # a different query each round: no tie with the round before
        ct[row] = qd[2 * 48 + j]                                               # in place: bumps the tensor's version
        qd2 = qd.clone(); qd2[3 * 48 + 7] = qd[2 * 48 + j]
        got = idx.search_many([qd2[a:a + 48] for a in range(0, len(Q), 48)], 10, tail_cus=tail)
        assert got[2][1][j, 0].item() == row and got[3][1][7, 0].item() == row
        assert abs(got[2][0][j, 0].item() - 1) < 2e-3
        want = [ShardIndex(ct).search(b, 10) for b in [qd2[a:a + 48] for a in range(0, len(Q), 48)]]
        for b, (g, w) in enumerate(zip(got, want)):
            _assert_same_topk_up_to_ties(ct, qd2[b * 48:(b + 1) * 48], g, w)


def test_search_many_cu_partitioned_streams_equal_batch_by_batch(hip):
    """The pipelined search on two streams with DISJOINT CU masks (scan on 256 - t CUs, tail on t): t in {0 = plain streams, 8, 32, 64},
    fp16 and int8 first passes, 64- and 200-query batches (the 200-query batch takes the persistent pass-A kernel, whose grid is sized
    by the scan stream's CU count): every batch bit-equal to `search`."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(64 * 1200 + 40, 256, 15); Q = SO.unit_rows_f16(7 * 64 + 200, 256, 16)
    qd = torch.from_numpy(Q).cuda()
    batches = [qd[a:a + 64] for a in range(0, 7 * 64, 64)] + [qd[7 * 64:]]
    for pre in (None, "int8"):
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=9, prefilter=pre)
        want = [idx.search(b, 10) for b in batches]
        for tail in (0, 8, 32, 64):
            got = idx.search_many(batches, 10, tail_cus=tail)
            for (s, i), (ws_, wi_) in zip(got, want):
                assert torch.equal(i, wi_) and torch.equal(s, ws_), (pre, tail)
    with pytest.raises(AssertionError):
        idx.search_many(batches, 10, tail_cus=12)


def test_int8_wide_query_tiles_on_a_ragged_shard_row_by_row(hip):
    """an int8 case with 128 < nq <= 1024 and n_rows % 256 != 0 (the persistent pass-A kernel's partial last tile, the
    aux single-row shortcut), every row checked against the fp32 scores of ALL rows."""
    from arxiv_rag_amd.index import ShardIndex
    for n, nq in ((64 * 333 + 37, 200), (256 * 50 + 1, 129), (64 * 401 + 63, 1024)):
        Cm = SO.unit_rows_f16(n, 256, 51); Q = SO.unit_rows_f16(nq, 256, 52)
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=3, prefilter="int8")
        s, i = idx.search(torch.from_numpy(Q).cuda(), 10)
        _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), 10, idx_base=3, tol=2e-6)
        s16, i16 = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=3).search(torch.from_numpy(Q).cuda(), 10)
        _assert_same_topk_up_to_ties(torch.from_numpy(Cm).cuda(), torch.from_numpy(Q).cuda(), (s, i), (s16, i16), idx_base=3)


def test_workspace_sizes_fp16_pass_does_not_pay_for_the_int8_pipeline(hip):
    """`arx_topk_workspace_bytes` is what the fp16 pass needs (no aux words, no candidate lists); the int8 pass asks for
    `arx_topk_workspace_bytes_i8` and refuses the smaller one."""
    from arxiv_rag_amd.index import ShardIndex
    lib = hip.load()
    small, big = lib.arx_topk_workspace_bytes(10_000_000, 1024, 768, 10), lib.arx_topk_workspace_bytes_i8(10_000_000, 1024, 768, 10)
    assert 0 < small < big and big - small > 10_000_000 // 64 * 1024 * 4       # wide fp16 batches reserve no aux words, no candidate lists
    assert lib.arx_topk_workspace_bytes(10_000_000, 64, 768, 10) < lib.arx_topk_workspace_bytes_i8(10_000_000, 64, 768, 10)
    Cm = SO.unit_rows_f16(64 * 300, 256, 1); Q = torch.from_numpy(SO.unit_rows_f16(8, 256, 2)).cuda()
    i16 = ShardIndex(torch.from_numpy(Cm).cuda()); i8 = ShardIndex(torch.from_numpy(Cm).cuda(), prefilter="int8")
    assert i16.workspace_bytes(8, 10) < i8.workspace_bytes(8, 10)
    s, i = i16.search(Q, 10, ws=i16.alloc_workspace(8, 10))
    with pytest.raises(hip.ArxError):
        i8.search(Q, 10, ws=i16.alloc_workspace(8, 10))
    s8, i8r = i8.search(Q, 10)
    assert torch.equal(i, i8r)


def test_clustered_row_generator(hip):
    """`arx_fill_clustered_rows_f16_at` (bench: embedding-like corpus): unit rows, a function of (seed, global row) only (a slice
    generated with row_base equals the slice of the whole), shared centres across row ranges (queries drawn beyond the corpus have
    close neighbours in it), a few hot dimensions carrying most of the energy."""
    from arxiv_rag_amd.index import fill_clustered_rows
    whole = fill_clustered_rows(5000, 256, seed=3, n_clusters=50)
    part = fill_clustered_rows(1000, 256, seed=3, n_clusters=50, row_base=2000)
    assert torch.equal(part, whole[2000:3000])
    nrm = whole.float().norm(dim=1)
    assert (nrm - 1).abs().max() < 2e-3
    q = fill_clustered_rows(64, 256, seed=3, n_clusters=50, row_base=1 << 40)
    best = (q.float() @ whole.float().T).max(dim=1).values
    assert best.min() > 0.7                                        # every query sits in a populated cluster (iid unit rows: ~0.25)
    other = fill_clustered_rows(64, 256, seed=4, n_clusters=50, row_base=1 << 40)
    assert (other.float() @ whole.float().T).max(dim=1).values.mean() < best.mean() - 0.2
    energy = (whole.float() ** 2).mean(dim=0)
    assert (energy > 10 * energy.median()).sum().item() == 3       # default: 3 hot dimensions at gain 6


def test_single_row_tail_equals_full_group_rescoring(hip):
    """Round 4: small fp16 batches (<= 128 queries) take ONE tail kernel that selects inside the block and rescoring only the arg-max row
    of each selected group, expanding a group only when its second-best pass-A score (aux word) reaches the provisional threshold.
    It must return, bit for bit, what the select + rescore kernel pair (all 64 rows of every selected group;
    `flags=ARX_TOPK_NO_SINGLE_ROW_TAIL`) returns — on random rows, ragged shards, tiny shards (fewer rows than k, fewer groups than
    K), k = 10 and 32, several top rows inside ONE group (the group must be expanded), near-tied and all-equal corpora, rows far from
    unit norm — and the oracle's rows."""
    from arxiv_rag_amd.index import ShardIndex
    NO = hip.TOPK_NO_SINGLE_ROW_TAIL
    rs = np.random.RandomState(12)
    cases = [(64 * 700 + 13, 256, 37, 10), (64 * 123 + 1, 128, 128, 32), (5, 128, 3, 10), (700, 384, 1, 10), (64 * 40, 768, 65, 32),
             (256 * 1030 + 255, 128, 64, 10), (64 * 300 + 9, 256, 200, 10), (64 * 90, 384, 256, 32), (64 * 16 * 2100 + 5, 128, 256, 10)]
    for n, d, nq, k in cases:
        Cm = SO.unit_rows_f16(n, d, 100 + n % 7); Q = SO.unit_rows_f16(nq, d, 200 + nq)
        if n > 5000:
            g = 17 * 64                                                        # five of query 0's best rows inside one 64-row group
            for j, r in enumerate((g + 3, g + 9, g + 31, g + 32, g + 63, g + 8, g + 10)):      # g+8..g+10: three of them in ONE 4-row block
                v = Q[0].astype(np.float32) * (0.9 - 0.01 * j) + 0.05 * rs.standard_normal(d).astype(np.float32)
                Cm[r] = (v / np.linalg.norm(v)).astype(np.float16)
        ct, qd = torch.from_numpy(Cm).cuda(), torch.from_numpy(Q).cuda()
        idx = ShardIndex(ct, idx_base=3)
        s, i = idx.search(qd, k)
        f_new = idx.certificate_stats()
        s0, i0 = idx.search(qd, k, flags=NO)
        assert torch.equal(i, i0) and torch.equal(s, s0), (n, d, nq, k)
        assert f_new[0] <= 1
        if n >= k:
            _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=3)
        else:
            assert (i[:, n:] == -1).all() and torch.isinf(s[:, n:]).all() and (i[:, :n] >= 3).all()
        if n > 5000:
            assert {g + 3, g + 9, g + 31, g + 32, g + 63, g + 8, g + 10} <= set((i[0] - 3).tolist())
        for hook in (dict(drop_best=1), dict(tau_mult=1e9)):                  # the certificate's fallback from the new kernel: same answers
            sh, ih = idx.search(qd, k, **hook)
            assert torch.equal(ih, i) and torch.equal(sh, s), (n, hook)
            assert idx.certificate_stats()[0] == (nq if n > 5000 else idx.certificate_stats()[0])    # (a shard of < K groups leaves nothing out)
    Cn, Qn, planted = _near_tied_corpus(60)
    idx = ShardIndex(torch.from_numpy(Cn).cuda(), idx_base=7)
    for k in (10, 32):
        s, i = idx.search(torch.from_numpy(Qn).cuda(), k)
        s0, i0 = idx.search(torch.from_numpy(Qn).cuda(), k, flags=NO)
        assert torch.equal(i, i0) and torch.equal(s, s0)
        _assert_topk_valid(Cn, Qn, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=7)
    Ce = np.tile(SO.unit_rows_f16(1, 128, 1), (64 * 300 + 5, 1)); Qe = SO.unit_rows_f16(4, 128, 2)
    s, i = ShardIndex(torch.from_numpy(Ce).cuda()).search(torch.from_numpy(Qe).cuda(), 10)
    assert np.array_equal(i.cpu().numpy(), np.tile(np.arange(10), (4, 1)))
    # the int8 pipeline's first step takes the same kernel in its COLLECT form (one row per selected group, the select kernel's lists in
    # front of it): same rows as with every selected group rescored in full, narrow and wide query tiles, ragged shards, k = 10 / 32
    for n, d, nq, k in ((64 * 700 + 13, 256, 37, 10), (64 * 333 + 37, 256, 200, 10), (64 * 401 + 63, 128, 1030, 32), (5, 128, 3, 10),
                        (64 * 16 * 1100 + 7, 128, 64, 10)):
        Cm = SO.unit_rows_f16(n, d, 300 + n % 5); Q = SO.unit_rows_f16(nq, d, 400 + nq)
        if n > 5000:
            for j, r in enumerate((17 * 64 + 3, 17 * 64 + 9, 17 * 64 + 31)):
                v = Q[0].astype(np.float32) * (0.9 - 0.01 * j) + 0.05 * rs.standard_normal(d).astype(np.float32)
                Cm[r] = (v / np.linalg.norm(v)).astype(np.float16)
        ct, qd = torch.from_numpy(Cm).cuda(), torch.from_numpy(Q).cuda()
        i8x = ShardIndex(ct, idx_base=3, prefilter="int8")
        s, i = i8x.search(qd, k)
        s0, i0 = i8x.search(qd, k, flags=NO)
        assert torch.equal(i, i0) and torch.equal(s, s0), (n, d, nq, k)
        sd, idd = i8x.search(qd, k, drop_best=1)                              # a forgotten group comes back through the candidate lists
        assert torch.equal(idd, i) and torch.equal(sd, s)
        if n >= k:
            _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=3, tol=2e-6)
    # a shard beyond 2 048 super-groups (the 16-candidates-per-lane instance of the kernel), ragged end
    big = SO.unit_rows_f16(64 * 16 * 2100 + 77, 128, 5); Qb = SO.unit_rows_f16(9, 128, 6)
    idx = ShardIndex(torch.from_numpy(big).cuda())
    s, i = idx.search(torch.from_numpy(Qb).cuda(), 10)
    s0, i0 = idx.search(torch.from_numpy(Qb).cuda(), 10, flags=NO)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    _assert_topk_valid(big, Qb, s.cpu().numpy(), i.cpu().numpy(), 10)


def test_search_topic_ordered_rows_whole_groups_near_tied(hip):
    """The hard layout for group-max selection and for the 4-row tail: TOPIC ORDER (`fill_clustered_rows(n_clusters=-100)`: runs of 100
    consecutive rows share a centre, as the chunks of one paper do), queries = corpus rows + noise.  A query's neighbours fill whole 64-row
    groups with near-tied rows: the selected groups' second bounds reach the threshold and they must be EXPANDED; the int8 bound lets
    whole runs through as (query, group) candidates.  Answers: exact, row by row against fp32 scores of every row — fp16 tail (small
    shard: the 4-row path), the kernel pair (flag), int8, k = 10 and 32, 40 and 200 queries."""
    from arxiv_rag_amd.index import ShardIndex, fill_clustered_rows
    n, d = 64 * 2000 + 17, 256
    ct = fill_clustered_rows(n, d, seed=5, n_clusters=-100)
    assert torch.equal(fill_clustered_rows(1000, d, seed=5, n_clusters=-100, row_base=3000), ct[3000:4000])
    run_cos = (ct[:100].float() @ ct[:100].float().T).mean().item(); far_cos = (ct[:100].float() @ ct[5000:5100].float().T).abs().mean().item()
    assert run_cos > 0.8 and far_cos < 0.2                                    # rows of a run are neighbours, runs are unrelated
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    rows = torch.randint(0, n, (200,), generator=g, device="cuda")
    q = torch.nn.functional.normalize(ct[rows].float() + 0.01 * torch.randn((200, d), generator=g, device="cuda"), dim=1).to(torch.float16)
    Cm, Q = ct.cpu().numpy(), q.cpu().numpy()
    idx, idx8 = ShardIndex(ct, idx_base=2), ShardIndex(ct, idx_base=2, prefilter="int8")
    for nq, k in ((40, 10), (200, 10), (40, 32)):
        s, i = idx.search(q[:nq], k)
        _assert_topk_valid(Cm, Q[:nq], s.cpu().numpy(), i.cpu().numpy(), k, idx_base=2, tol=2e-6)
        assert (i[:, 0] - 2 == rows[:nq]).float().mean() > 0.9                # (a query's own row leads unless a twin in its run beats it)
        s0, i0 = idx.search(q[:nq], k, flags=hip.TOPK_NO_SINGLE_ROW_TAIL)
        _assert_same_topk_up_to_ties(ct, q[:nq], (s, i), (s0, i0), idx_base=2)
        s8, i8 = idx8.search(q[:nq], k)
        _assert_topk_valid(Cm, Q[:nq], s8.cpu().numpy(), i8.cpu().numpy(), k, idx_base=2, tol=2e-6)


def test_more_than_1024_queries_with_a_small_last_pass_on_a_small_shard(hip):
    """Found by tools/search_soak.py (a GPU memory fault): 1 100 queries = internal passes of 1 024 + 76 on a shard small enough for the
    aux-word tail.  The tail choice must follow the CALL's query count (as the workspace layout does): a wide call reserves no aux region,
    so its small last pass must not write one.  fp16 and int8, checked row by row, and the workspace sizing of `search_many` with batches on
    both sides of the 256-query boundary."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(64 * 1500 + 11, 128, 61)
    ct = torch.from_numpy(Cm).cuda()
    for nq in (1100, 1024 + 256, 2048 + 1):
        Q = SO.unit_rows_f16(nq, 128, 62)
        qd = torch.from_numpy(Q).cuda()
        for pre in (None, "int8"):
            idx = ShardIndex(ct, idx_base=5, prefilter=pre)
            s, i = idx.search(qd, 10)
            _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), 10, idx_base=5, tol=2e-6)
            got = idx.search_many([qd[:256], qd[256:513], qd[513:1100]], 10)
            assert torch.equal(torch.cat([x[1] for x in got]), i[:1100]) and torch.equal(torch.cat([x[0] for x in got]), s[:1100])

def test_merge_kernel_exact(hip):
    from arxiv_rag_amd.index import merge_partials
    rs = np.random.RandomState(0)
    P, nq, k = 8, 37, 10
    s = -np.sort(-rs.standard_normal((P, nq, k)).astype(np.float32), axis=2)
    i = rs.randint(0, 10**9, size=(P, nq, k)).astype(np.int64)
    s[3, :, 5:] = -np.inf; i[3, :, 5:] = -1
    s[1, 0, 0] = s[2, 0, 0] = 9.0; i[1, 0, 0] = 500; i[2, 0, 0] = 100
    ms, mi = merge_partials(torch.from_numpy(s).cuda(), torch.from_numpy(i).cuda(), k)
    es, ei = SO.merge_partials(s, i, k)
    assert np.array_equal(mi.cpu().numpy(), ei) and np.array_equal(ms.cpu().numpy(), es)
    assert mi[0, 0].item() == 100 and mi[0, 1].item() == 500


def test_full_size_properties(hip):
    """BASELINE sizes through size-independent properties: (a) one full bench batch (1024 x 256 tokens, mpnet-base):
    unit norms, finite, duplicate chunks give bit-identical rows, permuting the batch permutes the rows;
    (b) BASELINE configs[2] at full size, 10 M x 768 fp16 corpus generated in HBM and 10 000 queries: planted exact
    copies of queries come back as top-1 with score ~1, results sorted, distinct, in range, independent of the query
    batching; sharding the corpus in two and merging gives the identical answer; recall@10 vs the oracle on 8 queries."""
    from arxiv_rag_amd.encoder import HipEncoder
    from arxiv_rag_amd.index import ShardIndex, fill_unit_rows, merge_partials
    cfg = C.MPNET_BASE
    enc = HipEncoder(cfg, seeded_state_dict(cfg, seed=0), max_tokens=1024 * 256, max_seqs=1024)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ids = torch.randint(4, cfg.vocab_size - 1, (1024, 256), generator=g, device="cuda", dtype=torch.int32)
    ids[:, 0] = 0; ids[:, 255] = 2
    ids[513] = ids[7]
    lens = torch.full((1024,), 256, dtype=torch.int32, device="cuda")
    a = enc.forward_tokens(ids, lens, 256, 1024 * 256)
    assert torch.isfinite(a).all() and (a.norm(dim=1) - 1).abs().max() < 1e-5
    assert torch.equal(a[513], a[7])
    perm = torch.randperm(1024, device="cuda")
    b = enc.forward_tokens(ids[perm].contiguous(), lens, 256, 1024 * 256)
    assert torch.equal(b, a[perm])
    enc.close()

    # BASELINE configs[2] at full size: 10 M x 768 fp16 resident (15.36 GB), 10 000 queries
    N, D, NQ = 10_000_000, 768, 10_000
    corpus = fill_unit_rows(N, D, seed=7)
    Q = fill_unit_rows(NQ, D, seed=11)
    rows = torch.arange(300, device="cuda") * 33331 + 13
    corpus[rows] = Q[:300]
    idx = ShardIndex(corpus)
    s, i = idx.search(Q, 10)
    assert torch.equal(i[:300, 0], rows) and (s[:300, 0] - 1).abs().max() < 2e-3
    assert (s[:, :-1] >= s[:, 1:]).all() and (i >= 0).all() and (i < N).all()
    assert (i.sort(dim=1).values[:, 1:] != i.sort(dim=1).values[:, :-1]).all()          # 10 distinct rows per query
    # any query batching gives the same answer (64 / 256 / 1024-wide internal tiles)
    s2, i2 = idx.search(Q[:64], 10); assert torch.equal(i2, i[:64]) and torch.equal(s2, s[:64])
    s3, i3 = idx.search(Q[1000:1256], 10); assert torch.equal(i3, i[1000:1256]) and torch.equal(s3, s[1000:1256])
    # two row shards + merge kernel == one shard
    h = N // 2 + 77
    Qs = Q[:512].contiguous()
    p0 = ShardIndex(corpus[:h], 0).search(Qs, 10); p1 = ShardIndex(corpus[h:], h).search(Qs, 10)
    ms, mi = merge_partials(torch.stack([p0[0], p1[0]]), torch.stack([p0[1], p1[1]]), 10)
    assert torch.equal(mi, i[:512]) and torch.equal(ms, s[:512])
    # recall@10 against the oracle on an 8-query subset over the same fp16 values (blocked numpy over 10 M rows)
    qsub = torch.cat([Q[:4], Q[5000:5004]]).cpu().numpy()
    rs, ri = SO.topk_search(corpus.cpu().numpy(), qsub, 11)
    got = torch.cat([i[:4], i[5000:5004]]).cpu().numpy()
    for q in range(8):
        if set(got[q].tolist()) != set(ri[q, :10].tolist()):
            assert rs[q, 9] - rs[q, 10] < 1e-6


def test_configs3_eight_shards_of_625k_rows_merge_to_the_single_index_answer(hip):
    """BASELINE configs[3]'s data path on ONE GPU (the 8-GPU node is the driver's): the 5 M x 768 corpus cut with `shard_bounds` into
    8 shards of 625 k rows, each generated independently from (seed, GLOBAL row index) as a rank would, searched with its global
    `idx_base`; `merge_partials` of the 8 partial lists must equal ONE 5 M-row index bit for bit, for all 10 000 queries; the int8
    pre-filter on the shards gives the same rows; recall@10 vs the oracle on an 8-query subset."""
    from arxiv_rag_amd.index import ShardIndex, fill_unit_rows, merge_partials, shard_bounds
    N, D, NQ, P = 5_000_000, 768, 10_000, 8
    whole = fill_unit_rows(N, D, seed=7)
    Q = fill_unit_rows(NQ, D, seed=11)
    parts, parts8 = [], []
    for r in range(P):
        lo, hi = shard_bounds(N, P, r)
        assert hi - lo == 625_000
        sh = fill_unit_rows(hi - lo, D, seed=7, row_base=lo)
        assert torch.equal(sh, whole[lo:hi])                                   # a rank's slice IS the corpus's rows
        parts.append(ShardIndex(sh, idx_base=lo).search(Q, 10))
        parts8.append(ShardIndex(sh, idx_base=lo, prefilter="int8").search(Q[:256], 10))
        assert (parts[-1][1] >= lo).all() and (parts[-1][1] < hi).all()
    ms, mi = merge_partials(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), 10)
    gs, gi = ShardIndex(whole).search(Q, 10)
    assert torch.equal(mi, gi) and torch.equal(ms, gs)
    m8s, m8i = merge_partials(torch.stack([p[0] for p in parts8]), torch.stack([p[1] for p in parts8]), 10)
    _assert_same_topk_up_to_ties(whole, Q[:256], (m8s, m8i), (gs[:256], gi[:256]))
    qsub = torch.cat([Q[:4], Q[7000:7004]]).cpu().numpy()
    rs, ri = SO.topk_search(whole.cpu().numpy(), qsub, 11)
    got = torch.cat([mi[:4], mi[7000:7004]]).cpu().numpy()
    for q in range(8):
        if set(got[q].tolist()) != set(ri[q, :10].tolist()):
            assert rs[q, 9] - rs[q, 10] < 1e-6


def test_configs4_rank_slice_6p25m_rows_of_dim_1024(hip):
    """BASELINE configs[4]'s per-rank slice in the precision that is feasible (fp8 inputs miss the 1e-3 bar; the
    bge-large shape runs in bf16): rows [3 N, 4 N) of the 50 M x 1024 corpus = 6.25 M x 1024 fp16 (12.8 GB) resident on one GPU,
    searched at Qb = 1 / 64 / 256: answers independent of the batching, planted copies of queries come back first with their global
    ids, the int8 pre-filter returns the same rows, recall@10 vs the oracle on a 4-query subset."""
    from arxiv_rag_amd.index import ShardIndex, fill_unit_rows
    N, D, base = 6_250_000, 1024, 3 * 6_250_000
    corpus = fill_unit_rows(N, D, seed=7, row_base=base)
    Q = fill_unit_rows(256, D, seed=11)
    rows = torch.arange(32, device="cuda") * 191_113 + 5
    corpus[rows] = Q[:32]
    idx = ShardIndex(corpus, idx_base=base)
    s, i = idx.search(Q, 10)
    assert torch.equal(i[:32, 0], rows + base) and (s[:32, 0] - 1).abs().max() < 2e-3
    assert (s[:, :-1] >= s[:, 1:]).all() and (i >= base).all() and (i < base + N).all()
    s64, i64 = idx.search(Q[:64], 10); assert torch.equal(i64, i[:64]) and torch.equal(s64, s[:64])
    s1, i1 = idx.search(Q[100:101], 10); assert torch.equal(i1, i[100:101]) and torch.equal(s1, s[100:101])
    idx8 = ShardIndex(corpus, idx_base=base, prefilter="int8")
    for a, b in ((0, 64), (100, 101)):
        s8, i8 = idx8.search(Q[a:b], 10)
        _assert_same_topk_up_to_ties(corpus, Q[a:b], (s8, i8), (s[a:b], i[a:b]), idx_base=base)
    del idx8
    rs, ri = SO.topk_search(corpus.cpu().numpy(), Q[40:44].cpu().numpy(), 11, idx_base=base)
    got = i[40:44].cpu().numpy()
    for q in range(4):
        if set(got[q].tolist()) != set(ri[q, :10].tolist()):
            assert rs[q, 9] - rs[q, 10] < 1e-6


def _clustered_rows(n, d, n_clusters, seed, spread=0.35, outlier_dims=3, outlier_gain=6.0):
    """Rows as real sentence embeddings are distributed, not iid: tight clusters around a few hundred centres (a query's neighbours
    all score within the int8 bound's slack of each other) and a few outlier dimensions that carry much more energy than the rest
    (they set max|x|, hence the quantisation scale of every row)."""
    rs = np.random.RandomState(seed)
    gain = np.ones(d, np.float32); gain[rs.choice(d, size=outlier_dims, replace=False)] = outlier_gain
    cen = rs.standard_normal((n_clusters, d)).astype(np.float32) * gain
    x = cen[rs.randint(n_clusters, size=n)] + spread * rs.standard_normal((n, d)).astype(np.float32) * gain
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def test_search_int8_prefilter_on_clustered_anisotropic_rows(hip):
    """the int8 pre-filter's candidate budget was tuned on iid unit rows.  On clustered rows with outlier dimensions the
    bound lets far more groups through: the answers must stay exact (checked row by row against fp32 scores of every row), overflow
    must stay PER QUERY (a query in a 4 000-row cluster overflows alone; queries with ordinary neighbourhoods take the fast
    pipeline), and the adaptive index must switch the pre-filter off when most of a batch overflows."""
    from arxiv_rag_amd.index import ShardIndex
    d, n = 256, 64 * 1500
    Cm = _clustered_rows(n, d, 300, seed=41)
    Q = _clustered_rows(24, d, 300, seed=41)[:24].copy()                      # same centres: every query sits inside a cluster
    for k in (10, 32):
        idx = ShardIndex(torch.from_numpy(Cm).cuda(), idx_base=11, prefilter="int8")
        s, i = idx.search(torch.from_numpy(Q).cuda(), k)
        _assert_topk_valid(Cm, Q, s.cpu().numpy(), i.cpu().numpy(), k, idx_base=11, tol=2e-6)
        flagged, pairs = idx.certificate_stats()
        assert 0 <= flagged <= 24 and pairs <= 24 * 4096
    # one query inside a huge near-duplicate cluster, the rest ordinary: only that query may be flagged
    Cr = SO.unit_rows_f16(64 * 2000, d, 9); Qr = SO.unit_rows_f16(16, d, 10)
    rs = np.random.RandomState(6)
    dup = rs.choice(len(Cr), size=6000, replace=False)
    v = Qr[5].astype(np.float32)
    near = v[None, :] + 0.02 * rs.standard_normal((6000, d)).astype(np.float32)
    Cr[dup] = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(np.float16)
    idx = ShardIndex(torch.from_numpy(Cr).cuda(), prefilter="int8")
    s, i = idx.search(torch.from_numpy(Qr).cuda(), 10)
    _assert_topk_valid(Cr, Qr, s.cpu().numpy(), i.cpu().numpy(), 10, tol=2e-6)
    flagged, _ = idx.certificate_stats()
    assert flagged <= 1, flagged                                              # per-query overflow: the batch's other 15 queries are untouched
    # adaptive policy: a corpus of identical rows overflows every query -> the index falls back to the fp16 pass for good
    Ci = np.tile(SO.unit_rows_f16(1, 128, 1), (64 * 5000, 1)); Qi = SO.unit_rows_f16(8, 128, 2)
    ad = ShardIndex(torch.from_numpy(Ci).cuda(), prefilter="int8", adaptive=True)
    s, i = ad.search(torch.from_numpy(Qi).cuda(), 10)
    assert ad.prefilter_disabled and np.array_equal(i.cpu().numpy(), np.tile(np.arange(10), (8, 1)))
    s2, i2 = ad.search(torch.from_numpy(Qi).cuda(), 10)
    assert torch.equal(i2, i) and torch.equal(s2, s)


def test_int8_index_is_centred_rows_with_a_large_common_component_keep_the_prefilter(hip):
    """Anisotropic embeddings (every row = a shared direction + an individual part; mean pairwise cosine 0.5 ... 0.98 here: models like bge
    at the low end, the encoder's own rows under seeded weights at the high end) are hard for an int8 bound whose slack is proportional to
    the size of the ROW and of the QUERY: rows score within the slack of each other and most groups become candidates.  The index
    quantises rows MINUS the shard's sampled mean (arx_topk_build_i8) and adds q . mean back per query; with ARX_TOPK_I8_CENTRE_QUERY
    (ShardIndex turns it on by itself when |mean|^2 >= 0.25) the query is quantised minus its component along the mean direction too and
    the rank-one term that leaves is added exactly in pass A.  Measured (tools/centred_debug.py, 192 k x 768,
    profiles/r04/int8_centred_index.md), candidate (query, group) pairs per query of the 3 000 groups: cosine 0.74 — 2 850 and EVERY query
    overflowing (un-centred), 610 (rows centred), 110 (both); cosine 0.98 — 2 989 / 2 989 / 130.  Here: answers are the exact rows
    (against the fp16 pass, near-ties by fp32 scores), no query overflows, the candidate lists are as short as on iid rows, the adaptive
    index keeps the pre-filter ON; rows-only centring (centre_query=False) is held to its own, weaker, numbers."""
    from arxiv_rag_amd.index import ShardIndex
    F = torch.nn.functional
    d, n = 768, 64 * 3000 + 17
    g = torch.Generator(device="cuda"); g.manual_seed(77)
    u = torch.randn(d, generator=g, device="cuda"); u /= u.norm()
    for amp, cos_lo, cos_hi in ((0.3, 0.45, 0.55), (0.5, 0.70, 0.78), (2.0, 0.97, 0.985)):
        def rows(m):
            return F.normalize(amp * u[None, :] + 0.3 * F.normalize(torch.randn((m, d), generator=g, device="cuda"), dim=1), dim=1).half()
        C_ = rows(n); Q_ = rows(300)
        cosm = float((C_[:512].float() @ C_[512:1024].float().T).mean().item())
        assert cos_lo < cosm < cos_hi, cosm
        ref = ShardIndex(C_, idx_base=5)
        for nq in (1, 64, 300):
            i8 = ShardIndex(C_, idx_base=5, prefilter="int8", adaptive=True)
            assert i8.centre_query and abs(i8.i8_mean_norm ** 2 - cosm) < 0.03
            a = i8.search(Q_[:nq], 10)
            flagged, pairs = i8.certificate_stats()
            b = ref.search(Q_[:nq], 10)
            _assert_same_topk_up_to_ties(C_, Q_[:nq], a, b, idx_base=5)
            assert not i8.prefilter_disabled and flagged == 0, (amp, nq, flagged)
            assert pairs <= 300 * nq, (amp, nq, pairs)
        if amp <= 0.5:                                            # rows-only centring: still exact, weaker lists
            i8 = ShardIndex(C_, idx_base=5, prefilter="int8", centre_query=False)
            a = i8.search(Q_[:64], 10)
            flagged, pairs = i8.certificate_stats()
            _assert_same_topk_up_to_ties(C_, Q_[:64], a, ref.search(Q_[:64], 10), idx_base=5)
            assert flagged <= 2 and pairs <= 1200 * 64, (amp, flagged, pairs)
    # per-QUERY quantities: a batch mixing on-axis queries, off-axis ones (q . mean ~ 0), the mean direction itself (q' ~ 0: the query has
    # almost no int8 form) and a zero query is answered row for row, 1 100 queries wide (two internal passes, the persistent kernel)
    mhat = F.normalize(C_[:4096].float().mean(0), dim=0)
    mix = torch.cat([Q_[:8], F.normalize(torch.randn((8, d), generator=g, device="cuda"), dim=1).half(), mhat[None, :].half(),
                     (-mhat[None, :]).half(), torch.zeros((1, d), device="cuda").half()])
    for qs in (mix, torch.cat([mix, rows(1100 - len(mix))])):
        i8 = ShardIndex(C_, prefilter="int8")
        assert i8.centre_query
        _assert_same_topk_up_to_ties(C_, qs, i8.search(qs, 10), ShardIndex(C_).search(qs, 10))


def test_int8_bounds_are_upper_bounds_of_every_group(hip):
    """The int8 pass promises, per (query, 64-row group), an UPPER BOUND of the true fp16 score of every row of the group.  Checked directly — not through the final answers, which the certificate would repair — by
    running the scan alone (ARX_TOPK_SCAN_ONLY) and reading the bound array out of the workspace (layout: 256 bytes of counters, then
    [groups][round_up(queries, 64)] floats): every kernel
    form (per-tile 64 / 128 / 256-query tiles, the persistent one), rows with and without a large common component, the query centred or not,
    ragged shard, rows of norm 0.2 ... 3."""
    from arxiv_rag_amd.index import ShardIndex
    from arxiv_rag_amd import _lib
    F = torch.nn.functional
    d, n = 768, 64 * 700 + 29
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    u = F.normalize(torch.randn(d, generator=g, device="cuda"), dim=0)
    for amp in (0.0, 0.6, 2.0):
        base = F.normalize(amp * u[None, :] + 0.3 * F.normalize(torch.randn((n, d), generator=g, device="cuda"), dim=1), dim=1)
        nrm = torch.empty(n, device="cuda").uniform_(0.2, 3.0, generator=g) if amp == 0.6 else torch.ones(n, device="cuda")
        C_ = (base * nrm[:, None]).half()
        Qall = F.normalize(amp * u[None, :] + 0.3 * F.normalize(torch.randn((300, d), generator=g, device="cuda"), dim=1), dim=1).half()
        n_groups = (n + 63) // 64
        for cq in (False, True):
            idx = ShardIndex(C_, prefilter="int8", centre_query=cq)
            for nq in (1, 64, 128, 300):
                Q_ = Qall[:nq]
                ws = idx.alloc_workspace(nq, 10)
                idx.search(Q_, 10, ws=ws, flags=_lib.TOPK_SCAN_ONLY)
                torch.cuda.synchronize()
                ldg = (nq + 63) // 64 * 64
                ub = ws[256:256 + n_groups * ldg * 4].view(torch.float32).view(n_groups, ldg)[:, :nq]
                true = (Q_.float() @ C_.float().T).T                                    # [n, nq]
                true = torch.cat([true, torch.full((n_groups * 64 - n, nq), float("-inf"), device="cuda")]).view(n_groups, 64, nq)
                tmax = true.max(dim=1).values                                             # [groups, nq]
                slack = (ub - tmax)
                assert slack.min().item() >= -1e-7, (amp, cq, nq, slack.min().item())
                # not vacuous: the bound is tight to a few hundredths on average (and far tighter on centred anisotropic rows)
                assert slack.mean().item() < 0.2, (amp, cq, nq, slack.mean().item())
                # the aux word of the same (query, group): high half = an upper bound (bf16 image, rounded up) of every row of the group EXCEPT the one
                # at the position in its low 6 bits — what lets the candidate step read one row of a group.  (Layout, csrc/search.hip topk_layout:
                # counters, bounds, two selection arrays of nsplit x ldg x 36 words, then the aux words in the bounds' shape; 256-byte aligned.)
                r256 = lambda b: (b + 255) // 256 * 256
                n_super = (n_groups + 15) // 16
                nsplit = max(1, min(256, (n_super + 7) // 8))
                off = 256 + r256(n_groups * ldg * 4) + 2 * r256(nsplit * ldg * 36 * 4)
                aux = ws[off:off + n_groups * ldg * 4].view(torch.int32).view(n_groups, ldg)[:, :nq]
                ub2 = (aux & -65536).view(torch.float32)
                arg = (aux & 63).long()                                                   # [groups, nq]
                others = true.clone()
                others.scatter_(1, arg[:, None, :], float("-inf"))
                o2 = others.max(dim=1).values
                fin = torch.isfinite(o2)
                assert (ub2[fin] - o2[fin]).min().item() >= -1e-7, (amp, cq, nq, (ub2[fin] - o2[fin]).min().item())
                # (and it IS the second bound: never above the first by more than its 16-bit rounding)
                assert (ub2 - ub - ub.abs() * 0.008).max().item() <= 1e-6, (amp, cq, nq)


def test_int8_index_follows_writes_to_the_corpus(hip):
    """the int8 copy is a snapshot; rows written afterwards (ShardSink.put, the encoder) must not be searched through
    stale int8 values.  The index notices the tensor's version counter and rebuilds."""
    from arxiv_rag_amd.index import ShardIndex
    Cm = SO.unit_rows_f16(64 * 300, 256, 3); Q = SO.unit_rows_f16(4, 256, 4)
    ct = torch.from_numpy(Cm).cuda()
    idx = ShardIndex(ct, prefilter="int8")
    idx.search(torch.from_numpy(Q).cuda(), 10)
    ct[12345] = torch.from_numpy(Q[2]).cuda()                                 # a row that now matches query 2 exactly
    s, i = idx.search(torch.from_numpy(Q).cuda(), 10)
    assert i[2, 0].item() == 12345 and abs(s[2, 0].item() - 1) < 2e-3


@pytest.mark.parametrize("attn", ["1", "2", "4"])
@pytest.mark.parametrize("preset", ["all-mpnet-base-v2", "all-MiniLM-L6-v2"])
def test_attention_block_forced_rescale(hip, preset, attn):
    need_dev(hip, ATTN_KERNELS[attn])
    """The fused attention kernel alone on crafted q/k/v: (a) ordinary scores, (b) a late key whose score jumps far
    above everything before it (forces the lazy-reference rescale branch, cdna guide rule 26), (c) a first tile of very
    negative scores followed by large ones, (d) ragged lengths incl. 1 and a 33-token row (masked last tile).
    Reference: fp64 softmax attention on the same bf16-rounded inputs, MPNet bias from the oracle's Toeplitz table."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.PRESETS[preset]
    sd = seeded_state_dict(cfg, seed=9, std=0.02)
    enc = HipEncoder(cfg, sd, max_tokens=4096, max_seqs=16, attn_kernel=ATTN_KERNELS[attn])
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    lens = np.array([256, 200, 33, 1, 64, 255, 97], np.int32)
    T = int(lens.sum())
    rs = np.random.RandomState(4)
    qkv = rs.standard_normal((T, 3 * H)).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum(lens)])
    # (b) sequence 0: key 230 aligned with every query of head 0, 40x larger -> score jump >> 8 (log2 units) at tile 7
    qkv[cu[0] + 230, H:H + dh] = 40.0 * np.sign(qkv[cu[0]:cu[1], 0:dh].mean(0) + 1e-3)
    qkv[cu[0]:cu[1], 0:dh] = np.abs(qkv[cu[0]:cu[1], 0:dh]) * np.sign(qkv[cu[0] + 230, H:H + dh])
    # (c) sequence 1, head 1: first 32 keys anti-aligned (very negative scores), later keys strongly aligned
    qh = slice(dh, 2 * dh)
    base = np.sign(rs.standard_normal(dh)).astype(np.float32)
    qkv[cu[1]:cu[2], qh] = base * (1 + 0.1 * rs.rand(200, dh))
    qkv[cu[1]:cu[1] + 32, H + dh:H + 2 * dh] = -30.0 * base
    qkv[cu[1] + 32:cu[2], H + dh:H + 2 * dh] = 6.0 * base * rs.rand(168, 1)
    q16 = torch.from_numpy(qkv).to(torch.bfloat16)
    qd = q16.cuda().contiguous()
    ctx = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device="cuda")
    rc = hip.load().arx_encoder_attention(enc._handle, qd.data_ptr(), torch.from_numpy(lens).cuda().data_ptr(), len(lens), 256,
                                          ctx.data_ptr(), torch.cuda.current_stream().cuda_stream)
    hip.check(rc, "arx_encoder_attention")
    got = ctx.float().cpu().numpy()
    worst = _attention_worst_err(got, q16, lens, cfg, sd)
    assert np.isfinite(got).all()
    assert worst < 2e-2, worst                  # bf16 P and bf16 output; relative to max |v| of the head
    enc.close()


def _attention_worst_err(got, q16, lens, cfg, sd):
    """Asserts |kernel - fp64 softmax attention| <= attention_budget element by element (tests/helpers.py: MPNet bias for the batch's own
    max_len); returns the worst error over all (sequence, head) relative to the head's max |v|."""
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    g = torch.as_tensor(got).cuda().double()
    x = q16.cuda()
    ref, spv, serr = attention_fp64(x, lens, cfg, sd)
    r = ((g - ref).abs() / attention_budget(ref, spv, serr, lens, cfg)).max().item()
    assert r <= 1, ("outside the fp64 budget", r)
    cu = np.concatenate([[0], np.cumsum(lens)])
    v = x[:, 2 * H:].double().abs()
    worst = 0.0
    for b in range(len(lens)):
        L = int(lens[b])
        if L == 0:
            continue
        e = (g - ref)[cu[b]:cu[b + 1]].abs().view(L, nh, dh).amax((0, 2))
        vm = v[cu[b]:cu[b + 1]].view(L, nh, dh).amax((0, 2))
        worst = max(worst, (e / (vm + 1e-9)).max().item())
    return worst


@pytest.mark.parametrize("preset", ["all-mpnet-base-v2", "all-MiniLM-L6-v2"])
def test_attention_optimistic_pass_range_check(hip, preset):
    """attention_tr_kernel first runs softmax against the fixed reference 0 (no running maximum) and keeps the result only if every
    row sum of the wave stayed inside [2^-100, 2^100]; otherwise the wave redoes its queries with the exact running-maximum loop.
    Crafted heads drive every outcome: (a) ordinary scores (accepted), (b) scores around +-60 base-2 units (accepted, far from 1),
    (c) every score of a head below -126 (all P underflow to 0: row sum 0 -> redo), (d) scores above +127 (inf -> redo), (e) a head
    whose row sums reach ~2^110 without any single overflow (finite but outside the accepted range -> redo), (f) one extreme row
    in an otherwise ordinary wave (the whole wave redoes), ragged lengths with a masked last tile.  Against an fp64 softmax."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.PRESETS[preset]
    sd = seeded_state_dict(cfg, seed=9, std=0.02)
    enc = HipEncoder(cfg, sd, max_tokens=4096, max_seqs=16)
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    lens = np.array([256, 250, 131, 256, 77, 33, 1], np.int32)
    T = int(lens.sum())
    cu = np.concatenate([[0], np.cumsum(lens)])
    rs = np.random.RandomState(21)
    qkv = rs.standard_normal((T, 3 * H)).astype(np.float32)
    unit = np.sign(rs.standard_normal(dh)).astype(np.float32)            # +-1 per dim: q.k = c * dh for aligned rows
    ln2 = np.log(2.0)

    def head(b, hd, qscale, kvals):
        """queries of (b, hd) = qscale * unit; key row t = kvals[t] * unit  ->  score (base 2) = qscale * kvals[t] * sqrt(dh) / ln 2"""
        n = lens[b]
        qkv[cu[b]:cu[b] + n, hd * dh:(hd + 1) * dh] = qscale * unit
        qkv[cu[b]:cu[b] + n, H + hd * dh:H + (hd + 1) * dh] = np.asarray(kvals, np.float32)[:n, None] * unit

    s2 = np.sqrt(dh) / ln2                                               # base-2 units per unit of qscale * kval
    head(0, 1, 1.0, np.linspace(-60, 60, 256) / s2)                      # (b) +-60: accepted
    head(0, 2, 1.0, -(200 + 20 * rs.rand(256)) / s2)                     # (c) all below -126: redo
    head(1, 0, 1.0, np.where(np.arange(256) % 7 == 0, 300.0, 5.0) / s2)  # (d) overflow: redo
    head(1, 3, 1.0, np.full(256, 103.0) / s2)                            # (e) 250 keys x 2^103 ~ 2^111: finite, out of range -> redo
    head(2, 2, 1.0, np.linspace(-150, -130, 256) / s2)                   # (c) with a masked last tile (131 keys)
    qkv[cu[3] + 17, 4 * dh:5 * dh] = 400.0 / s2 * unit                   # (f) one extreme query row ...
    qkv[cu[3]:cu[4], H + 4 * dh:H + 5 * dh] = rs.rand(256, 1).astype(np.float32) * unit   # ... against ordinary keys of that head
    q16 = torch.from_numpy(qkv).to(torch.bfloat16)
    qd = q16.cuda().contiguous()
    ctx = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.check(hip.load().arx_encoder_attention(enc._handle, qd.data_ptr(), torch.from_numpy(lens).cuda().data_ptr(), len(lens), 256,
                                               ctx.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_encoder_attention")
    got = ctx.float().cpu().numpy()
    assert np.isfinite(got).all()
    worst = _attention_worst_err(got, q16, lens, cfg, sd)
    assert worst < 2e-2, worst
    enc.close()


@pytest.mark.parametrize("preset", ["all-mpnet-base-v2", "all-MiniLM-L6-v2"])
def test_attention_ring_stream_many_items(hip, preset):
    """The streaming attention kernel with MORE (sequence, head) items than persistent blocks, so that every block's slot
    stream runs through item boundaries, the ring wraps many times and the counted waits see output stores between slot-loads:
    600 ragged sequences (lengths 0, 1, 31..33, 63..65, 127..129, 191..193, 255, 256 and random ones), 200 launches apart from
    one another in nothing but data.  Against the whole-item kernel (same tiles and MFMA order; another softmax reference) and, for
    every (sequence, head), against the fp64 budget."""
    from arxiv_rag_amd.encoder import HipEncoder
    need_dev(hip, ATTN_KERNELS["2"])
    cfg = C.PRESETS[preset]
    sd = seeded_state_dict(cfg, seed=9, std=0.02)
    H = cfg.hidden
    rs = np.random.RandomState(12)
    special = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 0, 2, 250, 130]
    lens = np.array(special + list(rs.randint(0, 257, size=580)), np.int32)
    lens[40] = 256                                            # max_len = 256 whatever the draw
    T = int(lens.sum())
    qkv = (rs.standard_normal((T, 3 * H)) * 1.5).astype(np.float32)
    q16 = torch.from_numpy(qkv).to(torch.bfloat16)
    qd = q16.cuda().contiguous()
    dlens = torch.from_numpy(lens).cuda()
    outs = {}
    for attn in ("1", "2", "4"):
        enc = HipEncoder(cfg, sd, max_tokens=T + 256, max_seqs=len(lens), attn_kernel=ATTN_KERNELS[attn])
        res = []
        for rep in range(3):
            ctx = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device="cuda")
            rc = hip.load().arx_encoder_attention(enc._handle, qd.data_ptr(), dlens.data_ptr(), len(lens), 256, ctx.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
            hip.check(rc, "arx_encoder_attention")
            res.append(ctx)
        torch.cuda.synchronize()
        assert torch.equal(res[0].view(torch.int16), res[1].view(torch.int16)) and torch.equal(res[0].view(torch.int16), res[2].view(torch.int16))
        outs[attn] = res[0].float().cpu().numpy()
        enc.close()
    assert np.isfinite(outs["2"]).all() and np.isfinite(outs["4"]).all()
    scale = np.abs(q16.float().numpy()[:, 2 * H:]).max()
    assert np.abs(outs["2"] - outs["1"]).max() < 1.6e-2 * scale          # one bf16 ulp of the output at most (v1 runs softmax against the
    assert (outs["2"] != outs["1"]).mean() < 0.6                         # fixed reference 0, the streaming kernels against a running maximum)
    assert np.abs(outs["4"] - outs["1"]).max() < 3.2e-2 * scale          # 16-query waves: other MFMA shape, other summation order
    assert (outs["4"] != outs["1"]).mean() < 0.5
    for vv in ("2", "4"):                                                 # every (sequence, head) against fp64
        err = _attention_worst_err(outs[vv], q16, lens, cfg, sd)
        assert err < 2e-2, (vv, err)


def test_collection_query_shape_and_ranking(hip, tmp_path):
    """stage-4 files -> HBM-resident collection -> Chroma-shaped query."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.store import HipCollection
    Cm = SO.unit_rows_f16(3000, 128, 5).astype(np.float32)
    chunks = [{"chunk_id": f"c{i}", "text": f"text {i}", "metadata": {"paper_id": f"p{i % 7}", "section": "s", "quality_score": 0.9}} for i in range(3000)]
    GEN.save_embeddings_to_disk_fallback(chunks, list(Cm), output_dir=str(tmp_path / "saved"))
    col = HipCollection.from_disk(tmp_path / "saved")
    assert col.count() == 3000
    Q = SO.unit_rows_f16(4, 128, 6)
    res = col.query(query_embeddings=Q.astype(np.float32), n_results=10)
    rs, ri = SO.topk_search(Cm.astype(np.float16), Q, 10)
    for qi in range(4):
        assert res["indices"][qi] == ri[qi].tolist()
        assert res["ids"][qi] == [f"c{j}" for j in ri[qi]]
        assert np.allclose(res["distances"][qi], 2 - 2 * rs[qi], atol=1e-5)
        assert res["documents"][qi][0] == f"text {ri[qi][0]}" and res["metadatas"][qi][0]["paper_id"] == f"p{ri[qi][0] % 7}"


@pytest.mark.parametrize("variant", [89, 9, 8, 13])
def test_linear_layer_variants_vs_fp32(hip, variant):
    """arx_gemm_bf16 (the linear layer of the path) against an fp64 matmul on the same bf16-rounded operands:
    every main-loop schedule kept in the tree, every epilogue mode it supports, ragged M/N (masked edge tiles), and K = 192 / 320 / 448:
    an odd number of 64-wide k-tiles (> 1) in the 4-phase loop that pass A of the search shares."""
    lib = hip.load()
    g = torch.Generator(device="cuda"); g.manual_seed(variant)
    st = torch.cuda.current_stream().cuda_stream
    for (M, N, K) in ((230, 192, 64), (517, 64, 128), (1000, 384, 384), (300, 1536, 384), (777, 768, 768), (2048, 2304, 768),
                      (300, 256, 192), (777, 768, 320), (517, 384, 448)):
        A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
        for mode in (0, 1, 2):
            want = A.double() @ W.double().T + b.double()
            if mode == 1:
                want = torch.nn.functional.gelu(want)
            if mode == 2:
                want = want + R.double()
            out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
            hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode,
                                        variant, st), "arx_gemm_bf16")
            pre, perr = gemm_epilogue_fp64(mode, A, W, b, resid=R)      # the per-element budget of tests/helpers.py
            assert (pre - want).abs().max().item() <= 1e-9 * max(1.0, want.abs().max().item())
            err = ((out.double() - want).abs() / gemm_epilogue_budget(pre, perr)).max().item()
            assert err <= 1, (variant, M, N, K, mode, err)


@pytest.mark.parametrize("variant", [8, 9])
def test_gemm_full_line_stores_stay_inside_the_output(hip, variant):
    """Epilogue v3 writes complete 128-B lines: lanes mq and mq ^ 8 exchange 16-B pieces, so a lane stores rows it did not compute (row
    mq + 8 of its block, or mq - 8).  With ragged M the partner's row may not exist, and with N % 256 == 128 half of the last n-tile's waves
    have no columns: nothing may be written past row M (guard rows behind the output keep their pattern) or past column N (it would land
    in the next row: every value is compared), for every row count around the 8- and 16-row boundaries of a row block."""
    lib = hip.load()
    g = torch.Generator(device="cuda"); g.manual_seed(100 + variant)
    st = torch.cuda.current_stream().cuda_stream
    GUARD = 24
    for N, K in ((256, 128), (384, 128), (768, 256)):
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        for M in (1, 7, 8, 9, 15, 17, 121, 129, 136, 255, 257, 263, 264, 391):
            A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
            R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
            for mode in (0, 1, 2):
                buf = torch.full((M + GUARD, N), -7.0, device="cuda", dtype=torch.bfloat16)
                hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), buf.data_ptr(), M, N, K, mode,
                                            variant, st), "arx_gemm_bf16")
                torch.cuda.synchronize()
                assert (buf[M:] == -7.0).all().item(), (variant, M, N, K, mode, "write past row M")
                want, perr = gemm_epilogue_fp64(mode, A, W, b, resid=R)      # float64, with the per-element budget of tests/helpers.py
                err = ((buf[:M].double() - want).abs() / gemm_epilogue_budget(want, perr)).max().item()
                assert err <= 1, (variant, M, N, K, mode, err)


def test_persistent_gemm_bitwise_equals_per_tile_kernel(hip):
    """The persistent form of the 4-phase GEMM (prefetch stream running through tile boundaries, several tiles per block,
    a ragged last tile row) must reproduce the per-tile kernel bit for bit: same k order, same epilogue."""
    lib = hip.load()
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    st = torch.cuda.current_stream().cuda_stream
    for (M, N, K) in ((70001, 768, 768), (33000, 2304, 768), (40000, 768, 3072), (300, 512, 128)):
        A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
        for mode in (0, 1, 2):
            outs = []
            for variant in (8, 9, 9):
                out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
                hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode,
                                            variant, st), "arx_gemm_bf16")
                outs.append(out)
            assert not torch.isnan(outs[0].float()).any()
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), (M, N, K, mode)
            assert torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16)), (M, N, K, mode)
        rows = torch.randint(0, M, (512,), device="cuda", generator=g)
        want = A[rows].float() @ W.float().T + b + R[rows].float()
        assert (outs[2][rows].float() - want).abs().max().item() < 0.02 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("variant", [8, 9])
def test_gemm_counted_wait_schedule_race_screen(hip, variant):
    """The 4-phase kernels order LDS-DMA data by counted vmcnt + barriers only; an early read would show up as rare wrong
    tiles.  Screen: 30 back-to-back launches per shape under memory load (a copy stream running beside them) must all be
    bit-identical to the first, whose sampled rows match an fp32 matmul."""
    lib = hip.load()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    junk_a = torch.empty((1 << 28,), dtype=torch.uint8, device="cuda"); junk_b = torch.empty_like(junk_a)
    for (M, N, K, mode) in ((16384, 768, 768, 2), (8192, 3072, 768, 1), (8192, 768, 3072, 2), (4099, 2304, 768, 0), (1024, 256, 128, 0)):
        A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
        first = None
        for it in range(30):
            with torch.cuda.stream(side):
                junk_b.copy_(junk_a, non_blocking=True)
            out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
            hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode,
                                        variant, st), "arx_gemm_bf16")
            if first is None:
                first = out
                want = A[:512].float() @ W.float().T + b
                want = torch.nn.functional.gelu(want) if mode == 1 else want + R[:512].float() if mode == 2 else want
                assert (out[:512].float() - want).abs().max().item() < 0.02 * max(1.0, want.abs().max().item())
            else:
                assert torch.equal(out.view(torch.int16), first.view(torch.int16)), (variant, M, N, K, mode, it)
        torch.cuda.synchronize()


@pytest.mark.parametrize("opts", [{"ln_fold": False}] + [{"attn_kernel": ATTN_KERNELS[a]} for a in ("0", "1", "2", "4")]
                         + [{"gemm_schedule": g} for g in (13, 8, 9)], ids=[f"env{i}" for i in range(8)])
def test_alternative_schedules_agree(hip, golden_dir, opts):
    """The schedules shipped beside the default (explicit LayerNorm kernels, first attention kernel, 2-stage / per-tile /
    persistent GEMM everywhere) against the same
    golden vectors as the default path, and against the default path itself."""
    from arxiv_rag_amd.encoder import HipEncoder
    need_dev(hip, opts.get("attn_kernel"))
    g = np.load(golden_dir / "full_shapes.npz")
    key, cfg = "all-mpnet-base-v2:w05", C.MPNET_BASE
    seed, std, bstd, jit = g[key + ":wspec"]
    sd = seeded_state_dict(cfg, seed=int(seed), std=std, bias_std=bstd, ln_jitter=jit)
    ids, lens, ref = g[key + ":ids"], g[key + ":lens"], g[key + ":emb"]
    base = HipEncoder(cfg, sd)
    e0 = base.encode_tokens(ids, lens).cpu().numpy()
    base.close()
    alt = HipEncoder(cfg, sd, **opts)
    e1 = alt.encode_tokens(ids, lens).cpu().numpy()
    alt.close()
    assert _cos(e1, ref).min() > 1 - 1e-3
    assert _cos(e1, e0).min() > 1 - 3e-4


def test_small_batch_gemm_vs_fp32_and_tile_kernels(hip):
    """csrc/gemm_small.h alone (arx_gemm_bf16 variant 70): split-K wave tiles + row-wise epilogue, at every (N, K) the encoders use,
    at row counts around its 16-row tile (1, 12, 16, 17, 100, 256), modes bias / bias+GELU / bias+residual, against an fp64 matmul of
    the same bf16 operands and against the 256 x 256-tile kernels (one bf16 ulp: another summation order); K = 192 / 320 / 448:
    odd numbers of 64-wide k-tiles."""
    lib = hip.load()
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    st = torch.cuda.current_stream().cuda_stream
    for (N, K) in ((2304, 768), (768, 768), (3072, 768), (768, 3072), (1152, 384), (384, 384), (1536, 384), (384, 1536),
                   (3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (192, 64), (128, 64), (64, 128), (384, 192), (768, 320), (256, 448)):
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        for M in (1, 12, 16, 17, 100, 256):
            A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
            R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
            for mode in (0, 1, 2):
                outs = []
                for variant in (70, 13):
                    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
                    hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode,
                                                variant, st), "arx_gemm_bf16")
                    outs.append(out.double())
                want = A.double() @ W.double().T + b.double()
                want = torch.nn.functional.gelu(want) if mode == 1 else want + R.double() if mode == 2 else want
                pre, perr = gemm_epilogue_fp64(mode, A, W, b, resid=R)
                bud = gemm_epilogue_budget(pre, perr)               # per element (tests/helpers.py); both kernels inside it: two budgets apart at most
                assert (pre - want).abs().max().item() <= 1e-9 * max(1.0, want.abs().max().item())
                assert ((outs[0] - want).abs() <= bud).all().item(), (N, K, M, mode, ((outs[0] - want).abs() / bud).max().item())
                assert ((outs[1] - want).abs() <= bud).all().item(), (N, K, M, mode, ((outs[1] - want).abs() / bud).max().item())
                assert ((outs[0] - outs[1]).abs() <= 2 * bud).all().item(), (N, K, M, mode)
    # the medium half of the low-latency schedule (variant 71: 128 x 128 tiles) at row counts between its bounds, ragged edges included
    for (N, K) in ((2304, 768), (768, 3072), (1152, 384), (1024, 4096), (192, 64), (384, 192), (768, 320), (256, 448)):
        W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        b = torch.randn((N,), device="cuda", generator=g)
        for M in (257, 1000, 4097):
            A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
            R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
            for mode in (0, 1, 2):
                out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
                hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode, 71, st), "arx_gemm_bf16")
                want = A.double() @ W.double().T + b.double()
                want = torch.nn.functional.gelu(want) if mode == 1 else want + R.double() if mode == 2 else want
                pre, perr = gemm_epilogue_fp64(mode, A, W, b, resid=R)
                assert (pre - want).abs().max().item() <= 1e-9 * max(1.0, want.abs().max().item())
                r71 = ((out.double() - want).abs() / gemm_epilogue_budget(pre, perr)).max().item()
                assert r71 <= 1, (N, K, M, mode, r71)
    N, K, M, mode = 384, 1536, 256, 2
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16); b = torch.randn((N,), device="cuda", generator=g)
    A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16); R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty((M, N), device="cuda", dtype=torch.bfloat16)
    # a second call on the same inputs: bit-repeatable (fixed split order)
    out2 = torch.empty_like(out)
    hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out2.data_ptr(), M, N, K, mode, 70, st), "arx_gemm_bf16")
    hip.check(lib.arx_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), R.data_ptr(), out.data_ptr(), M, N, K, mode, 70, st), "arx_gemm_bf16")
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    with pytest.raises(hip.ArxError):          # beyond its row limit the small-batch path refuses (the forward never sends such a batch there)
        big = torch.zeros((300, K), device="cuda", dtype=torch.bfloat16)
        o = torch.empty((300, N), device="cuda", dtype=torch.bfloat16)
        hip.check(lib.arx_gemm_bf16(big.data_ptr(), W.data_ptr(), b.data_ptr(), o.data_ptr(), o.data_ptr(), 300, N, K, 0, 70, st), "arx_gemm_bf16")


@pytest.mark.parametrize("key,cfg", [("all-mpnet-base-v2:w05", C.MPNET_BASE), ("all-MiniLM-L6-v2:w05", C.MINILM_L6),
                                     ("BAAI_bge-large-en-v1.5:w05", C.BGE_LARGE)])
def test_low_latency_schedule_on_query_batches(hip, golden_dir, key, cfg):
    """`arx_encoder_set_low_latency`: query-sized batches (1, 3, 8 short sequences: <= 256 token rows) through the split-K schedule,
    against the golden vectors (transformers fp32 modules) of the same sequences and against the default schedule of the same handle; a batch above 256 rows with the option ON takes the default kernels and is bit-identical to the option OFF."""
    from arxiv_rag_amd.encoder import HipEncoder
    g = np.load(golden_dir / "full_shapes.npz")
    if key + ":ids" not in g.files:
        pytest.skip(f"{key} not in the fixture")
    seed, std, bstd, jit = g[key + ":wspec"]
    sd = seeded_state_dict(cfg, seed=int(seed), std=std, bias_std=bstd, ln_jitter=jit)
    ids, lens, ref = g[key + ":ids"], g[key + ":lens"], g[key + ":emb"]
    enc = HipEncoder(cfg, sd)
    order = np.argsort(lens)                       # the fixture's shortest sequences first
    differs = False
    for take in (1, 3, 8):
        idx = order[:take]
        while int(lens[idx].sum()) > 256 and len(idx) > 1:
            idx = idx[:-1]
        if int(lens[idx].sum()) > 256:
            continue
        sub_ids = ids[idx][:, :int(lens[idx].max())]
        e_def = enc.encode_tokens(sub_ids, lens[idx]).cpu().numpy()
        e_ll = enc.encode_tokens(sub_ids, lens[idx], low_latency=True).cpu().numpy()
        assert np.isfinite(e_ll).all()
        assert _cos(e_ll, ref[idx]).min() > 1 - 1e-3            # rows do not depend on the batch they are in: the fixture's rows apply
        assert _cos(e_ll, e_def).min() > 1 - 3e-4
        differs |= not np.array_equal(e_ll, e_def)
    assert differs                                  # it IS another schedule (a one-token batch may round to the same bits; not all three)
    # the whole fixture (up to ~1 800 token rows): the medium half of the option, 128 x 128 tiles
    big = enc.encode_tokens(ids, lens).cpu().numpy()
    big_ll = enc.encode_tokens(ids, lens, low_latency=True).cpu().numpy()
    assert _cos(big_ll, ref).min() > 1 - 1e-3 and _cos(big_ll, big).min() > 1 - 3e-4
    # above 8 192 rows the option changes nothing: bit-identical rows
    reps = 8192 // max(int(lens.sum()), 1) + 1
    ids_r, lens_r = np.tile(ids, (reps, 1)), np.tile(lens, reps)
    assert int(lens_r.sum()) > 8192
    huge = enc.encode_tokens(ids_r, lens_r).cpu().numpy()
    huge_ll = enc.encode_tokens(ids_r, lens_r, low_latency=True).cpu().numpy()
    assert np.array_equal(huge, huge_ll)
    enc.close()


@pytest.mark.parametrize("cfg", [C.TINY_MPNET, C.TINY_BERT], ids=["tiny-mpnet", "tiny-bert"])
def test_low_latency_schedule_tiny_configs_vs_oracle(hip, cfg):
    """the small-batch schedule at the smallest shapes (H = 64: one 64-column tile per row, K = 64: two k-steps) on a ragged batch incl.
    1-token and full-length sequences, against the fp32 oracle and the default schedule"""
    from arxiv_rag_amd.encoder import HipEncoder
    sd = seeded_state_dict(cfg, seed=2, std=0.05, bias_std=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(1)
    lens = np.array([64, 40, 17, 5, 1, 33, 64, 2], np.int64)           # 226 token rows
    ids = np.full((len(lens), 64), cfg.pad_id, np.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(4, cfg.vocab_size, size=n)
    ref = EO.encode_tokens(sd, cfg, ids, lens)
    enc = HipEncoder(cfg, sd)
    e_def = enc.encode_tokens(ids, lens).cpu().numpy()
    e_ll = enc.encode_tokens(ids, lens, low_latency=True).cpu().numpy()
    assert _cos(e_ll, ref).min() > 1 - 1e-3
    assert _cos(e_ll, e_def).min() > 1 - 3e-4
    e_ll2 = enc.encode_tokens(ids, lens, low_latency=True).cpu().numpy()
    assert np.array_equal(e_ll, e_ll2)                                   # fixed split order: repeatable bit for bit
    enc.close()


@pytest.mark.parametrize("name,lens", [("all-MiniLM-L6-v2", [512, 400, 300, 257, 511, 33]),
                                       ("all-mpnet-base-v2", [384, 300, 257, 383, 5])])
def test_long_sequences_vs_oracle(hip, name, lens):
    """Sequences beyond 256 tokens (all-mpnet-base-v2 truncates at 384, BERT-style models at 512): attention runs two
    query blocks per (sequence, head) over up to 16 key tiles, LDS holds 512-key K/V; against the fp32 oracle."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.PRESETS[name]
    sd = seeded_state_dict(cfg, seed=8, std=0.04, bias_std=0.02, ln_jitter=0.05)
    rs = np.random.RandomState(3)
    lens = np.array(lens, np.int64)
    S = int(lens.max())
    ids = np.full((len(lens), S), cfg.pad_id, np.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(4, cfg.vocab_size - 1, size=n)
    ref = EO.encode_tokens(sd, cfg, ids, lens)
    enc = HipEncoder(cfg, sd)
    emb = enc.encode_tokens(ids, lens).cpu().numpy()
    assert _cos(emb, ref).min() > 1 - 1e-3
    enc.close()


def test_adjacent_cosine_vs_reference_helper(hip):
    """second client of the encoder: adjacent-sentence cosine, against the reference's
    _cosine_similarity restated in the oracle (text_processor.py:1601-1605)."""
    from arxiv_rag_amd.encoder import adjacent_cosines
    rs = np.random.RandomState(0)
    for n, d in ((1, 384), (2, 384), (57, 384), (300, 768)):
        e = rs.standard_normal((n, d)).astype(np.float32) * rs.uniform(0.1, 3, size=(n, 1)).astype(np.float32)
        got = adjacent_cosines(torch.from_numpy(e).cuda()).cpu().numpy()
        want = np.array([EO.cosine_similarity(e[i], e[i + 1]) for i in range(n - 1)], np.float32)
        assert got.shape == want.shape and (n < 2 or np.abs(got - want).max() < 1e-5)


def test_semantic_chunker_gpu_similarities_give_reference_chunks(hip):
    """fixture embeddings -> arx_adjacent_cosine -> host grouping == the chunks the reference's loop produced."""
    import json
    from pathlib import Path
    from arxiv_rag_amd.encoder import adjacent_cosines
    from arxiv_rag_amd.semantic import group_sentences
    fx = json.loads((Path(__file__).parent / "golden" / "semantic_chunker.json").read_text(encoding="utf-8"))
    for c in fx["cases"]:
        e = torch.tensor(c["embeddings"], dtype=torch.float32, device="cuda")
        sims = adjacent_cosines(e).cpu().numpy()
        assert np.abs(sims - np.array(c["similarities"], np.float32)).max() < 1e-5
        assert group_sentences(c["sentences"], sims, c["max_chunk_size"], c["min_chunk_size"], c["metadata"]) == c["expected_chunks"]


# ------------------------------------------------------------------ text in, files out: the drop-in script on the GPU
def _tiny_text_models():
    from arxiv_rag_amd import config as CFG
    from arxiv_rag_amd.encoder import HipSentenceEncoder
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from arxiv_rag_amd.weights import seeded_state_dict
    from tests.helpers import OracleSentenceModel, synthetic_vocab
    cfg = CFG.TINY_BERT
    sd = seeded_state_dict(cfg, seed=4, std=0.05)
    tok = WordPieceTokenizer.from_vocab(synthetic_vocab(cfg), cfg)
    return cfg, HipSentenceEncoder(cfg, sd, tok), OracleSentenceModel(cfg, sd, tok)


def test_cli_text_to_files_gpu_vs_oracle_model(hip, tmp_path, monkeypatch):
    """Same CLI, same chunk tree, the HIP sentence encoder vs the oracle-backed stand-in: identical metadata/index
    files, embeddings within the parity bar (cosine >= 1 - 1e-3), for both --embedding-workers paths."""
    import json
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    cfg, hipm, orm = _tiny_text_models()
    make_chunk_tree(tmp_path / "in", n_files=6, chunks_per_file=7, seed=2)
    outs = {}
    for tag, model in (("hip", hipm), ("oracle", orm)):
        monkeypatch.chdir(tmp_path)
        (tmp_path / tag).mkdir()
        monkeypatch.chdir(tmp_path / tag)
        rc = GEN.main([str(tmp_path / "in"), "--min-quality", "0.0", "--skip-chroma", "--batch-size", "16"],
                      model_factory=lambda name, m=model: m)
        assert rc == 0
        d = tmp_path / tag / "embeddings_saved"
        outs[tag] = (np.load(d / "embeddings.npy"), (d / "metadata.json").read_bytes(), json.loads((d / "index.json").read_text()))
    eh, mh, ih = outs["hip"]; eo, mo, io_ = outs["oracle"]
    assert mh == mo and ih == io_
    assert eh.dtype == eo.dtype == np.float64 and eh.shape == eo.shape and eh.shape[0] > 0
    assert min(_cos(eh[i], eo[i]) for i in range(len(eh))) >= 1 - 1e-3
    hipm.encoder.close()


def test_cli_fast_path_keeps_the_reference_error_policy(hip, tmp_path, monkeypatch):
    """The dispatcher hands a HIP encoder many quanta per encode() call; when such a call raises, it must fall back to the
    per-quantum worker and end where the reference ends (GEN:155-169): only the offending chunk becomes a zero row, every other
    row is what an undisturbed run produces."""
    import json
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    cfg, hipm, _ = _tiny_text_models()
    make_chunk_tree(tmp_path / "in", n_files=5, chunks_per_file=9, seed=5)
    victim = sorted((tmp_path / "in").rglob("*.json"))[2]
    doc = json.loads(victim.read_text())
    doc["chunks"][4]["text"] = "poison " + doc["chunks"][4]["text"]
    victim.write_text(json.dumps(doc))

    class Poisoned:
        coalesce_batches = True
        def __init__(self, inner): self.inner, self.calls = inner, []
        def get_sentence_embedding_dimension(self): return self.inner.get_sentence_embedding_dimension()
        def encode(self, texts, **kw):
            self.calls.append(len(texts))
            if any(t.startswith("poison") for t in texts):
                raise RuntimeError("injected")
            return self.inner.encode(texts, **kw)

    outs = {}
    for tag, model in (("clean", hipm), ("poisoned", Poisoned(hipm))):
        (tmp_path / tag).mkdir(); monkeypatch.chdir(tmp_path / tag)
        assert GEN.main([str(tmp_path / "in"), "--min-quality", "0.0", "--skip-chroma", "--batch-size", "8", "--chunks-per-worker", "10"],
                        model_factory=lambda name, m=model: m) == 0
        outs[tag] = (np.load(tmp_path / tag / "embeddings_saved" / "embeddings.npy"),
                     json.loads((tmp_path / tag / "embeddings_saved" / "metadata.json").read_text()), model)
    ec, mc, _ = outs["clean"]; ep, mp_, pm = outs["poisoned"]
    assert mc == mp_ and ec.shape == ep.shape
    zero = [i for i in range(len(ep)) if not ep[i].any()]
    assert len(zero) == 1 and mc[zero[0]]["chunk_id"] == doc["chunks"][4].get("chunk_id", mc[zero[0]]["chunk_id"])
    keep = [i for i in range(len(ep)) if i != zero[0]]
    assert np.array_equal(ec[keep], ep[keep])                  # identical rows: batching never changes a row
    assert pm.calls[0] == 45 and 1 in pm.calls                 # one fast call over all quanta first, per-item retries at the end
    hipm.encoder.close()


def test_encode_feeder_slabs_and_device_rows(hip):
    """encode(): the multi-slab feeder path returns the same rows as one slab; encode_device keeps input order."""
    cfg, hipm, orm = _tiny_text_models()
    rs = np.random.RandomState(5)
    words = ["ab", "cd", "graph", "x", "lattice", "qed", "zz"]
    texts = [" ".join(rs.choice(words, size=rs.randint(1, 30))) for _ in range(300)] + [""]
    one = hipm.encode(texts, batch_size=32, normalize_embeddings=True)         # coalesced: one 301-sequence forward
    hipm.coalesce_batches = False
    small = hipm.encode(texts, batch_size=32, normalize_embeddings=True)       # the caller's batches, as given
    hipm.slab_texts = 64; hipm.first_slab_texts = 16
    many = hipm.encode(texts, batch_size=32, normalize_embeddings=True)        # feeder path, several slabs
    assert np.array_equal(one, small) and np.array_equal(one, many)           # rows do not depend on batch composition
    dev = hipm.encode_device(texts, batch_size=32, normalize_embeddings=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), one)
    want = orm.encode(texts, batch_size=32, normalize_embeddings=True)
    assert min(_cos(one[i], want[i]) for i in range(len(texts))) >= 1 - 1e-3
    hipm.encoder.close()


def test_semantic_chunks_end_to_end_vs_oracle_model(hip):
    """sentence split -> HIP encode (un-normalised) -> arx_adjacent_cosine -> grouping, against the same walk fed by
    the oracle model and the reference's numpy cosine; similarities within 2e-3 of the 0.7 threshold are excluded
    from the chunk comparison (bf16 encoder vs fp32 oracle)."""
    from arxiv_rag_amd.semantic import group_sentences, semantic_chunks, split_sentences
    from arxiv_rag_amd.encoder import adjacent_cosines
    cfg, hipm, orm = _tiny_text_models()
    rs = np.random.RandomState(9)
    words = ["graph", "neural", "lattice", "qed", "proof", "of", "the", "bounded", "spectrum", "we", "show"]
    text = " ".join(" ".join(rs.choice(words, size=rs.randint(4, 25))).capitalize() + "." for _ in range(80))
    sents = split_sentences(text)
    eo = orm.encode(sents, normalize_embeddings=False)
    so = np.array([EO.cosine_similarity(eo[i], eo[i - 1]) for i in range(1, len(sents))])
    sh = adjacent_cosines(hipm.encode_device(sents)).cpu().numpy()
    assert np.abs(sh - so).max() < 2e-3
    assert semantic_chunks("Too short.", hipm) is None
    got = semantic_chunks(text, hipm, max_chunk_size=600, min_chunk_size=50, metadata={"paper_id": "p"})
    assert got and all(c["metadata"]["chunk_method"] == "semantic" for c in got)
    if np.abs(so - 0.7).min() > 2e-3:
        assert got == group_sentences(sents, so, 600, 50, {"paper_id": "p"})
    hipm.encoder.close()


def test_semantic_chunks_batch_equals_per_document(hip):
    """One encode + one adjacent-cosine launch over the sentences of many documents gives, per document, exactly what the
    per-document call gives (rows do not depend on batch composition; boundary pairs are ignored)."""
    from arxiv_rag_amd.semantic import semantic_chunks, semantic_chunks_batch
    cfg, hipm, _ = _tiny_text_models()
    rs = np.random.RandomState(21)
    words = ["graph", "neural", "lattice", "qed", "proof", "of", "the", "bounded", "spectrum", "we", "show"]
    docs = []
    for d in range(12):
        n = [0, 1, 2, 7, 30, 55][d % 6]
        docs.append(" ".join(" ".join(rs.choice(words, size=rs.randint(4, 25))).capitalize() + "." for _ in range(n)))
    mds = [{"paper_id": f"p{d}"} if d % 2 else None for d in range(len(docs))]
    got = semantic_chunks_batch(docs, hipm, max_chunk_size=400, min_chunk_size=40, metadatas=mds)
    want = [semantic_chunks(t, hipm, max_chunk_size=400, min_chunk_size=40, metadata=m) for t, m in zip(docs, mds)]
    assert got == want
    assert got[0] is None and got[1] is None and got[4] is not None
    hipm.encoder.close()
