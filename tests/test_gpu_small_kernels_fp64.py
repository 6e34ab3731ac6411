"""The small kernels between the large ones, each against the plain references of tests/small_kernels_fp64.py (checked on CPU by
tests/test_small_kernels_refs.py):
  a. arx_topk_merge over its whole admitted range (n_parts * k <= 4096: candidate slots 0 .. 63 of every lane), bit for bit;
  b. arx_rows_max_norm_f16, the rounded-UP bound the exactness certificate rests on, inside a derived window at dims on and off the
     512-column wave pass and shards beyond the 32 768-row grid cap;
  c. the pooled row: zero-length sequences, the fp16 row against the f32 row, its norm (the search's default max_row_norm), the
     packing offsets of scan_lens_kernel beyond its 256 threads, the id clamp of embed_ln_kernel;
  d. arx_adjacent_cosine against float64 within a derived budget, off the 256-column wave stride, with ld > dim;
  e. arx_f32_to_bf16 on every rounding case, bit for bit.
Budgets and windows are derived (small_kernels_fp64.py), none is measured; the measured ratios are in profiles/small_kernels_fp64.md."""
import dataclasses

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import seeded_state_dict
from tests import small_kernels_fp64 as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ARX_ERR_ARG = -1


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- a. merge ----------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(1, 1), (1, 32), (2, 32), (3, 7), (8, 10), (64, 32), (130, 31), (128, 32), (512, 8), (4096, 1)]
SENT_S, SENT_I = 12345.0, -777


def _merge(hip, s, i, k):
    """arx_topk_merge into sentinel-filled outputs -> (rc, scores, ids)"""
    P, nq = s.shape[:2]
    ds, di = torch.from_numpy(s).cuda(), torch.from_numpy(i).cuda()
    os_ = torch.full((nq, k), SENT_S, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k), SENT_I, dtype=torch.int64, device="cuda")
    rc = hip.load().arx_topk_merge(ds.data_ptr(), di.data_ptr(), P, nq, k, os_.data_ptr(), oi.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, os_.cpu().numpy(), oi.cpu().numpy()


def _assert_merge(hip, s, i, k, what):
    rc, gs, gi = _merge(hip, s, i, k)
    assert rc == 0, (what, hip.load().arx_last_error())
    es, ei = R.merge_ref(s, i, k)
    assert np.array_equal(gi, ei), (what, "ids", np.argwhere(gi != ei)[:4].tolist())
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32)), (what, "score bits")


@pytest.mark.parametrize("P,k", MERGE_SHAPES)
def test_merge_whole_admitted_range(hip, P, k):
    """ragged last blocks (a block serves 4 queries), empty parts and queries, fewer than k valid entries, ties across parts / lanes / slots
    with the lower id in the later part, the answer in the last slot of its lanes: small_kernels_fp64.merge_inputs"""
    for nq in (1, 4, 5, 37):
        s, i = R.merge_inputs(P, k, nq, seed=1000 * P + 10 * k + nq)
        _assert_merge(hip, s, i, k, (P, k, nq))


def test_merge_does_not_need_sorted_lists(hip):
    for P, k in ((130, 31), (8, 10)):
        s, i = R.merge_inputs(P, k, 6, seed=3, sort_lists=False)
        _assert_merge(hip, s, i, k, (P, k, "unsorted"))


@pytest.mark.parametrize("P,k", [(129, 32), (4097, 1)])
def test_merge_refuses_more_than_4096_candidates(hip, P, k):
    s = np.zeros((P, 3, k), np.float32)
    i = np.arange(P * 3 * k, dtype=np.int64).reshape(P, 3, k)
    rc, gs, gi = _merge(hip, s, i, k)
    assert rc == ARX_ERR_ARG
    assert (gs == SENT_S).all() and (gi == SENT_I).all()


# ---- b. max row norm -----------------------------------------------------------------------------------------------------------------
NORM_DIMS = [8, 64, 72, 504, 512, 520, 768, 1032, 8192]
FAMILIES = ("unit", "1e-3", "0.01..8", "+-60000")


def _norm_rows(dim):
    return [1, 5, 300] if dim == 8192 else [1, 3, 4, 5, 32768, 32769, 70001]


def _max_norm(hip, t):
    out = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")          # the result must not depend on what was there
    hip.check(hip.load().arx_rows_max_norm_f16(t.data_ptr(), t.shape[0], t.shape[1], out.data_ptr(), _stream()), "arx_rows_max_norm_f16")
    return float(out.item())


@pytest.mark.parametrize("dim", NORM_DIMS)
def test_max_row_norm_is_a_tight_upper_bound(hip, dim):
    """ref <= got <= ref (1 + 2^-12)(1 + D 2^-24)(1 + 2^-22) (norm_window), per family, per shard size, with the largest row first, last, at
    row 32 768 and at the start of the final partial group of 4.  A shard is pool rows gathered on the device; the reference is numpy's
    float64 norm of those fp16 rows (of the whole shard where it is small)."""
    npool = 61
    pool = R.norm_pool(dim, seed=dim, n=npool)
    pn = R.row_norms_ref(pool)
    dpool = torch.from_numpy(pool).cuda()
    lo_r, hi_r = np.inf, -np.inf
    for n_rows in _norm_rows(dim):
        for fam, fname in enumerate(FAMILIES):
            base = min(fam, 2) * npool                                        # the +-60000 row is planted among rows of norm 0.01..8
            idx = base + (np.arange(n_rows) * 7 + fam) % npool
            shard = dpool[torch.from_numpy(idx).cuda()].contiguous()
            ref = float(pn[np.unique(idx)].max())
            if n_rows * dim <= 1 << 20:
                assert abs(R.max_norm_ref(shard.cpu().numpy()) - ref) <= 1e-15 * ref
            if fam < 3:                                                       # the family's largest row doubled (exact in fp16)
                top = base + int(np.argmax(pn[base:base + npool]))
                planted = (pool[top].astype(np.float32) * 2).astype(np.float16)
            else:
                planted = pool[3 * npool + n_rows % npool]
            pref = R.max_norm_ref(planted[None])
            assert pref > 1.5 * ref
            cases = [(None, ref)] if fam < 3 else []
            cases += [(p, pref) for p in sorted({0, n_rows - 1, 4 * ((n_rows - 1) // 4)} | ({32768} if n_rows > 32768 else set()))]
            drow = torch.from_numpy(planted).cuda()
            for pos, want in cases:
                if pos is not None:
                    keep = shard[pos].clone()
                    shard[pos] = drow
                got = _max_norm(hip, shard)
                if pos is not None:
                    shard[pos] = keep
                lo, hi = R.norm_window(want, dim)
                lo_r, hi_r = min(lo_r, got / want - 1), max(hi_r, got / want - 1)
                assert lo <= got <= hi, (dim, n_rows, fname, pos, got / want - 1, hi / want - 1)
    print(f"max norm D={dim}: got / ref - 1 in [{lo_r:.3e}, {hi_r:.3e}], window [0, {R.norm_window(1.0, dim)[1] - 1:.3e}]")


@pytest.mark.parametrize("dim", NORM_DIMS)
def test_max_row_norm_zero_inf_nan(hip, dim):
    """an all-zero shard gives exactly 0; one +inf component gives +inf, one NaN component gives NaN (the caller refuses such a shard),
    the bad row in the last position, the bad component in the last column"""
    pool = torch.from_numpy(R.norm_pool(dim, seed=dim + 1, n=8)[:8]).cuda()
    for n_rows in ([1, 5, 300] if dim == 8192 else [1, 5, 32769]):
        shard = pool[torch.arange(n_rows, device="cuda") % 8].contiguous()
        assert _max_norm(hip, torch.zeros_like(shard)) == 0.0
        shard[n_rows - 1, dim - 1] = float("inf")
        assert _max_norm(hip, shard) == float("inf"), (dim, n_rows)
        shard[n_rows - 1, dim - 1] = float("nan")
        got = _max_norm(hip, shard)
        assert got != got, (dim, n_rows, got)


# ---- c. pooled rows -------------------------------------------------------------------------------------------------------------------
POOL_CFGS = {"tiny-mpnet-mean": C.TINY_MPNET, "tiny-bert-mean": C.TINY_BERT, "tiny-bert-cls": C.TINY_BERT_CLS}
WIDE_CFGS = {"minilm-384": dataclasses.replace(C.MINILM_L6, layers=2, vocab_size=1000),
             "mpnet-768": dataclasses.replace(C.MPNET_BASE, layers=2, vocab_size=1000),
             "bge-1024": dataclasses.replace(C.BGE_LARGE, layers=2, vocab_size=1000)}
SENT16 = 7.0
PAD16 = 8


def _ids(cfg, lens, seed, width=None):
    rs = np.random.RandomState(seed)
    ids = np.full((len(lens), width or max(int(np.max(lens)), 1)), cfg.pad_id, np.int32)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(4, cfg.vocab_size, size=int(n))
    return ids


def _forward(enc, ids, lens, normalize=True, ll=False, max_len=None):
    """one forward into an f32 [B, H] and an fp16 [B, H + 8] buffer (out16_stride = H + 8, sentinel-filled) -> numpy (f32, fp16)"""
    B, H = len(lens), enc.cfg.hidden
    lens = np.ascontiguousarray(lens, np.int32)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    d_lens = torch.from_numpy(lens).cuda()
    o32 = torch.full((B, H), 9.0, dtype=torch.float32, device="cuda")
    o16 = torch.full((B, H + PAD16), SENT16, dtype=torch.float16, device="cuda")
    enc.forward_tokens(d_ids, d_lens, max_len or max(int(lens.max()), 1), int(lens.sum()), out=o32, out_f16=o16,
                       normalize=bool(normalize), low_latency=ll)
    torch.cuda.synchronize()
    return o32.cpu().numpy(), o16.cpu().numpy()


def _check_f16_rows(o32, o16, lens, normalize, what):
    """the fp16 row is the f32 row rounded, element by element; the padding keeps its sentinel; empty rows are exactly zero in both;
    normalize: every non-empty fp16 row has float64 norm within 2^-9 of 1 (the search's default max_row_norm).  -> worst |norm - 1|"""
    H = o32.shape[1]
    assert np.isfinite(o32).all(), what
    assert np.array_equal(o16[:, :H].view(np.uint16), o32.astype(np.float16).view(np.uint16)), (what, "fp16 row != float16(f32 row)")
    assert (o16[:, H:] == SENT16).all(), (what, "fp16 padding overwritten")
    empty = np.asarray(lens) == 0
    assert (o32[empty] == 0).all() and (o16[empty, :H] == 0).all(), (what, "an empty sequence must pool to zeros")
    if not normalize or empty.all():
        return 0.0
    nrm = np.sqrt((o16[~empty, :H].astype(np.float64) ** 2).sum(1))
    assert (np.abs(nrm - 1) <= 2.0 ** -9).all(), (what, "fp16 row norm", nrm.min(), nrm.max())
    return float(np.abs(nrm - 1).max())


EMPTY_BATCHES = {"first-middle-last": [0, 5, 64, 0, 17, 1, 0], "all-but-one": [0, 0, 9, 0, 0], "over-256-tokens": [64, 0, 64, 64, 0, 64, 64, 30, 0]}


@pytest.mark.parametrize("ll", [False, True], ids=["default", "low-latency"])
@pytest.mark.parametrize("fold", ["1", "0"], ids=["fold", "explicit"])
@pytest.mark.parametrize("name", list(POOL_CFGS))
def test_empty_sequences_and_the_fp16_row(hip, name, fold, ll):
    """Zero-length sequences give exact zeros under every schedule and pooling mode (the LN-fold pool must not return beta), normalised or
    not; the fp16 row a shard receives is the f32 row rounded, of norm <= 1 + 2^-9; and (default schedules) the other rows are the bits
    of the same sequences encoded without the empty ones."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = POOL_CFGS[name]
    sd = seeded_state_dict(cfg, seed=11, std=0.05, bias_std=0.05, ln_jitter=0.1)
    enc = HipEncoder(cfg, sd, ln_fold=(fold == "1"))
    worst = 0.0
    for bname, lens in EMPTY_BATCHES.items():
        lens = np.array(lens, np.int32)
        ids = _ids(cfg, lens, 3)
        full = lens > 0
        for normalize in (1, 0):
            o32, o16 = _forward(enc, ids, lens, normalize, ll)
            worst = max(worst, _check_f16_rows(o32, o16, lens, normalize, (name, fold, ll, bname, normalize)))
            assert (np.abs(o32[full]).max(1) > 0).all()
            if not ll:
                p32, p16 = _forward(enc, ids[full], lens[full], normalize, ll)
                assert np.array_equal(o32[full].view(np.uint32), p32.view(np.uint32)), (name, fold, bname, normalize)
                assert np.array_equal(o16[full].view(np.uint16), p16.view(np.uint16)), (name, fold, bname, normalize)
    enc.close()
    print(f"pooled rows {name} fold={fold} low_latency={ll}: worst |fp16 row norm - 1| = {worst:.3e} (bound 2^-9 = {2.0 ** -9:.3e})")


@pytest.mark.parametrize("name", list(WIDE_CFGS))
def test_full_width_fp16_rows_keep_the_default_row_norm(hip, name):
    """the search's default max_row_norm = 0 stands for rows of norm <= 1 + 2^-9: full-width rows as the encoder writes them"""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = WIDE_CFGS[name]
    sd = seeded_state_dict(cfg, seed=41, std=0.04, bias_std=0.03, ln_jitter=0.1)
    lens = np.array([256, 1, 33, 100, 0, 7], np.int32)
    ids = _ids(cfg, lens, 5)
    enc = HipEncoder(cfg, sd, max_tokens=int(lens.sum()) + 64, max_seqs=len(lens))
    worst = max(_check_f16_rows(*_forward(enc, ids, lens, 1, ll), lens, 1, (name, ll)) for ll in (False, True))
    enc.close()
    print(f"pooled rows {name}: worst |fp16 row norm - 1| = {worst:.3e} (bound 2^-9 = {2.0 ** -9:.3e})")


@pytest.mark.parametrize("n_seqs", [255, 256, 257, 1025, 3001])
def test_packing_offsets_beyond_256_sequences(hip, n_seqs):
    """scan_lens_kernel is one block of 256 threads, each summing ceil(n / 256) lengths: every row of a batch of n sequences (lengths
    0, 1, 2, 3, 7) is the bits of the same sequence encoded inside its own 64-sequence slice; empty rows are zero."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = C.TINY_MPNET
    sd = seeded_state_dict(cfg, seed=12, std=0.05, bias_std=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(n_seqs)
    lens = rs.choice([0, 1, 2, 3, 7], size=n_seqs).astype(np.int32)
    ids = _ids(cfg, lens, 6, width=8)
    enc = HipEncoder(cfg, sd, max_tokens=int(lens.sum()) + 64, max_seqs=n_seqs)
    o32, o16 = _forward(enc, ids, lens, 1, False, max_len=7)
    _check_f16_rows(o32, o16, lens, 1, n_seqs)
    for s0 in range(0, n_seqs, 64):
        sl = slice(s0, s0 + 64)
        assert lens[sl].sum() > 0
        p32, p16 = _forward(enc, ids[sl], lens[sl], 1, False, max_len=7)
        assert np.array_equal(o32[sl].view(np.uint32), p32.view(np.uint32)), (n_seqs, s0, np.flatnonzero((o32[sl] != p32).any(1))[:8].tolist())
        assert np.array_equal(o16[sl].view(np.uint16), p16.view(np.uint16)), (n_seqs, s0)
    enc.close()


@pytest.mark.parametrize("name", ["tiny-mpnet-mean", "tiny-bert-cls"])
def test_out_of_range_ids_are_clamped(hip, name):
    """embed_ln_kernel clamps ids to [0, vocab): -5, vocab_size and 2^31 - 1 inside the valid length give the bits of 0, vocab_size - 1 and
    vocab_size - 1, in the layer-0 tap and in the output"""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = POOL_CFGS[name]
    sd = seeded_state_dict(cfg, seed=13, std=0.05, bias_std=0.05, ln_jitter=0.1)
    lens = np.array([10, 64, 3, 1], np.int32)
    good = _ids(cfg, lens, 8)
    bad = good.copy()
    V = cfg.vocab_size
    for (r, c), (b, g) in zip([(0, 0), (0, 9), (1, 31), (1, 63), (2, 1), (3, 0)],
                              [(-5, 0), (V, V - 1), (2 ** 31 - 1, V - 1), (-5, 0), (V, V - 1), (2 ** 31 - 1, V - 1)]):
        bad[r, c], good[r, c] = b, g
    enc = HipEncoder(cfg, sd)
    t_bad, t_good = enc.tap_hidden(bad, lens, 0), enc.tap_hidden(good, lens, 0)
    assert np.isfinite(t_bad).all() and np.array_equal(t_bad.view(np.uint32), t_good.view(np.uint32))
    e_bad, e_good = _forward(enc, bad, lens)[0], _forward(enc, good, lens)[0]
    assert np.array_equal(e_bad.view(np.uint32), e_good.view(np.uint32))
    other = good.copy(); other[0, 0] = 5 if good[0, 0] != 5 else 6
    assert not np.array_equal(enc.tap_hidden(other, lens, 0), t_good)          # the tap does depend on that id
    enc.close()


# ---- d. adjacent cosine ---------------------------------------------------------------------------------------------------------------
COS_DIMS = [4, 12, 252, 256, 260, 384, 768, 1024, 8192]
COS_SENT = -3.0


def _cosines(hip, e, padded):
    """arx_adjacent_cosine on e [n, D] (numpy f32), contiguous or through a view with ld = D + 4 whose padding columns hold NaN, into a
    sentinel-filled buffer of n - 1 + 4 floats -> numpy [n - 1]"""
    n, D = e.shape
    if padded:
        buf = torch.full((n, D + 4), float("nan"), dtype=torch.float32, device="cuda")
        buf[:, :D] = torch.from_numpy(e).cuda()
        view = buf[:, :D]
    else:
        view = torch.from_numpy(e).cuda()
    ld = view.stride(0) if n > 0 else D + (4 if padded else 0)
    out = torch.full((max(n - 1, 0) + 4,), COS_SENT, dtype=torch.float32, device="cuda")
    hip.check(hip.load().arx_adjacent_cosine(view.data_ptr(), ld, n, D, out.data_ptr(), _stream()), "arx_adjacent_cosine")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[max(n - 1, 0):] == COS_SENT).all(), "a store past the last pair"
    return out[:max(n - 1, 0)]


@pytest.mark.parametrize("dim", COS_DIMS)
def test_adjacent_cosine_vs_fp64(hip, dim):
    """|got - fp64| <= (ceil(D / 256) * 4 + 14) 2^-24 S per pair (cosine_budget): rows of scale 1e-3 .. 1e3, identical and negated pairs,
    a cancelling pair, NaN on both sides of a zero row; ragged last blocks of pairs (a block serves 4)."""
    worst = 0.0
    for n in (0, 1, 2, 5, 6, 1001):
        e = R.cosine_rows(n, dim, seed=dim * 7 + n)
        ref, S = R.cosine_ref(e)
        bud = R.cosine_budget(dim, S)
        for padded in (False, True):
            got = _cosines(hip, e, padded).astype(np.float64)
            assert got.shape == ref.shape
            if n < 2:
                continue
            ok = ~np.isnan(ref)
            assert np.array_equal(np.isnan(got), ~ok), (dim, n, padded, "NaN exactly on both sides of a zero row")
            r = np.abs(got - ref)[ok] / bud[ok]
            worst = max(worst, float(r.max()))
            assert (r <= 1).all(), (dim, n, padded, float(r.max()), int(np.flatnonzero(ok)[r.argmax()]))
        if n == 1001:
            assert np.isnan(ref[499]) and np.isnan(ref[500]) and ok.sum() == 998
            assert abs(ref[1] - 1) < 1e-12 and abs(ref[3] + 1) < 1e-12
    print(f"adjacent cosine D={dim}: worst |got - fp64| / budget = {worst:.3f}")


# ---- e. f32 -> bf16 ---------------------------------------------------------------------------------------------------------------------
BF16_SENT = 0x5A5A


def _to_bf16(hip, bits, offset=0, n=None):
    """arx_f32_to_bf16 on bits[offset : offset + n] into a destination of n + 8 sentinel-filled elements -> uint16 [n]"""
    n = len(bits) - offset if n is None else n
    src = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    dst = torch.full((n + 8,), BF16_SENT, dtype=torch.int16, device="cuda")
    hip.check(hip.load().arx_f32_to_bf16(src.data_ptr() + 4 * offset, dst.data_ptr(), n, _stream()), "arx_f32_to_bf16")
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[n:] == BF16_SENT).all(), "a store past element n"
    return out[:n]


def _assert_bf16(got, bits, what):
    want = R.bf16_rne_ref(bits)
    nan = R.f32_is_nan(bits)
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (what, [(hex(int(bits[j])), hex(int(got[j])), hex(int(want[j]))) for j in bad[:6]])
    assert R.bf16_is_nan(got[nan]).all() and np.array_equal(got[nan] >> 15, (bits[nan] >> 31).astype(np.uint16)), (what, "NaN")


def test_f32_to_bf16_every_rounding_case(hip):
    """bitwise equal to round-to-nearest-even on the integers over every high half x the low halves that decide a rounding (ties on both
    parities, subnormals, +-0, +-inf, the largest finite f32 -> inf) and 2^20 + 3 random patterns; a NaN stays a NaN of its sign"""
    for what, bits in (("exhaustive", R.bf16_exhaustive_bits()), ("random", R.bf16_random_bits())):
        _assert_bf16(_to_bf16(hip, bits), bits, what)
    bits = R.bf16_random_bits(1)
    for n in (0, 1, 255, 256, 257):
        _assert_bf16(_to_bf16(hip, bits, offset=5, n=n), bits[5:5 + n], n)
