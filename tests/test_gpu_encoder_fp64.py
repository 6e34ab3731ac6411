"""The encoder checked against float64 (tests/helpers.py: attention_fp64 / attention_budget, embed_ln_fp64, layer_fp64, pool_fp64), one
operation at a time, so that a local fault cannot hide in an end-to-end cosine:
  - the attention kernels through arx_encoder_attention over every launch shape of launch_attn (csrc/encoder.hip): head dim 32 / 64, with
    and without the MPNet bias, max_len <= 128 (4 waves), 129..256 and 257..512 (8 waves, two query blocks), variants 0 and 1 (2 and 4
    on dev builds), against a per-element budget derived from the kernels' arithmetic;
  - each layer of every schedule (LN-fold default, explicit LayerNorm, the two halves of the low-latency option) fed the kernel's own
    previous tap, the embeddings and the pooled rows;
  - the fused one-pass row statistics against the two-pass LayerNorm kernel as the pre-LN rows' |mean| / spread grows.
Every budget is shown to be tight: the same data under a nearby wrong operation, computed in float64, must break it."""
import dataclasses

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import adversarial_state_dict, seeded_state_dict
from tests.helpers import (ATTN_FAULTS, ATTN_KERNELS, U8, attention_budget, attention_fp64, embed_ln_fp64, layer_fp64, need_dev, pool_fp64)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD_ROWS = 40
GUARD_BITS = 0x7FC1                                   # a NaN with a payload: a stray store of any value changes it


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ---- 1. attention -------------------------------------------------------------------------------------------------------------------
HEADS = {"minilm": C.MINILM_L6, "mpnet": C.MPNET_BASE, "bge-large": C.BGE_LARGE, "tiny-mpnet": C.TINY_MPNET}
# max_len class -> lengths (max first); short and long rows mixed in every batch
LEN_CLASSES = {
    "le128": [128, 0, 1, 2, 31, 32, 33, 127, 64, 100],
    "le256": [256, 1, 129, 255, 2, 0, 33, 200, 128],
    "le512": [512, 1, 257, 383, 384, 385, 511, 2, 31, 129, 256],
}


def _attn_cells():
    cells = []
    for head, cfg in HEADS.items():
        for lc in LEN_CLASSES:
            for attn in ("0", "1", "2", "4"):
                if attn == "2" and lc != "le256":                        # the streaming kernels serve 129..256 only
                    continue
                if attn == "4" and (lc != "le256" or cfg.head_dim != 64):
                    continue
                cells.append((head, lc, attn))
    return cells


def _attn_encoder(hip, cfg, lens, seed, attn):
    """A one-layer handle of the head shape (the attention call reads only its bias table); MPNet bias entries ~ N(0, 1.5^2), the size
    of a trained model's, so that every bucket matters."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg1 = dataclasses.replace(cfg, layers=1, vocab_size=64)
    sd = seeded_state_dict(cfg1, seed=seed, std=0.02)
    if cfg.arch == C.ARCH_MPNET:
        rs = np.random.RandomState(seed + 1)
        sd["encoder.relative_attention_bias.weight"] = (rs.standard_normal((cfg.rel_buckets, cfg.heads)) * 1.5).astype(np.float32)
    enc = HipEncoder(cfg1, sd, max_tokens=int(np.sum(lens)) + 256, max_seqs=len(lens), attn_kernel=ATTN_KERNELS[attn])
    return enc, cfg1, sd


def _spotlight_qkv(cfg, lens, seed):
    """N(0, 1) q / k / v, and in every sequence b one spotlight head (b mod heads): all its queries lean on one direction u, keys 0 and
    len-1 are u scaled so that each takes a probability of about 0.25, and their v rows are +-4 w -- distinctive rows whose weight any
    one-key-too-many / too-few / bias / query-row mistake moves."""
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    rs = np.random.RandomState(seed)
    T = int(np.sum(lens))
    qkv = rs.standard_normal((T, 3 * H)).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum(lens)])
    for b, L in enumerate(lens):
        if L == 0:
            continue
        hd = b % nh
        u = np.sign(rs.standard_normal(dh)).astype(np.float32)
        w = np.sign(rs.standard_normal(dh)).astype(np.float32)
        qs = slice(hd * dh, (hd + 1) * dh)
        ks = slice(H + hd * dh, H + (hd + 1) * dh)
        vs = slice(2 * H + hd * dh, 2 * H + (hd + 1) * dh)
        rows = slice(cu[b], cu[b + 1])
        qkv[rows, qs] = u + 0.3 * rs.standard_normal((L, dh)).astype(np.float32)
        target = np.log(max(1.0, 1.7 * (L - 2) / 2))                     # e^score ~ half the other keys' mass (their e^s averages ~1.7)
        qkv[cu[b], ks] = qkv[cu[b + 1] - 1, ks] = u * np.float32(target / np.sqrt(dh))
        qkv[cu[b], vs] = 4 * w
        qkv[cu[b + 1] - 1, vs] = -4 * w
    return qkv


def _run_attention(hip, enc, q16, lens, max_len):
    """ctx of arx_encoder_attention in a NaN-filled buffer with GUARD_ROWS rows behind row T; returns (ctx [T, H] float64, guard intact)."""
    T, H = q16.shape[0], q16.shape[1] // 3
    buf = torch.full((T + GUARD_ROWS, H), GUARD_BITS, dtype=torch.int16, device="cuda")
    dlens = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    hip.check(hip.load().arx_encoder_attention(enc._handle, q16.data_ptr(), dlens.data_ptr(), len(lens), max_len, buf.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "arx_encoder_attention")
    torch.cuda.synchronize()
    guard_ok = bool((buf[T:] == GUARD_BITS).all().item())
    return buf[:T].view(torch.bfloat16).double(), guard_ok


def check_attention_fp64(got, q16, lens, cfg, sd, what):
    """|got - fp64| <= attention_budget element by element; returns the worst error / budget"""
    ref, spv, serr = attention_fp64(q16, lens, cfg, sd)
    bud = attention_budget(ref, spv, serr, lens, cfg)
    assert torch.isfinite(got).all(), (what, "non-finite output")
    r = ((got - ref).abs() / bud).max().item()
    assert r <= 1, (what, "outside the budget", r)
    return r


def _per_seq_head_ratio(a, ref, bud, lens, cfg):
    """max |a - ref| / budget per (sequence, head) -> [n_seqs, heads] numpy"""
    nh, dh = cfg.heads, cfg.head_dim
    r = ((a - ref).abs() / bud).view(-1, nh, dh).amax(-1)                 # [T, nh]
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = np.zeros((len(lens), nh))
    for b in range(len(lens)):
        if lens[b]:
            out[b] = r[cu[b]:cu[b + 1]].amax(0).cpu().numpy()
    return out


@pytest.mark.parametrize("head,lc,attn", _attn_cells())
def test_attention_fp64_every_launch_shape(hip, head, lc, attn):
    """One cell of the dispatch matrix: worst error inside the budget, finite rows, guard rows untouched; each fault of ATTN_FAULTS
    (bias faults on bias heads) breaks the budget on at least one (sequence, head) of the same data."""
    need_dev(hip, ATTN_KERNELS[attn])
    cfg = HEADS[head]
    lens = np.array(LEN_CLASSES[lc], np.int32)
    seed = 1000 + 17 * list(HEADS).index(head) + list(LEN_CLASSES).index(lc)
    enc, cfg1, sd = _attn_encoder(hip, cfg, lens, seed, attn)
    q16 = torch.from_numpy(_spotlight_qkv(cfg, lens, seed)).to(torch.bfloat16).cuda()
    got, guard_ok = _run_attention(hip, enc, q16, lens, int(lens.max()))
    enc.close()
    assert guard_ok, (head, lc, attn, "a store past row T")
    worst = check_attention_fp64(got, q16, lens, cfg1, sd, (head, lc, attn))
    ref, spv, serr = attention_fp64(q16, lens, cfg1, sd)
    bud = attention_budget(ref, spv, serr, lens, cfg1)
    margins = {}
    for fault in ATTN_FAULTS:
        if fault.startswith("bias") and cfg.arch != C.ARCH_MPNET:
            continue
        bad = attention_fp64(q16, lens, cfg1, sd, fault=fault)[0]
        m = _per_seq_head_ratio(bad, ref, bud, lens, cfg1).max()
        margins[fault] = m
        assert m > 1, (head, lc, attn, fault, "the budget does not see this fault", m)
    print(f"attention {head:10s} {lc} v{attn}: worst/budget {worst:.3f}; smallest fault/budget {min(margins.values()):.1f} "
          + " ".join(f"{k}={v:.1f}" for k, v in margins.items()))


# ---- 2. each layer ------------------------------------------------------------------------------------------------------------------
LAYER_K = 8
# Budget of a tap against layer_fp64 fed the previous tap, per element: 2^-8 |ref| (the tap's own bf16 rounding: bf16 keeps 8 significant
# bits) + LAYER_K 2^-8 rms(ref row).
# The second term covers the layer's other bf16 roundings carried through the LayerNorms: qkv, ctx, the GELU output, the pre-LN sums y1 and
# y2 and the LN1 output (each 2^-8 of an element of up to ~4 row rms, mostly averaged out by the next product); the folded schedule also
# reads bf16(W gamma) and takes its residual LN2(y2) unrounded where the reference reads the rounded tap (one more 2^-8 per element).
EMBED_K = 0.05            # tap 0: fp32 gather + LayerNorm, one bf16 rounding: 2^-8 |ref| + fp32 terms far below 0.05 2^-8 rms
SCHEDULES = {             # HipEncoder options, low_latency, lengths
    "fold": ({}, False, [512, 1, 300, 129, 33, 2, 64]),
    "explicit": ({"ln_fold": False}, False, [512, 1, 300, 129, 33, 2, 64]),
    "ll-splitk": ({}, True, [1, 2, 100, 33, 64, 50]),                # <= 256 rows: split-K GEMMs, statistics in the GEMM epilogue
    "ll-128tiles": ({}, True, [512, 1, 300, 129, 33, 2, 64]),       # 257..8192 rows: 128 x 128 tiles
}
LAYER_CFGS = {"mpnet": dataclasses.replace(C.MPNET_BASE, layers=3), "minilm": dataclasses.replace(C.MINILM_L6, layers=3),
              "bge-large": dataclasses.replace(C.BGE_LARGE, layers=2)}


def _ids(cfg, lens, seed):
    rs = np.random.RandomState(seed)
    ids = np.full((len(lens), max(lens)), cfg.pad_id, np.int32)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(4, cfg.vocab_size, size=n)
    return ids


def _rms(ref):
    return ref.pow(2).mean(-1, keepdim=True).sqrt()


def layer_errors(enc, sd, cfg, ids, lens, low_latency, faults=False):
    """Layer-at-a-time errors of one schedule in units of 2^-8 rms(ref row), beyond the tap's own rounding 2^-8 |ref|:
    -> (per-layer worst [layers + 1] (entry 0: embeddings), taps, {fault: worst / budget})."""
    taps = [torch.from_numpy(enc.tap_hidden(ids, lens, l, low_latency=low_latency)).cuda().double() for l in range(cfg.layers + 1)]
    worst, fault_r = [], {}

    def excess(got, ref):
        return (((got - ref).abs() - U8 * ref.abs()) / (U8 * _rms(ref))).max().item()

    def ratio(bad, ref, k):
        return ((bad - ref).abs() / (U8 * ref.abs() + k * U8 * _rms(ref))).max().item()

    e0 = embed_ln_fp64(sd, cfg, ids, lens, device="cuda")
    worst.append(excess(taps[0], e0))
    if faults:
        f = "pos_off_by_one" if cfg.arch == C.ARCH_MPNET else "no_token_type"
        fault_r[f] = ratio(embed_ln_fp64(sd, cfg, ids, lens, device="cuda", fault=f), e0, EMBED_K)
    for l in range(1, cfg.layers + 1):
        ref = layer_fp64(sd, cfg, l - 1, taps[l - 1], lens)
        worst.append(excess(taps[l], ref))
        if faults and l == cfg.layers:
            for f in ("prev_ln", "no_oproj_residual"):
                fault_r[f] = ratio(layer_fp64(sd, cfg, l - 1, taps[l - 1], lens, fault=f), ref, LAYER_K)
    return worst, taps, fault_r


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(LAYER_CFGS))
def test_each_layer_vs_fp64(hip, name, sched):
    from arxiv_rag_amd.encoder import HipEncoder
    opts, ll, lens = SCHEDULES[sched]
    cfg = LAYER_CFGS[name]
    sd = seeded_state_dict(cfg, seed=31 + list(LAYER_CFGS).index(name), std=0.04, bias_std=0.03, ln_jitter=0.1)
    lens = np.array(lens, np.int32)
    ids = _ids(cfg, lens, 5)
    enc = HipEncoder(cfg, sd, max_tokens=int(lens.sum()) + 64, max_seqs=len(lens), **opts)
    worst, taps, fault_r = layer_errors(enc, sd, cfg, ids, lens, ll, faults=True)
    raw = enc.encode_tokens(ids, lens, normalize=False, low_latency=ll).double()
    unit = enc.encode_tokens(ids, lens, normalize=True, low_latency=ll).double()
    enc.close()
    print(f"layers {name:9s} {sched:11s}: worst error / (2^-8 rms) beyond the tap's rounding, per tap: "
          + " ".join(f"{w:.2f}" for w in worst))
    assert worst[0] <= EMBED_K, (name, sched, "embeddings", worst[0])
    assert max(worst[1:]) <= LAYER_K, (name, sched, "layers", worst)
    # pooled rows: the fold schedule pools LN2(y2) in fp32, from its fused statistics, where the reference pools the rounded tap (2^-8 of
    # each element), plus fp32 sums; half a unit more for the statistics
    pooled, mag = pool_fp64(taps[-1], lens, cfg)
    pbud = 1.5 * U8 * mag + 1e-6 * mag.max()
    pr = ((raw - pooled).abs() / pbud).max().item()
    assert torch.isfinite(raw).all() and pr <= 1, (name, sched, "pooled", pr)
    nrm = raw.norm(dim=1, keepdim=True)
    assert (unit - raw / nrm).abs().max().item() <= 2.0 ** -20, (name, sched, "unit rows are not raw / |raw|")
    if cfg.pool == C.POOL_MEAN:
        bad = pool_fp64(taps[-1], lens, cfg, fault="count_pad_row")[0]
        fault_r["count_pad_row"] = ((bad - pooled).abs() / pbud).max().item()
    print(f"layers {name:9s} {sched:11s}: pooled worst/budget {pr:.3f}; faults/budget "
          + " ".join(f"{k}={v:.1f}" for k, v in fault_r.items()))
    for f, r in fault_r.items():
        assert r > 1, (name, sched, f, "the budget does not see this fault", r)


@pytest.mark.parametrize("name", ["mpnet", "minilm"])
def test_fused_row_statistics_vs_two_pass_layernorm(hip, name):
    """Row-offset sweep on adversarial weights: every pre-LN row offset by 0, 4, 16, 64 (|mean| >> spread at the top).  The LN-fold schedule
    derives each row's mean / rstd from per-64-column partial sums (ln_finalize_kernel; the split-K path in its GEMM epilogue), the explicit
    schedule runs the two-pass layernorm_kernel; both read the same bf16 pre-LN stream, whose rounding costs them alike.  The fold
    schedule's worst layer-at-a-time error must stay within 2x the explicit schedule's plus one bf16 ulp of the row rms, at both batch
    sizes."""
    from arxiv_rag_amd.encoder import HipEncoder
    cfg = dataclasses.replace(C.PRESETS["all-mpnet-base-v2" if name == "mpnet" else "all-MiniLM-L6-v2"], layers=2)
    runs = {"big": np.array([384, 1, 300, 129, 33, 2], np.int32), "small": np.array([1, 2, 100, 33, 64, 50], np.int32)}
    rows = []
    for off in (0.0, 4.0, 16.0, 64.0):
        sd = adversarial_state_dict(cfg, seed=77, row_offset=off)
        res = {}
        for fold in ("1", "0"):
            for size, lens in runs.items():
                enc = HipEncoder(cfg, sd, max_tokens=int(lens.sum()) + 64, max_seqs=len(lens), ln_fold=(fold == "1"))
                ids = _ids(cfg, lens, 9)
                res[fold, size] = max(layer_errors(enc, sd, cfg, ids, lens, low_latency=(fold == "1" and size == "small"))[0][1:])
                enc.close()
        rows.append((off, res))
        print(f"row offset {off:4.0f} {name}: worst error / (2^-8 rms)  fold {res['1', 'big']:.2f} explicit {res['0', 'big']:.2f} | "
              f"split-K fold {res['1', 'small']:.2f} explicit {res['0', 'small']:.2f}")
    for off, res in rows:
        for size in runs:
            assert res["1", size] <= 2 * res["0", size] + 1, (name, off, size, res)
