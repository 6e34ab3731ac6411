"""The float64 encoder references of tests/helpers.py (attention_fp64, embed_ln_fp64, layer_fp64, pool_fp64) against the fp32 numpy
oracle (oracle/encoder_oracle.py), on CPU: the GPU module tests/test_gpu_encoder_fp64.py trusts them as its yardstick."""
import dataclasses
import math

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import layer_keys, seeded_state_dict
from oracle import encoder_oracle as EO
from tests.helpers import (ATTN_FAULTS, attention_fp64, embed_ln_fp64, layer_fp64, pool_fp64)

torch = pytest.importorskip("torch")


def _packed(a, lens):
    return np.concatenate([a[b, :n] for b, n in enumerate(lens)], 0)


def _bf16_sd(sd):
    """matrices rounded to bf16 (what HipEncoder uploads): the oracle then computes on the same values as layer_fp64"""
    return {k: (torch.from_numpy(v).to(torch.bfloat16).float().numpy() if v.ndim == 2 and "embeddings" not in k and "relative" not in k
                else v) for k, v in sd.items()}


def _close(got, want, what):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got - want).max() / max(1e-30, np.abs(want).max())
    assert err < 2e-5, (what, err)


@pytest.mark.parametrize("cfg", [dataclasses.replace(C.TINY_MPNET, heads=2), dataclasses.replace(C.TINY_BERT, heads=1)],
                         ids=["mpnet-bias", "bert"])
def test_attention_fp64_matches_the_oracle_softmax(cfg):
    """Up to 300 keys: MPNet buckets beyond the 128-position max_distance; the oracle's [heads, S, S] bias (position_bias) restated."""
    sd = seeded_state_dict(cfg, seed=3, std=0.05)
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    lens = np.array([300, 0, 1, 2, 129, 37], np.int64)
    rs = np.random.RandomState(0)
    qkv = rs.standard_normal((int(lens.sum()), 3 * H)).astype(np.float32)
    ctx, spv, serr = attention_fp64(torch.from_numpy(qkv), lens, cfg, sd)
    S = int(lens.max())
    bias = EO.position_bias(sd, cfg, S)
    cu = np.concatenate([[0], np.cumsum(lens)])
    for b, L in enumerate(lens):
        if L == 0:
            continue
        seg = qkv[cu[b]:cu[b + 1]].reshape(L, 3, nh, dh).transpose(1, 2, 0, 3)
        sc = seg[0] @ seg[1].transpose(0, 2, 1) / np.float32(math.sqrt(dh))
        if bias is not None:
            sc = sc + bias[:, :L, :L]
        p = np.exp(sc - sc.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        want = (p @ seg[2]).transpose(1, 0, 2).reshape(L, H)
        _close(ctx[cu[b]:cu[b + 1]], want, ("ctx", b))
        _close(spv[cu[b]:cu[b + 1]], (p @ np.abs(seg[2])).transpose(1, 0, 2).reshape(L, H), ("spv", b))
    assert (serr > 0).all() and (serr < 1e-3).all()
    for f in ATTN_FAULTS:                                          # every fault is a different operation
        if f.startswith("bias") and bias is None:
            continue
        bad = attention_fp64(torch.from_numpy(qkv), lens, cfg, sd, fault=f)[0]
        assert (bad - ctx).abs().max().item() > 1e-3, f


@pytest.mark.parametrize("cfg", [C.TINY_MPNET, C.TINY_BERT, C.TINY_BERT_CLS], ids=["mpnet", "bert", "bert-cls"])
def test_embed_layer_and_pool_fp64_match_the_oracle(cfg):
    sd = _bf16_sd(seeded_state_dict(cfg, seed=4, std=0.05, bias_std=0.05, ln_jitter=0.1))
    lens = np.array([64, 1, 0, 33, 2], np.int64)
    rs = np.random.RandomState(1)
    ids = np.full((len(lens), 64), cfg.pad_id, np.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = rs.randint(4, cfg.vocab_size, size=n)
    mask = np.arange(64)[None] < lens[:, None]
    add_mask = np.where(mask, np.float32(0), np.finfo(np.float32).min).astype(np.float32)[:, None, None, :]
    x = EO.embeddings(sd, cfg, ids)
    e = embed_ln_fp64(sd, cfg, ids, lens)
    _close(e, _packed(x, lens), "embed")
    bias = EO.position_bias(sd, cfg, 64)
    for i in range(cfg.layers):
        got = layer_fp64(sd, cfg, i, torch.from_numpy(_packed(x, lens)), lens)
        x = EO.encoder_layer(sd, cfg, i, x, add_mask, bias)
        _close(got, _packed(x, lens), ("layer", i))
    pooled, mag = pool_fp64(torch.from_numpy(_packed(x, lens)), lens, cfg)
    want = EO.pool(x, lens, cfg.pool)
    want[lens == 0] = 0
    _close(pooled, want, "pool")
    assert (mag[lens > 0] > 0).all() and (mag[lens == 0] == 0).all()
    # the faults the GPU module shows its budgets would catch are different operations
    assert (embed_ln_fp64(sd, cfg, ids, lens, fault="pos_off_by_one" if cfg.arch == C.ARCH_MPNET else "no_token_type") - e).abs().max() > 0.05
    xp = torch.from_numpy(_packed(x, lens))
    ok = layer_fp64(sd, cfg, 1, xp, lens)
    assert (layer_fp64(sd, cfg, 1, xp, lens, fault="prev_ln") - ok).abs().max() > 0.05
    assert (layer_fp64(sd, cfg, 1, xp, lens, fault="no_oproj_residual") - ok).abs().max() > 0.05
    if cfg.pool == C.POOL_MEAN:
        assert (pool_fp64(xp, lens, cfg, fault="count_pad_row")[0] - pooled).abs().max() > 0.05
