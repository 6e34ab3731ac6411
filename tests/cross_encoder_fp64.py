"""float64 restatement of a BertForSequenceClassification cross-encoder (test-only): segment-aware embeddings, the encoder layers of
tests/helpers.py (matrices rounded to bf16 as HipEncoder uploads them), the CLS row, pooler tanh and classifier, all in float64.

Each stage takes a `fault=` that restates a nearby wrong operation, so that every budget checked against these references can be
shown tight:
  "type0"     every token takes token-type row 0 (segment B ignored)
  "seg_late"  segment B starts one token late (its first token keeps type 0)
  "no_tanh"   the pooler without its tanh
  "mean_pool" the pooler applied to the mean of the last hidden rows instead of the CLS row
"""
import numpy as np

from tests.helpers import _t64, layer_fp64, layer_norm_fp64

EMBED_FAULTS = ("type0", "seg_late")
HEAD_FAULTS = ("no_tanh", "mean_pool")
FAULTS = EMBED_FAULTS + HEAD_FAULTS


def embed_ln_pairs_fp64(sd, cfg, ids, lens, seg_b, device="cpu", fault=None):
    """ids [B, S], lens [B], seg_b [B] -> packed [sum(lens), H] float64: LN(word[id] + pos[s] + token_type[s >= seg_b])."""
    ids = np.asarray(ids, np.int64)
    lens = np.asarray(lens, np.int64)
    seg = np.asarray(seg_b, np.int64) + (1 if fault == "seg_late" else 0)
    s = np.arange(ids.shape[1])[None]
    keep = s < lens[:, None]
    pos = np.minimum(np.broadcast_to(s, ids.shape), cfg.max_pos - 1)
    typ = (s >= seg[:, None]).astype(np.int64)
    if fault == "type0":
        typ[:] = 0
    ids_c = np.clip(ids, 0, cfg.vocab_size - 1)
    e = (_t64(sd["embeddings.word_embeddings.weight"][ids_c[keep]], device)
         + _t64(sd["embeddings.position_embeddings.weight"][pos[keep]], device)
         + _t64(sd["embeddings.token_type_embeddings.weight"][typ[keep]], device))
    return layer_norm_fp64(e, _t64(sd["embeddings.LayerNorm.weight"], device), _t64(sd["embeddings.LayerNorm.bias"], device), cfg.ln_eps)


def encoder_pairs_fp64(sd, cfg, ids, lens, seg_b, device="cpu", fault=None):
    """-> packed last hidden rows [sum(lens), H] float64 (embedding faults only)."""
    x = embed_ln_pairs_fp64(sd, cfg, ids, lens, seg_b, device=device, fault=fault if fault in EMBED_FAULTS else None)
    for i in range(cfg.layers):
        x = layer_fp64(sd, cfg, i, x, lens)
    return x


def cls_rows(x, lens, fault=None):
    """Packed rows -> [B, H]: the first row of each sequence (fault "mean_pool": the mean of its rows); empty sequences give zeros."""
    import torch
    lens = np.asarray(lens, np.int64)
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = torch.zeros((len(lens), x.shape[1]), dtype=torch.float64, device=x.device)
    for b, L in enumerate(lens):
        if L:
            out[b] = x[cu[b]:cu[b + 1]].mean(0) if fault == "mean_pool" else x[cu[b]]
    return out


def pair_head_fp64(cls, head, fault=None):
    """CLS rows [n, H] -> (logits [n, L], pooled [n, H]) float64; f32 head weights taken as they are (the kernel reads them unrounded)."""
    import torch
    x = _t64(cls)
    dev = x.device
    z = x @ _t64(head["pooler.dense.weight"], dev).T + _t64(head["pooler.dense.bias"], dev)
    p = z if fault == "no_tanh" else torch.tanh(z)
    return p @ _t64(head["classifier.weight"], dev).T + _t64(head["classifier.bias"], dev), p


def score_pairs_fp64(sd, head, cfg, ids, lens, seg_b, device="cpu", fault=None):
    """The whole chain -> (logits [n, L], CLS rows [n, H], pooled [n, H]) float64."""
    x = encoder_pairs_fp64(sd, cfg, ids, lens, seg_b, device=device, fault=fault)
    h = cls_rows(x, lens, fault="mean_pool" if fault == "mean_pool" else None)
    logits, p = pair_head_fp64(h, head, fault="no_tanh" if fault == "no_tanh" else None)
    return logits, h, p


def head_budget(cls, head):
    """Per-logit bound [n, L] on |f32 head - fp64 head| for the kernel's arithmetic (fp32 dots of length H, any summation order: at
    most H 2^-24 of the sum of |terms| each, doubled for the rounding of the partials and the bias; tanh within 4 ulp of its value
    plus 2^-24 absolute; the first stage's error reaches the logits through |W_c| since |tanh'| <= 1):
      e1 = H 2^-23 (|W_p| |h| + |b_p|) + 4 2^-23 |p| + 2^-24
      e2 = |W_c| e1 + H 2^-23 (|W_c| |p| + |b_c|)"""
    import torch
    x = _t64(cls)
    dev = x.device
    H = x.shape[1]
    wp, bp = _t64(head["pooler.dense.weight"], dev), _t64(head["pooler.dense.bias"], dev)
    wc, bc = _t64(head["classifier.weight"], dev), _t64(head["classifier.bias"], dev)
    p = torch.tanh(x @ wp.T + bp)
    u = 2.0 ** -23
    e1 = H * u * (x.abs() @ wp.abs().T + bp.abs()) + 4 * u * p.abs() + 2.0 ** -24
    return e1 @ wc.abs().T + H * u * (p.abs() @ wc.abs().T + bc.abs())


def logit_bar(h_got, h_ref, head):
    """Per-logit bar [n, L] for logits the f32 head computed from the CLS rows `h_got` (read back from the GPU) against the fp64
    chain's `h_ref`: twice the head's response to that CLS error by a Taylor expansion around h_ref — first order signed,
    J = W_c diag(1 - p^2) W_p on the measured difference, plus the second-order remainder (|tanh''| / 2 <= 0.385) — plus
    `head_budget` for the f32 head itself.  It follows the encoder's real error, so it goes with the encoders' CLS cosine bar
    (1 - 1e-3); it is tight for the head: a missing tanh or a pooler fed the mean row breaks it."""
    g, r = _t64(h_got), _t64(h_ref)
    dev = r.device
    wp, wc = _t64(head["pooler.dense.weight"], dev), _t64(head["classifier.weight"], dev)
    _, p = pair_head_fp64(r, head)
    dh = g - r
    lin = ((dh @ wp.T) * (1 - p * p)) @ wc.T
    second = 0.385 * (dh.abs() @ wp.abs().T) ** 2 @ wc.abs().T
    return 2 * (lin.abs() + second) + head_budget(g, head)


def bf16_round_matrices(sd):
    """Encoder matrices rounded to bf16 (and back to f32) the way HipEncoder uploads them; vectors and embeddings unchanged."""
    import torch
    out = {}
    for k, v in sd.items():
        if v.ndim == 2 and k.startswith("encoder.layer."):
            out[k] = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).float().numpy()
        else:
            out[k] = v
    return out


def seeded_cross_weights(cfg, n_labels, seed):
    """The fixture's weights from (cfg, n_labels, seed): seeded encoder (LayerNorm jitter), token-type rows of std 0.5 so that segment B
    matters, seeded head; encoder matrices rounded to bf16 (what the GPU multiplies).  -> (encoder state dict, head state dict)."""
    from arxiv_rag_amd.weights import seeded_pair_head, seeded_state_dict
    sd = seeded_state_dict(cfg, seed=seed, std=0.08, bias_std=0.05, ln_jitter=0.1)
    sd["embeddings.token_type_embeddings.weight"] = (np.random.RandomState(seed + 1).standard_normal((2, cfg.hidden)) * 0.5).astype(np.float32)
    return bf16_round_matrices(sd), seeded_pair_head(cfg, n_labels, seed=seed + 2, std=0.2)


def weights_digest(sd, head):
    import hashlib
    h = hashlib.sha256()
    for d in (sd, head):
        for k in d:
            h.update(k.encode()); h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.digest()


def golden_weights(g, name, cfg, n_labels):
    """Regenerate a tiny-cross-encoder.npz entry's weights from its stored seed and check them bit for bit against its sha256."""
    sd, head = seeded_cross_weights(cfg, n_labels, int(g[f"{name}:seed"]))
    assert weights_digest(sd, head) == bytes(g[f"{name}:wdigest"]), "the fixture's weights do not regenerate from its seed"
    return sd, head
