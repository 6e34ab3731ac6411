"""Test-only helpers: an oracle-backed stand-in for the encoder so that the host logic (CLI, loader,
writer, order contract, fallbacks, multi-rank sharding) can be exercised on CPU.  Never imported by
the product package."""
import hashlib
import json
import numpy as np
import pytest

from arxiv_rag_amd import _lib
from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import seeded_state_dict
from oracle import encoder_oracle as EO

# the attention kernels under the labels the parametrised tests carry in their ids -> `HipEncoder(attn_kernel=...)`
ATTN_KERNELS = {"0": _lib.ATTN_STAGED, "1": _lib.ATTN_TRANSPOSED, "2": _lib.ATTN_RING, "4": _lib.ATTN_RING16}


def need_dev(hip, attn_kernel):
    if attn_kernel in (_lib.ATTN_RING, _lib.ATTN_RING16) and not (hip.load().arx_build_info() & 1):
        pytest.skip("streaming attention kernels are compiled only with ARX_HIPCC_EXTRA=-DARX_DEV_VARIANTS (csrc/build.sh)")


def tiny_weights(g, cfg):
    """The weights of a tiny golden fixture: stored as `w:<name>` arrays, or (tiny-bert-cls) regenerated from the stored
    `wspec` = (seed, std, bias_std, ln_jitter) and checked bit for bit against the stored sha256 `wdigest`."""
    if "wspec" not in g.files:
        return {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    seed, std, bstd, jit = g["wspec"]
    sd = seeded_state_dict(cfg, seed=int(seed), std=std, bias_std=bstd, ln_jitter=jit)
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode()); h.update(np.ascontiguousarray(sd[k]).tobytes())
    assert h.digest() == bytes(g["wdigest"]), "the fixture's weights do not regenerate from its seed"
    return sd


def synthetic_vocab(cfg, n_words=90):
    """specials + single characters + seeded pseudo-words/continuations; len == cfg.vocab_size."""
    rs = np.random.RandomState(7)
    if cfg.arch == C.ARCH_MPNET:
        toks = ["<s>", "<pad>", "</s>", "<unk>"]
    else:
        toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]
    letters = "abcdefghijklmnopqrstuvwxyz"
    toks += list(letters) + ["##" + c for c in letters] + list(".,;!?-()")
    seen = set(toks)
    while len(toks) < cfg.vocab_size:
        w = "".join(rs.choice(list(letters), size=rs.randint(2, 6)))
        w = w if rs.rand() < 0.6 else "##" + w
        if w not in seen:
            seen.add(w); toks.append(w)
    return {t: i for i, t in enumerate(toks)}


class OracleSentenceModel:
    """Same two methods as SentenceTransformer / HipSentenceEncoder, arithmetic by the numpy oracle."""

    def __init__(self, cfg, sd, tokenizer, fail_on=None):
        self.cfg, self.sd, self.tokenizer, self.fail_on = cfg, sd, tokenizer, fail_on or (lambda texts: False)
        self.calls = []

    def get_sentence_embedding_dimension(self):
        return self.cfg.hidden

    def encode(self, sentences, batch_size=32, normalize_embeddings=False, **kw):
        self.calls.append(len(sentences))
        if self.fail_on(sentences):
            raise RuntimeError("injected failure")
        seqs = self.tokenizer.encode_batch(list(sentences), self.cfg.max_seq_length)
        return EO.encode_ragged(self.sd, self.cfg, seqs, batch_size=batch_size, normalize=normalize_embeddings)


def make_chunk_tree(root, n_files=12, chunks_per_file=5, seed=0, words=None):
    """Synthetic stage-3 output: chunk JSON files with the schema of pipeline.py:369-387 + quality_score."""
    rs = np.random.RandomState(seed)
    words = words or ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa"]
    root.mkdir(parents=True, exist_ok=True)
    all_chunks = []
    for f in range(n_files):
        pid = f"0704.{f:04d}"
        chunks = []
        for c in range(chunks_per_file):
            text = " ".join(rs.choice(words, size=rs.randint(3, 40)))
            chunks.append({"chunk_id": f"{pid}_chunk_{c}", "text": text,
                           "metadata": {"quality_score": float(np.round(rs.uniform(0.8, 1.0), 3)), "paper_id": pid,
                                        "section": rs.choice(["Introduction", "Methods", "Results"]).item(), "chunk_index": c}})
        sub = root / ("a" if f % 2 else "b")
        sub.mkdir(exist_ok=True)
        (sub / f"{pid}.json").write_text(json.dumps({"paper_id": pid, "chunks": chunks}))
        all_chunks.extend(chunks)
    return all_chunks


# ---- exact top-k search checked against float64 -------------------------------------------------------------------------------------
# The certificate's tolerance (csrc/search.hip topk_search_impl, tau_scale) is the sum of two per-pass rounding budgets, both relative to
# |q|_2 |c|_2 >= sum |q_i c_i| (csrc/search_tail.h, rescore_kernel step 5), with u = 2^-24:
#   pass A (f16 MFMA, f32 accumulation; "8 roundings per 32-deep MFMA step"):                  A(D) = 0.25 D u
#   pass B (exact_row_score: f32 FMA chains of D/16 terms, their sum and a 3-step butterfly):  B(D) = (D/16 + 4) u
# tau = (A(D) + B(D)) |q| max|c| = (0.3125 D + 4) u |q| max|c|.
U24 = 2.0 ** -24


def pass_a_budget(dim):
    """A(D): |pass-A score - q.c| <= A(D) |q| |c| for every (query, row)."""
    return 0.25 * dim * U24


def pass_b_budget(dim):
    """B(D): |pass-B score - q.c| <= B(D) |q| |c| for every (query, row)."""
    return (dim / 16 + 4) * U24


def scores_fp64(q, c):
    """[nq, n] float64 dot products of the fp16 values (device tensors in, device tensor out), in row chunks whose product stays at or
    below 2^28 elements: torch's matmul on this stack has written zeros past element 2^29 of a larger result (tools/search_soak.py)."""
    import torch
    q64 = q.double()
    step = min(ROW_CHUNK, max(1, (1 << 28) // max(1, q.shape[0])))               # (and never the float64 copy of a whole multi-GB shard)
    return torch.cat([q64 @ c[a:a + step].double().T for a in range(0, c.shape[0], step)], dim=1)


ROW_CHUNK = 1 << 18


def row_norms_fp64(c):
    """[n] float64 L2 norms of the fp16 rows `c`, converted ROW_CHUNK rows at a time"""
    import torch
    return torch.cat([c[a:a + ROW_CHUNK].double().norm(dim=1) for a in range(0, max(1, c.shape[0]), ROW_CHUNK)])


def check_topk_fp64(c, q, s, i, k, idx_base=0, e=None, sample_rows=4, what=None):
    """Assert that (s, i) = search(q, k) over the fp16 rows `c` (device tensors) is an exact top-k by the certificate's own arithmetic.
    e = q.c in float64 (scores_fp64; a few rows cross-checked against numpy float64 on the host).  Per query:
      - ids are distinct and inside [idx_base, idx_base + n); the (-inf, -1) padding appears exactly when k > n;
      - pass B: every returned score s_j satisfies |s_j - e(q, id_j)| <= B(D) |q| |c_j|;
      - completeness: the answer is the top-k of the pass-B scores (the certificate's claim), so a row r left out has
        s_r <= min_j s_j, hence e_r - B(D) |q| |c_r| <= min_j (e_j + B(D) |q| |c_j|)   (<= min_j e_j + 2 B(D) |q| max|c|);
      - scores are non-increasing, and rows whose reported scores are bit-equal come in ascending id order.
    Returns e."""
    import torch
    n, D = c.shape
    nq = q.shape[0]
    if e is None:
        e = scores_fp64(q, c)
    if sample_rows:                                              # the device's float64 product against numpy's, on sampled queries and rows
        rows = torch.linspace(0, nq - 1, min(nq, sample_rows)).long()
        cols = torch.linspace(0, n - 1, min(n, 2048)).long()
        ref = q[rows].cpu().numpy().astype(np.float64) @ c[cols.to(c.device)].cpu().numpy().astype(np.float64).T
        got = e[rows][:, cols.to(e.device)].cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-13 * max(1e-30, float(np.abs(ref).max())), (what, "float64 matmul")
    B = pass_b_budget(D)
    qn = q.double().norm(dim=1)                                                  # [nq]
    cn = row_norms_fp64(c)                                                       # [n]
    kk = min(k, n)
    assert s.shape == (nq, k) and i.shape == (nq, k), what
    if k > n:
        assert (i[:, n:] == -1).all() and torch.isinf(s[:, n:]).all() and (s[:, n:] < 0).all(), (what, "padding")
    ids = i[:, :kk] - idx_base
    assert ((ids >= 0) & (ids < n)).all(), (what, "ids out of range")
    srt = ids.sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "duplicate ids")
    sk = s[:, :kk].double()
    assert torch.isfinite(sk).all(), (what, "non-finite score")
    ej = e.gather(1, ids)
    bj = B * qn[:, None] * cn[ids] * (1 + 1e-3)                                  # (1e-3: the second-order terms of gamma_n)
    err = (sk - ej).abs()
    assert (err <= bj).all(), (what, "pass-B score outside B(D)", ((err - bj) / (U24 * qn[:, None] * cn[ids]).clamp_min(1e-300)).max().item())
    if n > kk:
        lo = e - B * (1 + 1e-3) * qn[:, None] * cn[None, :]
        lo.scatter_(1, ids, float("-inf"))
        worst = lo.max(dim=1).values - (ej + bj).min(dim=1).values
        assert (worst <= 0).all(), (what, "a row left out beats the k-th", worst.max().item(), int(worst.argmax()))
    assert (s[:, :kk - 1] >= s[:, 1:kk]).all(), (what, "order")
    eq = s[:, :kk - 1] == s[:, 1:kk]
    assert (ids[:, :-1][eq] < ids[:, 1:][eq]).all(), (what, "tie order")
    return e


def check_prefix_answer(s, i, lim_c, k, base, what=None):
    """(s, i) = search_prefix with the limits `lim_c` (numpy int64, already clamped to the shard): no id at or beyond its query's limit,
    and the (-inf, -1) padding is exactly the missing rows."""
    import torch
    lim_t = torch.from_numpy(np.ascontiguousarray(lim_c)).to(i.device)[:, None]
    found = i >= 0
    assert (i[found] >= base).all() and (i < lim_t + base)[found].all(), (what, "an id at or beyond the limit")
    assert (i[~found] == -1).all() and (s[~found] == float("-inf")).all() and torch.isfinite(s[found]).all(), what
    assert torch.equal(found.sum(1), torch.clamp(lim_t[:, 0], max=k)), (what, "padding")


def allow_below(limit, n):
    """the bitmap (device int64 words, `where.pack_bitmap`) of the rows < limit of an n-row shard"""
    import torch
    from arxiv_rag_amd.where import pack_bitmap
    return torch.from_numpy(pack_bitmap(np.arange(n) < limit).view(np.int64)).cuda()


def check_against_filtered_and_fp64(idx, C_, Q_, lim_c, s, i, k, sample, what):
    """(s, i) = idx.search_prefix(Q_, limits, k).  For the sampled queries: bit-equal to the filtered search over the bitmap of rows < limit
    (queries that share a limit in one call), and an exact top-k of C[:limit] by float64."""
    import torch
    n, base = C_.shape[0], idx.idx_base
    by_limit = {}
    for j in sample:
        by_limit.setdefault(int(lim_c[j]), []).append(int(j))
    for limit, js in by_limit.items():
        jt = torch.tensor(js, device="cuda")
        q = Q_[jt].contiguous()
        fs, fi = idx.search(q, k, allow=allow_below(limit, n), n_allowed=limit)
        assert torch.equal(fi, i[jt]) and torch.equal(fs.view(torch.int32), s[jt].view(torch.int32)), \
            (what, "differs from the filtered search", limit, js[:4])
        if limit == 0:
            assert (i[jt] == -1).all() and (s[jt] == float("-inf")).all(), (what, "limit 0")
        else:
            check_topk_fp64(C_[:limit], q, s[jt], i[jt], k, idx_base=base, sample_rows=1, what=(what, limit))


# ---- encoder checked against float64 -------------------------------------------------------------------------------------------------
# References restate oracle/encoder_oracle.py in float64 (torch, on whatever device the inputs live) on the values the kernels read: bf16
# activations and matrices, fp32 biases, LayerNorm parameters and bias tables.  The optional `fault` of each reference computes a nearby
# WRONG operation, so that a test can show its budget would catch that mistake (the analogue of the search tolerance test).
U8 = 2.0 ** -8
ATTN_FAULTS = ("extra_key", "missing_key", "bias_shift", "bias_transpose", "query_shift")


def _t64(a, device=None):
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def bias_table_fp64(sd, cfg, S, device="cpu"):
    """MPNet: [heads, 2S+1] float64 Toeplitz table, entry (key - query) + S, from the oracle's bucket function (wide enough for one key
    past S and a shift by one); BERT: None."""
    if cfg.arch != C.ARCH_MPNET:
        return None
    d = np.arange(-S, S + 1)
    bucket = EO.relative_position_bucket(d, cfg.rel_buckets, cfg.rel_max_distance)
    return _t64(sd["encoder.relative_attention_bias.weight"][bucket].T, device)


def attention_fp64(qkv, lens, cfg, sd, fault=None):
    """Packed qkv [T, 3H] (bf16 or wider; device tensor) -> (ctx [T, H], spv [T, H], serr [T, heads]), all float64:
      ctx  = softmax(q k^T / sqrt(dh) + bias[key - query], keys < len) v per (sequence, head), the bias from the oracle's bucket function;
      spv  = sum_j p_ij |v_j| per output element (the scale of the kernel's P and accumulation roundings, see attention_budget);
      serr = a bound on the kernel's fp32 score error in base-2 units per (row, head), see attention_budget.
    fault: one of ATTN_FAULTS (a mistake the budget must expose): "extra_key" counts the clamped re-read of row len-1 as key len,
    "missing_key" drops key len-1, "bias_shift" reads bias[key - query + 1], "bias_transpose" reads bias[query - key], "query_shift"
    takes query row i+1 (clamped) for output row i."""
    import torch
    assert fault in (None,) + ATTN_FAULTS, fault
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    x = _t64(qkv)
    dev = x.device
    lens = np.asarray(lens, np.int64)
    cu = np.concatenate([[0], np.cumsum(lens)])
    S = int(max(lens.max(), 1)) + 1
    tbl = bias_table_fp64(sd, cfg, S, dev)
    if tbl is not None and fault == "bias_transpose":
        tbl = tbl.flip(1)                                        # entry d + S now holds bias[-d]
    ctx = torch.zeros((int(cu[-1]), H), dtype=torch.float64, device=dev)
    spv = torch.zeros_like(ctx)
    serr = torch.zeros((int(cu[-1]), nh), dtype=torch.float64, device=dev)
    l2e = 1.0 / np.log(2.0)
    for b in range(len(lens)):
        L = int(lens[b])
        if L == 0:
            continue
        seg = x[cu[b]:cu[b + 1]].view(L, 3, nh, dh).permute(1, 2, 0, 3)        # [3, nh, L, dh]
        q, k, v = seg[0], seg[1], seg[2]
        nk = L
        if fault == "query_shift":
            q = q[:, torch.clamp(torch.arange(1, L + 1, device=dev), max=L - 1)]
        if fault == "extra_key":
            k = torch.cat([k, k[:, L - 1:]], 1); v = torch.cat([v, v[:, L - 1:]], 1); nk = L + 1
        if fault == "missing_key" and L > 1:
            k = k[:, :L - 1]; v = v[:, :L - 1]; nk = L - 1
        raw = q @ k.transpose(1, 2)                                               # [nh, L, nk]
        sc = raw / np.sqrt(dh)
        bias = 0.0
        if tbl is not None:
            rel = torch.arange(nk, device=dev)[None, :] - torch.arange(L, device=dev)[:, None] + S
            if fault == "bias_shift":
                rel = rel + 1
            bias = tbl[:, rel]                                                    # [nh, L, nk]
            sc = sc + bias
        p = torch.softmax(sc, dim=-1)
        ctx[cu[b]:cu[b + 1]] = (p @ v).transpose(0, 1).reshape(L, H)
        spv[cu[b]:cu[b + 1]] = (p @ v.abs()).transpose(0, 1).reshape(L, H)
        # per key: the fp32 MFMA dot product (dh products, exact, summed in fp32), fma(acc, scale_log2e, bias * log2e) with both
        # constants rounded to fp32, and the score itself rounded -- in base-2 units
        dot_err = dh * U24 * (q.abs() @ k.abs().transpose(1, 2)) + 3 * U24 * raw.abs()
        e = l2e / np.sqrt(dh) * dot_err + 3 * U24 * l2e * (bias.abs() if tbl is not None else 0.0) + U24 * (sc.abs() * l2e)
        serr[cu[b]:cu[b + 1]] = e.max(dim=-1).values.transpose(0, 1)
    return ctx, spv, serr


def attention_budget(ref, spv, serr, lens, cfg):
    """Per-element bound on |kernel ctx - ref| for the fused attention kernels (csrc/encoder_kernels.h), float64 [T, H].  bf16 keeps 8
    significant bits, so round-to-nearest moves a value by at most 2^-8 of itself.
      score  s~_j = s_j + d_j with |d_j| <= E (serr, base-2 units; plus 2 ulps of exp2, 2^-23 / ln 2) -> each weight exp2(s~_j) is off by a
             factor within 2^(+-E): the normalised weights move by at most 2 (2^E - 1) relative, so |d ctx| <= 2 ln2 E (1 + ln2 E) spv;
      P      rounded to bf16 BEFORE both the PV MFMA and the row sum (an MFMA with ones), so the output is a weighted mean whose weights
             are off by (1 + e_j), |e_j| <= 2^-8: |d ctx| = |sum_j p_j (e_j - mean e) v_j| / (1 + mean e) <= 2 * 2^-8 / (1 - 2^-8) spv;
      sums   PV and the row sum accumulate L terms in fp32 (L 2^-24 each), the lazy rescale and the final division add a few roundings:
             (2 L + L / 16 + 4) 2^-24 spv;
      output rounded to bf16: 2^-8 (|ref| + the terms above).
    Together: a 2^-8 spv + 2^-8 |ref| + (score term), a = 2 (1 + 2^-7) + (2 L + L / 16 + 4) 2^-16, plus second-order terms."""
    import torch
    nh = cfg.heads
    dh = cfg.hidden // nh
    lens = np.asarray(lens, np.int64)
    L = torch.from_numpy(np.repeat(lens, lens).astype(np.float64)).to(ref.device)[:, None]
    a = 2 * (1 + 2.0 ** -7) + (2 * L + L / 16 + 4) * 2.0 ** -16
    E = serr.repeat_interleave(dh, dim=1) + 2 * U24 / np.log(2.0)
    ln2e = np.log(2.0) * E
    inner = a * U8 * spv + 2 * ln2e * (1 + ln2e) * spv
    return (U8 * (ref.abs() + inner) + inner) * (1 + 1e-6)


def _bf16_64(w, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(torch.bfloat16).to(device=device, dtype=torch.float64)


def layer_norm_fp64(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / (var + eps).sqrt() * g + b


def embed_ln_fp64(sd, cfg, ids, lens, device="cpu", fault=None):
    """ids [B, S] right-padded, lens [B] -> packed [sum(lens), H] float64: LN(word[id] + pos[p] (+ token_type[0] for BERT)), MPNet
    position ids from the count of non-pad tokens so far (pad-aware, oracle mpnet_position_ids), BERT p = 0, 1, ..., both clamped to
    max_pos - 1.
    fault: "pos_off_by_one" (MPNet ids one too high), "no_token_type" (BERT without the token-type row)."""
    import torch
    ids = np.asarray(ids, np.int64)
    lens = np.asarray(lens, np.int64)
    keep = np.arange(ids.shape[1])[None] < lens[:, None]
    if cfg.arch == C.ARCH_MPNET:
        pos = EO.mpnet_position_ids(ids, cfg.pad_id) + (1 if fault == "pos_off_by_one" else 0)
    else:
        pos = np.broadcast_to(np.arange(ids.shape[1])[None], ids.shape)
    pos = np.minimum(pos, cfg.max_pos - 1)                      # the kernel clamps as well
    e = _t64(sd["embeddings.word_embeddings.weight"][ids[keep]], device) + _t64(sd["embeddings.position_embeddings.weight"][pos[keep]], device)
    if cfg.arch != C.ARCH_MPNET and fault != "no_token_type":
        e = e + _t64(sd["embeddings.token_type_embeddings.weight"][0], device)
    return layer_norm_fp64(e, _t64(sd["embeddings.LayerNorm.weight"], device), _t64(sd["embeddings.LayerNorm.bias"], device), cfg.ln_eps)


def layer_fp64(sd, cfg, i, x, lens, fault=None):
    """Encoder layer i on packed hidden rows x [T, H] (device tensor) -> float64 [T, H]: matrices rounded to bf16 as HipEncoder uploads
    them, biases and LayerNorm parameters fp32, attention by attention_fp64, exact erf GELU, all arithmetic float64.
    fault: "prev_ln" (both LayerNorms take the previous layer's LN2 gamma / beta; layer 0 the embedding LayerNorm's),
    "no_oproj_residual" (y1 = ctx Wo^T + b without + x)."""
    import torch
    from arxiv_rag_amd.weights import layer_keys
    dev = x.device
    x = _t64(x)
    k = layer_keys(cfg, i)
    f32 = lambda n: _t64(sd[n], dev)
    lin = lambda a, n: a @ _bf16_64(sd[n + ".weight"], dev).T + f32(n + ".bias")
    wqkv = np.concatenate([sd[k[n] + ".weight"] for n in ("q", "k", "v")], 0)
    bqkv = np.concatenate([sd[k[n] + ".bias"] for n in ("q", "k", "v")], 0)
    qkv = x @ _bf16_64(wqkv, dev).T + _t64(bqkv, dev)
    ctx = attention_fp64(qkv, lens, cfg, sd)[0]
    if fault == "prev_ln":
        prev = layer_keys(cfg, i - 1)["ln2"] if i > 0 else "embeddings.LayerNorm"
        ln1 = ln2 = prev
    else:
        ln1, ln2 = k["ln1"], k["ln2"]
    y1 = lin(ctx, k["o"]) + (0.0 if fault == "no_oproj_residual" else x)
    a = layer_norm_fp64(y1, f32(ln1 + ".weight"), f32(ln1 + ".bias"), cfg.ln_eps)
    h = torch.nn.functional.gelu(lin(a, k["fc1"]))
    return layer_norm_fp64(lin(h, k["fc2"]) + a, f32(ln2 + ".weight"), f32(ln2 + ".bias"), cfg.ln_eps)


def pool_fp64(x, lens, cfg, fault=None):
    """Packed last hidden rows x [T, H] -> (pooled [B, H], mean |x| over the pooled rows [B, H]) float64: masked mean or CLS row;
    an empty sequence pools to zeros.  fault "count_pad_row": the mean divides by len + 1."""
    import torch
    x = _t64(x)
    lens = np.asarray(lens, np.int64)
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = torch.zeros((len(lens), x.shape[1]), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        rows = x[cu[b]:cu[b] + (1 if cfg.pool == C.POOL_CLS else L)]
        out[b] = rows.sum(0) / (rows.shape[0] + (1 if fault == "count_pad_row" else 0))
        mag[b] = rows.abs().mean(0)
    return out, mag


# ---- GEMM epilogues (csrc/gemm.h modes 0..6) checked against float64 -------------------------------------------------------------------
# Per-element budget of one linear layer's bf16 output against the float64 value of the same formula on the same bf16 / f32 inputs, with
# u = 2^-24 (U24) and 2^-8 (U8: round-to-nearest bf16 moves a value by at most 2^-8 of itself).  Every term is derived from the arithmetic,
# none is measured from a kernel:
#   accumulation   K u sum_k |a_k w_k|: bf16 products are exact in fp32, K - 1 fp32 additions in any order; modes 3/4 multiply the
#                  accumulator by rstd_m, and its error with it;
#   epilogue       one u of the result's magnitude bound per fp32 operation of the formula, counted without fused multiply-adds:
#                    modes 0/1  acc + b                                  1 op : 1 u (|acc| + |b|)
#                    modes 3/4  rstd * (acc - mean * s) + c              4 ops: 4 u (rstd (|acc| + |mean s|) + |c|)
#                    modes 2/5  (acc + b) + r                            2 ops: u (|acc| + |b|) + u (|acc| + |b| + |r|)
#                    mode 6     (acc + b) + (((r - mean) rstd) g + beta) 4 ops for the rebuilt residual, each within u L with
#                               L = |r - mean| rstd |g| + |beta|, then the two additions: u (2 (|acc| + |b|) + 5 L);
#   GELU           modes 1/4: the input error times max |GELU'| = 1.13, plus 1.75e-4, the bound csrc/gemm.h documents for gelu_poly_pk
#                  (the one constant taken from the project: the tests turn that comment into a checked contract);
#   output         U8 |ref|, and U8 of the error above (the rounding acts on the computed value).
GELU_POLY_BOUND = 1.75e-4
GELU_MAX_SLOPE = 1.13
EPI_FAULTS = ("trunc", "drop_k", "bias+4", "bias+8", "row+1", "rstd1", "s_unfolded", "mode6_as_5", "gamma_beta+8")
STAT_FAULTS = ("stats_unrounded", "partial_miss8", "partial_neighbour", "var_no_mu2")


def gelu_fp64(v):
    import torch
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


def bf16_trunc_fp64(v):
    """float64 -> the bf16 value obtained by dropping the low bits (round toward zero), as float64"""
    import torch
    return (v.float().view(torch.int32) & -65536).view(torch.float32).double()


def epi_fault_applies(fault, mode, M):
    if fault in ("trunc", "drop_k", "bias+4", "bias+8"):
        return True
    if fault == "row+1":
        return mode in (3, 4, 6) and M > 1
    if fault == "rstd1":
        return mode in (3, 4, 6)
    if fault == "s_unfolded":
        return mode in (3, 4)
    return mode == 6                                            # mode6_as_5, gamma_beta+8


def gemm_epilogue_fp64(mode, A, W, bias, resid=None, a_mean=None, a_rstd=None, s_vec=None, r_mean=None, r_rstd=None, r_gamma=None,
                       r_beta=None, fault=None, s_unfolded=None, acc=None, absacc=None):
    """One linear layer C = epi(A W^T) of csrc/gemm.h mode 0..6 in float64 on the values the kernel reads (A, W, resid bf16; vectors
    f32; row vectors may be longer than M) -> (pre, err): the value BEFORE the output rounding and the per-element bound on the kernel's
    fp32 error before that rounding (see above).  acc / absacc: A W^T and |A| |W|^T in float64 if the caller has them.
    fault (EPI_FAULTS): a nearby wrong operation the budget must expose; `err` is then meaningless.
      trunc: the output truncated to bf16 instead of rounded; drop_k: the last k element missing; bias+4 / bias+8: bias (modes 3/4: c)
      read 4 / 8 columns off; row+1: mean / rstd of row m + 1; rstd1: rstd = 1; s_unfolded: s_n of the unfolded weights; mode6_as_5: the
      residual not normalised; gamma_beta+8: the residual's gamma / beta read 8 columns off."""
    assert fault in (None,) + EPI_FAULTS and mode in range(7), (mode, fault)
    A64, W64 = _t64(A), _t64(W)
    M, K = A64.shape
    dev = A64.device
    acc = A64 @ W64.T if acc is None else acc
    absacc = A64.abs() @ W64.abs().T if absacc is None else absacc
    if fault == "drop_k":
        acc = acc - A64[:, -1:] * W64[:, -1][None, :]
    b = _t64(bias, dev)
    if fault in ("bias+4", "bias+8"):
        b = b.roll(-int(fault[-1]))
    rows = lambda v: (_t64(v, dev)[:M].roll(-1) if fault == "row+1" else _t64(v, dev)[:M])[:, None]
    lin = K * U24 * absacc
    if mode in (3, 4):
        mean, rstd = rows(a_mean), rows(a_rstd)
        if fault == "rstd1":
            rstd = rstd * 0 + 1
        s = _t64(s_unfolded if fault == "s_unfolded" else s_vec, dev)[None, :]
        v = rstd * (acc - mean * s) + b
        mag = rstd * (acc.abs() + (mean * s).abs()) + b.abs()
        err = rstd * lin + 4 * U24 * mag
    else:
        v = acc + b
        mag = acc.abs() + b.abs()
        err = lin + U24 * mag
    if mode in (1, 4):
        v = gelu_fp64(v)
        err = GELU_MAX_SLOPE * err + GELU_POLY_BOUND
    if mode in (2, 5):
        r = _t64(resid, dev)
        v = v + r
        err = lin + U24 * (2 * mag + r.abs())
    if mode == 6:
        r = _t64(resid, dev)
        if fault != "mode6_as_5":
            mean, rstd = rows(r_mean), rows(r_rstd)
            if fault == "rstd1":
                rstd = rstd * 0 + 1
            g, be = _t64(r_gamma, dev), _t64(r_beta, dev)
            if fault == "gamma_beta+8":
                g, be = g.roll(-8), be.roll(-8)
            ln = (r - mean) * rstd * g + be
            err = lin + U24 * (2 * mag + 5 * ((r - mean).abs() * rstd * g.abs() + be.abs()))
            r = ln
        v = v + r
    if fault == "trunc":
        v = bf16_trunc_fp64(v)
    return v, err


def gemm_epilogue_budget(pre, err):
    """|kernel output - pre| <= U8 |pre| + (1 + U8) err, per element"""
    return U8 * pre.abs() + (1 + U8) * err


def row_stats_fp64(out, eps, pre=None, fault=None):
    """LayerNorm statistics of the kernel's OWN bf16 output rows `out` [M, N] (so that a legitimate last-bit difference of the output does
    not move them), in float64 -> dict of (value, budget) per statistic:
      psum, psq [N / 64, M]: per-row sum / sum of squares of each 64-column slice, within 64 u sum |x| / 64 u sum x^2 (63 fp32 additions
        in any order; the squares of bf16 values are exact in fp32);
      mean [M] within (N + 2) u mean |x| (the slices' additions, the N / 64 partials', 1 / N rounded, the product);
      rstd [M] = 1 / sqrt(max(E[x^2] - mean^2, 0) + eps): an error of (N + 4) u E[x^2] in the variance moves it by the relative
        0.5 (N + 4) u E[x^2] / (var + eps); 4 u more for the addition of eps and rsqrt.
    fault (STAT_FAULTS), values only: stats_unrounded: the statistics of `pre` (the values before the output rounding);
    partial_miss8: a partial without its last 8 columns; partial_neighbour: partials written to the next slice; var_no_mu2: the
    variance without its - mean^2 term."""
    assert fault in (None,) + STAT_FAULTS, fault
    x = _t64(out)
    M, N = x.shape
    xs = x.view(M, N // 64, 64)
    res = {"psum": (xs.sum(-1).T, 64 * U24 * xs.abs().sum(-1).T), "psq": (xs.pow(2).sum(-1).T, 64 * U24 * xs.pow(2).sum(-1).T)}
    mean, ex2 = x.mean(1), x.pow(2).mean(1)
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    res["mean"] = (mean, (N + 2) * U24 * x.abs().mean(1))
    res["rstd"] = (rstd, rstd * (0.5 * (N + 4) * U24 * ex2 / (var + eps) + 4 * U24))
    if fault is None:
        return res
    y = _t64(pre).view(M, N // 64, 64) if fault == "stats_unrounded" else xs
    if fault == "partial_miss8":
        y = y[..., :56]
    ps, pq = y.sum(-1).T, y.pow(2).sum(-1).T
    if fault == "partial_neighbour":
        ps, pq = ps.roll(1, 0), pq.roll(1, 0)
    mu = ps.sum(0) / N
    v = pq.sum(0) / N - (0 if fault == "var_no_mu2" else mu * mu)
    return {"psum": ps, "psq": pq, "mean": mu, "rstd": (v.clamp_min(0) + eps).rsqrt()}


def fold_ln_fp64(W, gamma, beta, bias):
    """fold_ln_kernel in float64 from bf16 W [N, K] and f32 gamma / beta [K], bias [N] -> (prod, c, c_bud): prod = W gamma unrounded
    (the kernel's W' is the bf16 rounding of the fp32 product: the caller compares bit for bit, and checks s_n against the float64 sum of
    the device's own W' within K u sum |W'|: K fp32 additions of exact values); c_n = b_n + sum_k beta_k W[n][k], within
    (K + 1) u (|b_n| + sum |beta W|): K fused multiply-adds and the bias addition."""
    W64, g, be, b = _t64(W), _t64(gamma, W.device), _t64(beta, W.device), _t64(bias, W.device)
    K = W64.shape[1]
    return W64 * g, b + (W64 * be).sum(1), (K + 1) * U24 * (b.abs() + (W64 * be).abs().sum(1))


def epilogue_inputs(M, N, K, seed, device="cpu"):
    """Operands of one linear layer for every epilogue mode, chosen so that the LayerNorm plumbing matters: rows of A and of the residual
    have means of 1-3 row-rms and scales (hence rstd) spread over a decade, gamma = 1 +- 0.3, and bias, beta, s, c, the residual's gamma /
    beta are all non-constant and different from each other, so that any swap or shift between them is far outside the budget.
    W0: the unfolded bf16 matrix (modes 0-2, 5, 6); Wf, s, c: its LayerNorm fold (modes 3/4; fold_ln_kernel's formulas, here by torch);
    s_unf: sum_k W0 (the s_unfolded fault).  K > 1024 (only FFN-2 has such a K) takes GELU(N(0, 1)) rows for A.  Everything is drawn on
    the CPU (the same values on every machine) and moved to `device`.  Row vectors are padded to M rounded up to 256 (the tile kernels stage whole tiles)."""
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g).to(device)
    ru = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(device)
    cap = (M + 255) // 256 * 256

    def offset_rows(cols):
        scale = 10.0 ** (0.5 * ru(M, 1))
        off = (1 + (ru(M, 1) + 1)) * torch.sign(ru(M, 1))
        x = scale * (rn(M, cols) + off)
        x[:, -1] = scale[:, 0] * (1 + rn(M).abs()) * torch.sign(ru(M))      # the last k element is never negligible (the drop_k fault)
        x = x.to(torch.bfloat16)
        x64 = x.double()
        mean = x64.mean(1)
        rstd = ((x64 - mean[:, None]).pow(2).mean(1) + 1e-5).rsqrt()
        pad = lambda v: torch.cat([v.float(), torch.full((cap - M,), 777.0, device=device)])
        return x, pad(mean), pad(rstd)

    d = {"M": M, "N": N, "K": K, "row_cap": cap, "eps": 1e-5}
    d["A"], d["a_mean"], d["a_rstd"] = offset_rows(K)
    if K > 1024:                                                 # FFN-2's shape: its A operand is a GELU output, never LayerNorm-folded
        a = gelu_fp64(rn(M, K).double())
        a[:, -1] = 1 + rn(M).abs().double()
        d["A"] = a.to(torch.bfloat16)
    d["resid"], d["r_mean"], d["r_rstd"] = offset_rows(N)
    d["W0"] = (0.05 * rn(N, K)).to(torch.bfloat16)
    gamma, beta = 1 + 0.3 * ru(K), 0.2 + 0.3 * rn(K)
    d["bias"] = 0.5 + rn(N)
    w0 = d["W0"].float()
    d["Wf"] = (w0 * gamma).to(torch.bfloat16)
    d["s"] = d["Wf"].float().sum(1)
    d["c"] = d["bias"] + (w0 * beta).sum(1)
    d["s_unf"] = w0.sum(1)
    d["r_gamma"], d["r_beta"] = 1 + 0.3 * ru(N), 0.3 + 0.3 * rn(N)
    return d


def epilogue_ref_args(d, mode):
    """keyword arguments of gemm_epilogue_fp64 for mode `mode` on the operands of epilogue_inputs"""
    ln_in = mode in (3, 4)
    return dict(A=d["A"], W=d["Wf"] if ln_in else d["W0"], bias=d["c"] if ln_in else d["bias"], resid=d["resid"], a_mean=d["a_mean"],
                a_rstd=d["a_rstd"], s_vec=d["s"], r_mean=d["r_mean"], r_rstd=d["r_rstd"], r_gamma=d["r_gamma"], r_beta=d["r_beta"],
                s_unfolded=d["s_unf"])
