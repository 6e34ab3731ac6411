"""Test-only helpers: an oracle-backed stand-in for the encoder so that the host logic (CLI, loader,
writer, order contract, fallbacks, multi-rank sharding) can be exercised on CPU.  Never imported by
the product package."""
import hashlib
import json
import numpy as np

from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import seeded_state_dict
from oracle import encoder_oracle as EO


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
    step = max(1, (1 << 28) // max(1, q.shape[0]))
    return torch.cat([q64 @ c[a:a + step].double().T for a in range(0, c.shape[0], step)], dim=1)


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
    cn = c.double().norm(dim=1)                                                  # [n]
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
