"""Keyword side of hybrid search (`retrieval.use_hybrid_search`, `hybrid_alpha: 0.7`, 3-chunks/pipeline/config.yaml:67-68).

The reference configures hybrid search and has no code for it, so the definition is this project's:

* a term is a word-piece id of the model's own tokenizer (`WordPieceTokenizer._full_pieces`: no specials, no truncation);
* statistics are global over all ranks: `N` documents, `df(t)`, `avgdl = total_len / N`;
* a posting's impact is Lucene's BM25 (k1 = 1.2, b = 0.75, non-negative idf), float64 on the host, rounded once to f32:
  `idf = ln(1 + (N - df + 0.5) / (df + 0.5))`, `w = idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl))`;
* a query is its first 64 distinct word pieces, sorted by id; `bm25(q, d)` = the f32 sum of its terms' impacts in ascending id order;
* `arx_bm25_search` (csrc/bm25.hip) returns per query the n <= 32 rows with the largest `(score desc, row asc)`;
* `arx_bm25_search_filtered` does so among the rows a bitmap allows (one bitmap per query); scores, idf and avgdl are unchanged;
* `fuse` is relative-score fusion of the (global) dense and keyword lists: `alpha * normD + (1 - alpha) * normK`;
* `KeywordIndex.search_wide` (`arx_bm25_search_wide`) is the same top-n for n <= 1024 and `fuse_device` (`arx_hybrid_fuse`) is `fuse` on
  the device, bit for bit: hybrid search with long candidate lists (opt-in, `hybrid_on_device`);
* `build_postings_device` + `build_impacts_device` (`arx_bm25_build_postings`, `arx_bm25_build_impacts`, csrc/bm25_build.hip) are
  `build_postings` and `impacts_f64(...).astype(float32)` on the device, bit for bit: the index built in HBM from the flat word pieces
  (opt-in, `KeywordIndex(build_on_device=True)`; the host build stays the default).

`KeywordStats`, `build_postings`, `impacts_f64`, `flatten_pieces` and `fuse` are numpy only; `KeywordIndex` and the `*_device` functions
need the GPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

BM25_K1 = 1.2
BM25_B = 0.75
MAX_QUERY_TERMS = 64
MAX_N = 32                     # candidates per query (the list length limit of the cross-rank merge, as for the cosine search)
MAX_N_WIDE = 1024              # ... of `KeywordIndex.search_wide` and `fuse_device` (hybrid search on the device)


class KeywordStats:
    """Corpus statistics of BM25: `N` documents, `df` int64 [V] documents containing each term, `total_len` = sum of dl."""

    def __init__(self, N: int, df: np.ndarray, total_len: int):
        self.N, self.df, self.total_len = int(N), np.asarray(df, np.int64), int(total_len)

    @classmethod
    def from_postings(cls, term_ptr: np.ndarray, dl: np.ndarray) -> "KeywordStats":
        return cls(len(dl), np.diff(term_ptr), int(np.sum(dl, dtype=np.int64)))

    @classmethod
    def from_pieces(cls, piece_lists: Sequence[Sequence[int]], vocab_size: int) -> "KeywordStats":
        term_ptr, _, _, dl = build_postings(piece_lists, vocab_size)
        return cls.from_postings(term_ptr, dl)

    @property
    def avgdl(self) -> float:
        return float(self.total_len) / float(self.N) if self.N else 0.0

    def merge(self, other: "KeywordStats") -> "KeywordStats":
        """Statistics of the union of two disjoint document sets."""
        if self.df.shape != other.df.shape:
            raise ValueError(f"vocabulary sizes differ: {self.df.shape[0]} vs {other.df.shape[0]}")
        return KeywordStats(self.N + other.N, self.df + other.df, self.total_len + other.total_len)

    def all_reduce(self, group=None) -> "KeywordStats":
        """Sum over the ranks of `group` (a gloo host group: CPU tensors, nothing passes through device memory).  Without an
        initialised process group this is the identity."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        buf = torch.from_numpy(np.concatenate([np.array([self.N, self.total_len], np.int64), self.df]))
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        a = buf.numpy()
        return KeywordStats(int(a[0]), a[2:].copy(), int(a[1]))


def _host_group():
    """The gloo group host-side exchanges go through (the default group itself when that is gloo)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_backend() == "gloo":
        return None
    from .generate_embeddings_parallel import host_group
    return host_group()


def build_postings(piece_lists: Sequence[Sequence[int]], vocab_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> (term_ptr int64 [V + 1], rows uint32 [P], tf int32 [P], dl int64 [n_docs]): the postings of every term in CSR order, rows
    ascending inside a term.  One `unique` over the (term, row) pairs; no Python loop per posting."""
    n = len(piece_lists)
    dl = np.fromiter((len(p) for p in piece_lists), np.int64, n)
    total = int(dl.sum())
    terms = np.fromiter((t for p in piece_lists for t in p), np.int64, total)
    if total and (terms.min() < 0 or terms.max() >= vocab_size):
        raise ValueError(f"term id outside [0, {vocab_size})")
    rows = np.repeat(np.arange(n, dtype=np.int64), dl)
    pair, tf = np.unique(terms * max(n, 1) + rows, return_counts=True)          # sorted by (term, row)
    p_term = pair // max(n, 1)
    term_ptr = np.zeros(vocab_size + 1, np.int64)
    np.cumsum(np.bincount(p_term, minlength=vocab_size), out=term_ptr[1:])
    return term_ptr, (pair % max(n, 1)).astype(np.uint32), tf.astype(np.int32), dl


def idf_f64(stats: KeywordStats) -> np.ndarray:
    df = stats.df.astype(np.float64)
    return np.log1p((float(stats.N) - df + 0.5) / (df + 0.5))


def impacts_f64(term_ptr: np.ndarray, rows: np.ndarray, tf: np.ndarray, dl: np.ndarray, stats: KeywordStats) -> np.ndarray:
    """float64 impact of every posting, with the (global) statistics `stats`."""
    p_term = np.repeat(np.arange(len(term_ptr) - 1, dtype=np.int64), np.diff(term_ptr))
    idf = idf_f64(stats)[p_term]
    tff = tf.astype(np.float64)
    avgdl = stats.avgdl
    norm = BM25_K1 * (1.0 - BM25_B + BM25_B * dl[rows.astype(np.int64)].astype(np.float64) / avgdl) if len(rows) else np.zeros(0)
    return idf * tff * (BM25_K1 + 1.0) / (tff + norm)


def flatten_pieces(piece_lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (pieces int32 [T], doc_ptr int64 [n + 1]): the lists concatenated in order, `build_postings_device`'s input."""
    import itertools
    n = len(piece_lists)
    doc_ptr = np.zeros(n + 1, np.int64)
    if n:
        np.cumsum(np.fromiter(map(len, piece_lists), np.int64, n), out=doc_ptr[1:])
    flat = np.fromiter(itertools.chain.from_iterable(piece_lists), np.int64, int(doc_ptr[-1]))
    if len(flat) and (flat.min() < np.iinfo(np.int32).min or flat.max() > np.iinfo(np.int32).max):
        raise ValueError("term id outside the int32 range")
    return flat.astype(np.int32), doc_ptr


BUILD_TILE_TOKENS = 2048       # default tile of `arx_bm25_build_postings`: a block's chunk of tokens is a whole number of tiles
BUILD_ROUND_TOKENS = 256       # ... and a block walks its chunk this many tokens at a time (the smallest tile)


class DevicePostings:
    """What `build_postings_device` returns: `build_postings`' arrays in HBM (`term_ptr` int64 [V + 1], `post_row` uint32 as int32 bits
    and `post_tf` int32, each [max(P, 1)]), `doc_ptr` int64 [n + 1] in HBM for `build_impacts_device`, `n_postings` = P, and the host
    copies `KeywordIndex` keeps: `term_ptr_host` and `dl`."""

    def __init__(self, term_ptr, post_row, post_tf, doc_ptr, n_postings, term_ptr_host, dl):
        self.term_ptr, self.post_row, self.post_tf, self.doc_ptr = term_ptr, post_row, post_tf, doc_ptr
        self.n_postings, self.term_ptr_host, self.dl = int(n_postings), term_ptr_host, dl


def build_postings_raw(pieces_d, doc_ptr_d, n_tokens: int, n_docs: int, vocab_size: int, term_ptr, post_row, post_tf, n_post, bad,
                       tile_tokens: int = 0, max_blocks: int = 0) -> None:
    """`arx_bm25_build_postings_tuned` on device tensors the caller allocated (outputs with room for `n_tokens` postings); the
    workspace is this call's own."""
    import torch
    from . import _lib
    lib = _lib.load()
    need = lib.arx_bm25_build_workspace_bytes(int(n_tokens), int(n_docs), int(vocab_size))
    if need < 0:
        raise ValueError(f"n_tokens={n_tokens} must be below 2^31, n_docs={n_docs} below 2^32 and vocab_size={vocab_size} in [1, 2^24]")
    ws = torch.empty(need, dtype=torch.uint8, device=pieces_d.device)
    rc = lib.arx_bm25_build_postings_tuned(pieces_d.data_ptr(), int(n_tokens), doc_ptr_d.data_ptr(), int(n_docs), int(vocab_size),
                                           term_ptr.data_ptr(), post_row.data_ptr(), post_tf.data_ptr(), n_post.data_ptr(), bad.data_ptr(),
                                           ws.data_ptr(), ws.numel(), int(tile_tokens), int(max_blocks),
                                           torch.cuda.current_stream(pieces_d.device).cuda_stream)
    _lib.check(rc, "arx_bm25_build_postings")


def build_postings_device(pieces_flat, doc_ptr, vocab_size: int, device="cuda:0", tile_tokens: int = 0, max_blocks: int = 0) -> DevicePostings:
    """`build_postings` on the device, bit for bit (`arx_bm25_build_postings`).  `pieces_flat` int32 [T] and `doc_ptr` int64 [n + 1]
    (host arrays, `flatten_pieces`' layout).  `tile_tokens` / `max_blocks` choose the launch shape (tests, tuning): the answer's bits do
    not depend on it.  An id outside [0, V) raises `build_postings`' ValueError."""
    import torch
    pieces_flat, doc_ptr = np.ascontiguousarray(pieces_flat, np.int32), np.ascontiguousarray(doc_ptr, np.int64)
    n_tokens, n_docs, V = len(pieces_flat), len(doc_ptr) - 1, int(vocab_size)
    if pieces_flat.ndim != 1 or doc_ptr.ndim != 1 or n_docs < 0 or doc_ptr[0] != 0 or doc_ptr[-1] != n_tokens or np.any(np.diff(doc_ptr) < 0):
        raise ValueError("doc_ptr must be non-decreasing from 0 to len(pieces_flat)")
    dev = torch.device(device)
    # (never zero-sized device buffers: the C ABI wants non-null pointers even for a shard without tokens)
    pieces_d = torch.from_numpy(pieces_flat if n_tokens else np.zeros(1, np.int32)).to(dev)
    doc_ptr_d = torch.from_numpy(doc_ptr).to(dev)
    term_ptr = torch.empty(V + 1, dtype=torch.int64, device=dev)
    post_row = torch.empty(max(n_tokens, 1), dtype=torch.int32, device=dev)
    post_tf = torch.empty(max(n_tokens, 1), dtype=torch.int32, device=dev)
    n_post = torch.zeros(1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    build_postings_raw(pieces_d, doc_ptr_d, n_tokens, n_docs, V, term_ptr, post_row, post_tf, n_post, bad, tile_tokens, max_blocks)
    if int(bad.item()):
        raise ValueError(f"term id outside [0, {V})")
    P = int(n_post.item())
    if P == 0:
        post_row, post_tf = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    elif P < post_row.numel():                               # (the capacity was n_tokens: give the rest back)
        post_row, post_tf = post_row[:P].clone(), post_tf[:P].clone()
    return DevicePostings(term_ptr, post_row, post_tf, doc_ptr_d, P, term_ptr.cpu().numpy(), np.diff(doc_ptr))


def build_impacts_device(built: DevicePostings, stats: KeywordStats):
    """`impacts_f64(...).astype(float32)` on the device, bit for bit (`arx_bm25_build_impacts`), with the (global) statistics `stats`:
    -> post_w f32 [max(P, 1)] in HBM.  The idf table is `idf_f64(stats)` from the host (V doubles)."""
    import torch
    from . import _lib
    dev = built.term_ptr.device
    V = int(built.term_ptr.numel()) - 1
    if stats.df.shape[0] != V:
        raise ValueError("statistics are for another vocabulary size")
    post_w = torch.zeros(max(built.n_postings, 1), dtype=torch.float32, device=dev)
    idf = torch.from_numpy(idf_f64(stats)).to(dev)
    rc = _lib.load().arx_bm25_build_impacts(built.term_ptr.data_ptr(), built.post_row.data_ptr(), built.post_tf.data_ptr(), built.n_postings,
                                            built.doc_ptr.data_ptr(), len(built.dl), idf.data_ptr(), V, float(stats.avgdl), post_w.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "arx_bm25_build_impacts")
    return post_w


def distinct_terms(pieces: Sequence[int], exclude=()) -> List[int]:
    """The query's term list: distinct ids, the first 64 in order of appearance, sorted ascending."""
    seen, out = set(exclude), []
    for t in pieces:
        t = int(t)
        if t not in seen:
            seen.add(t)
            out.append(t)
            if len(out) == MAX_QUERY_TERMS:
                break
    return sorted(out)


def special_ids(tokenizer) -> set:
    """Ids the tokenizer's template adds around a sentence (bos / eos) plus the pad id: never query terms."""
    tok = tokenizer._tok
    tok.no_truncation()
    ids = set(tok.encode("", add_special_tokens=True).ids)
    ids.add(int(tokenizer.cfg.pad_id))
    return ids


def query_terms(tokenizer, texts: Sequence[str]) -> List[List[int]]:
    sp = special_ids(tokenizer)
    return [distinct_terms(p, exclude=sp) for p in tokenizer._full_pieces(list(texts))]


def pack_query_terms(term_lists: Sequence[Sequence[int]], vocab_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (q_terms int32 [nq, 64] -1 padded, q_nterms int32 [nq]); checks the kernel's contract on the host."""
    nq = len(term_lists)
    qt = np.full((nq, MAX_QUERY_TERMS), -1, np.int32)
    qn = np.zeros(nq, np.int32)
    for i, t in enumerate(term_lists):
        t = np.asarray(list(t), np.int64)
        if len(t) > MAX_QUERY_TERMS:
            raise ValueError(f"query {i}: {len(t)} terms (at most {MAX_QUERY_TERMS})")
        if len(t) and (t.min() < 0 or t.max() >= vocab_size):
            raise ValueError(f"query {i}: term id outside [0, {vocab_size})")
        if len(t) > 1 and not np.all(np.diff(t) > 0):
            raise ValueError(f"query {i}: term ids must be strictly ascending")
        qt[i, :len(t)] = t
        qn[i] = len(t)
    return qt, qn


def fuse(dense_scores, dense_ids, kw_scores, kw_ids, alpha: float, k: int):
    """Relative-score fusion of two global candidate lists per query.

    dense_* / kw_*: [nq, n] f32 scores and int64 row ids, unused slots id -1.  Within each list `norm(s) = (s - min) / (max - min)`
    (1 for every member when max == min); a row absent from a list gets 0 from that side.  `fused = alpha * normD + (1 - alpha) *
    normK` over the union, in float64, ranked (fused desc, row asc).  -> (fused f64 [nq, k], ids int64 [nq, k], dense f32 [nq, k],
    keyword f32 [nq, k]); the two score columns are nan where the row was not in that list; unused slots are (-inf, -1, nan, nan)."""
    if not (0.0 <= float(alpha) <= 1.0):
        raise ValueError(f"alpha={alpha} must be in [0, 1]")
    ds, di = np.atleast_2d(np.asarray(dense_scores, np.float32)), np.atleast_2d(np.asarray(dense_ids, np.int64))
    ks, ki = np.atleast_2d(np.asarray(kw_scores, np.float32)), np.atleast_2d(np.asarray(kw_ids, np.int64))
    nq = ds.shape[0]
    if ks.shape[0] != nq or ds.shape != di.shape or ks.shape != ki.shape:
        raise ValueError("list shapes disagree")
    out_f = np.full((nq, k), -np.inf, np.float64); out_i = np.full((nq, k), -1, np.int64)
    out_d = np.full((nq, k), np.nan, np.float32); out_k = np.full((nq, k), np.nan, np.float32)

    def norm(s, ids):
        keep = ids >= 0
        s64, rows = s[keep].astype(np.float64), ids[keep]
        if not len(rows):
            return {}, {}
        lo, hi = s64.min(), s64.max()
        nv = np.ones_like(s64) if hi == lo else (s64 - lo) / (hi - lo)
        return dict(zip(rows.tolist(), nv.tolist())), dict(zip(rows.tolist(), s[keep].tolist()))

    for q in range(nq):
        nd, rd = norm(ds[q], di[q])
        nk, rk = norm(ks[q], ki[q])
        rows = sorted(set(nd) | set(nk))
        fused = [(float(alpha) * nd.get(r, 0.0) + (1.0 - float(alpha)) * nk.get(r, 0.0), r) for r in rows]
        fused.sort(key=lambda fr: (-fr[0], fr[1]))
        for j, (f, r) in enumerate(fused[:k]):
            out_f[q, j], out_i[q, j] = f, r
            out_d[q, j], out_k[q, j] = rd.get(r, np.nan), rk.get(r, np.nan)
    return out_f, out_i, out_d, out_k


def fuse_device(dense_scores, dense_ids, kw_scores, kw_ids, alpha: float, k: int):
    """`fuse` on the device (`arx_hybrid_fuse`), bit for bit: device tensors in ([nq, n_dense] / [nq, n_kw], f32 scores and int64 ids,
    each list at most 1024 long with distinct ids), device tensors out (fused f64, ids int64, dense f32, keyword f32, each [nq, k],
    k <= 1024).  Nothing crosses to the host."""
    import torch
    from . import _lib
    if not (0.0 <= float(alpha) <= 1.0):
        raise ValueError(f"alpha={alpha} must be in [0, 1]")
    for name, t, dt in (("dense_scores", dense_scores, torch.float32), ("dense_ids", dense_ids, torch.int64),
                        ("kw_scores", kw_scores, torch.float32), ("kw_ids", kw_ids, torch.int64)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 or t.device != dense_scores.device:
            raise ValueError(f"{name} must be a 2-d {dt} tensor on the device of dense_scores")
    nq = dense_scores.shape[0]
    if kw_scores.shape[0] != nq or dense_scores.shape != dense_ids.shape or kw_scores.shape != kw_ids.shape:
        raise ValueError("list shapes disagree")
    n_dense, n_kw = int(dense_scores.shape[1]), int(kw_scores.shape[1])
    if not (1 <= n_dense <= MAX_N_WIDE and 1 <= n_kw <= MAX_N_WIDE and 1 <= int(k) <= MAX_N_WIDE):
        raise ValueError(f"list lengths {n_dense}, {n_kw} and k={k} must each be in [1, {MAX_N_WIDE}]")
    dev = dense_scores.device
    out_f = torch.empty((nq, k), dtype=torch.float64, device=dev); out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev); out_k = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if nq == 0:
        return out_f, out_i, out_d, out_k
    ds, di, ks, ki = dense_scores.contiguous(), dense_ids.contiguous(), kw_scores.contiguous(), kw_ids.contiguous()
    rc = _lib.load().arx_hybrid_fuse(ds.data_ptr(), di.data_ptr(), n_dense, ks.data_ptr(), ki.data_ptr(), n_kw, nq, float(alpha), int(k),
                                     out_f.data_ptr(), out_i.data_ptr(), out_d.data_ptr(), out_k.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "arx_hybrid_fuse")
    return out_f, out_i, out_d, out_k


class KeywordIndex:
    """This rank's BM25 impact index in HBM (CSR by term) and its top-n search through `arx_bm25_search`."""

    def __init__(self, pieces: Optional[Sequence[Sequence[int]]] = None, texts: Optional[Sequence[str]] = None, tokenizer=None,
                 vocab_size: Optional[int] = None, stats: Optional[KeywordStats] = None, idx_base: int = 0, device="cuda:0",
                 build_on_device: bool = False):
        """`pieces` (word-piece id lists) or `texts` + `tokenizer`.  `stats`: the GLOBAL statistics when this index is one shard of a
        larger corpus (None = this shard's own; "global" = this shard's own summed over all ranks of the host group).  Row r of the
        index is global row `idx_base + r`.
        `build_on_device` (False = nothing changes): the postings and their impacts are computed on the device
        (`build_postings_device`, `build_impacts_device`) and stay there; the index is the default build's, bit for bit.  `pieces` may
        then also be a `(pieces int32 [T], doc_ptr int64 [n + 1])` pair of numpy arrays, and `texts` go through
        `tokenizer.full_pieces_flat`, which yields such a pair without a Python list per chunk."""
        if pieces is None:
            if texts is None or tokenizer is None:
                raise ValueError("pass pieces, or texts with a tokenizer")
            pieces = tokenizer.full_pieces_flat(list(texts)) if build_on_device else tokenizer._full_pieces(list(texts))
        if vocab_size is None:
            if tokenizer is None:
                raise ValueError("vocab_size is needed when no tokenizer is given")
            vocab_size = int(tokenizer.cfg.vocab_size)
        if build_on_device:
            flat, doc_ptr = pieces if (isinstance(pieces, tuple) and len(pieces) == 2 and isinstance(pieces[0], np.ndarray)) else flatten_pieces(pieces)
            built = build_postings_device(flat, doc_ptr, int(vocab_size), device)
            self._setup(built.term_ptr_host, None, None, built.dl, int(vocab_size), stats, idx_base, device, tokenizer, built=built)
            return
        term_ptr, rows, tf, dl = build_postings(pieces, int(vocab_size))
        self._setup(term_ptr, rows, tf, dl, int(vocab_size), stats, idx_base, device, tokenizer)

    @classmethod
    def from_postings(cls, term_ptr: np.ndarray, rows: np.ndarray, tf: np.ndarray, dl: np.ndarray, stats: Optional[KeywordStats] = None,
                      idx_base: int = 0, device="cuda:0", tokenizer=None) -> "KeywordIndex":
        """An index over postings the caller already holds in `build_postings`' layout (synthetic corpora of the benchmark)."""
        self = cls.__new__(cls)
        self._setup(np.asarray(term_ptr, np.int64), np.asarray(rows, np.uint32), np.asarray(tf, np.int32), np.asarray(dl, np.int64),
                    len(term_ptr) - 1, stats, idx_base, device, tokenizer)
        return self

    def _setup(self, term_ptr, rows, tf, dl, vocab_size, stats, idx_base, device, tokenizer, built: Optional[DevicePostings] = None):
        """`built`: the postings are in HBM already (`build_on_device`); `rows` and `tf` are then None and nothing is uploaded."""
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.tokenizer, self.vocab_size, self.idx_base = tokenizer, int(vocab_size), int(idx_base)
        self.local_stats = KeywordStats.from_postings(term_ptr, dl)
        if isinstance(stats, str):
            if stats != "global":
                raise ValueError(f"stats={stats!r}: a KeywordStats, None or \"global\"")
            stats = self.local_stats.all_reduce(_host_group())
        self.stats = stats if stats is not None else self.local_stats
        if self.stats.df.shape[0] != self.vocab_size:
            raise ValueError("statistics are for another vocabulary size")
        self.device = torch.device(device)
        self.term_ptr_host = term_ptr
        self._ws = None
        if built is not None:
            self.n_rows, self.n_postings = len(dl), built.n_postings
            self.term_ptr, self.post_row, self.post_w = built.term_ptr, built.post_row, build_impacts_device(built, self.stats)
            return
        w64 = impacts_f64(term_ptr, rows, tf, dl, self.stats)
        self.n_rows, self.n_postings = len(dl), len(rows)
        self.term_ptr = torch.from_numpy(term_ptr).to(self.device)
        # (never zero-sized device buffers: the C ABI wants non-null pointers even for a shard without postings)
        self.post_row = torch.from_numpy(np.ascontiguousarray(rows if len(rows) else np.zeros(1, np.uint32)).view(np.int32)).to(self.device)
        self.post_w = torch.from_numpy(np.ascontiguousarray(w64.astype(np.float32) if len(rows) else np.zeros(1, np.float32))).to(self.device)

    # ---- queries ------------------------------------------------------------------------------------------------------------
    def query_terms(self, texts: Sequence[str]) -> List[List[int]]:
        if self.tokenizer is None:
            raise ValueError("this index was built without a tokenizer: pass term lists")
        return query_terms(self.tokenizer, texts)

    def _term_lists(self, queries) -> List[List[int]]:
        queries = list(queries)
        if queries and all(isinstance(q, str) for q in queries):
            return self.query_terms(queries)
        return [list(q) for q in queries]

    def posting_bytes(self, term_lists: Sequence[Sequence[int]]) -> np.ndarray:
        """Bytes of posting lists (row + impact, 8 per posting) each query's terms cover: the kernel's streaming work."""
        ln = np.diff(self.term_ptr_host)
        return np.array([8 * int(ln[np.asarray(list(t), np.int64)].sum()) if len(t) else 0 for t in term_lists], np.int64)

    def _check_filters(self, allow, filter_of, nq: int):
        """-> (allow as a contiguous [F, W] tensor, filter_of or None); ValueError for a wrong shape, dtype or device."""
        import torch
        n_words = (self.n_rows + 63) // 64

        def here(t):                                             # ("cuda" names the current device: only a stated index is compared)
            return t.device.type == self.device.type and (self.device.index is None or t.device.index == self.device.index)
        if not isinstance(allow, torch.Tensor) or allow.dtype != torch.int64 or not here(allow):
            raise ValueError(f"allow must be an int64 tensor on {self.device} (row bitmaps, [W] or [F, W])")
        if allow.dim() == 1:
            allow = allow[None]
        if allow.dim() != 2 or allow.shape[0] < 1 or allow.shape[1] != n_words:
            raise ValueError(f"allow has shape {tuple(allow.shape)}; expected [{n_words}] or [F, {n_words}] (ceil(n_rows / 64) words per filter)")
        if filter_of is not None:
            if not isinstance(filter_of, torch.Tensor) or filter_of.dtype != torch.int32 or not here(filter_of):
                raise ValueError(f"filter_of must be an int32 tensor on {self.device}")
            if tuple(filter_of.shape) != (nq,):
                raise ValueError(f"filter_of has shape {tuple(filter_of.shape)}; expected [{nq}] (one bitmap index per query)")
            filter_of = filter_of.contiguous()
        return allow.contiguous(), filter_of

    QUERY_STEP = 4096              # queries per kernel call (the grid's y extent is limited to 65535)
    WIDE_QUERY_STEP = 256          # queries per wide call: bounds the partial lists (at most 512 KiB per query) to 128 MiB

    def _search(self, export: str, n: int, n_max: int, step: int, queries, allow, filter_of, tile_rows: int, max_blocks: int):
        """`search` and `search_wide`: `export` is the library's call (and names its workspace function), `n_max` its limit on n,
        `step` the queries per call."""
        import torch
        from . import _lib
        if not (1 <= n <= n_max):
            raise ValueError(f"n={n} must be in [1, {n_max}]")
        if allow is None and filter_of is not None:
            raise ValueError("filter_of needs allow")
        qt, qn = pack_query_terms(self._term_lists(queries), self.vocab_size)
        nq = len(qn)
        if allow is not None:
            allow, filter_of = self._check_filters(allow, filter_of, nq)
        out_s = torch.full((nq, n), float("-inf"), dtype=torch.float32, device=self.device)
        out_i = torch.full((nq, n), -1, dtype=torch.int64, device=self.device)
        if nq == 0 or self.n_rows == 0:
            return out_s, out_i
        qt_d, qn_d = torch.from_numpy(qt).to(self.device), torch.from_numpy(qn).to(self.device)
        wide = export == "arx_bm25_search_wide"
        need = (self.lib.arx_bm25_wide_workspace_bytes if wide else self.lib.arx_bm25_workspace_bytes)(self.n_rows, min(nq, step), n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        for a in range(0, nq, step):
            b = min(nq, a + step)
            filters = () if export == "arx_bm25_search_tuned" else (                      # (the one export without the filter arguments)
                None if allow is None else allow.data_ptr(), 0 if allow is None else int(allow.shape[0]),
                None if filter_of is None else filter_of[a:b].data_ptr())
            rc = getattr(self.lib, export)(
                self.term_ptr.data_ptr(), self.post_row.data_ptr(), self.post_w.data_ptr(), self.vocab_size, self.n_rows, *filters,
                qt_d[a:b].data_ptr(), qn_d[a:b].data_ptr(), b - a, n, out_s[a:b].data_ptr(), out_i[a:b].data_ptr(), self.idx_base,
                self._ws.data_ptr(), self._ws.numel(), int(tile_rows), int(max_blocks), st)
            _lib.check(rc, export.replace("_tuned", ""))
        return out_s, out_i

    def search(self, queries, n: int = MAX_N, tile_rows: int = 0, max_blocks: int = 0, allow=None, filter_of=None):
        """`queries`: texts, or term-id lists (strictly ascending).  -> (scores f32 [nq, n], ids int64 [nq, n]) on the device; unused
        slots are (-inf, -1).  `tile_rows` / `max_blocks` choose the launch shape (tests, tuning): the answer's bits do not depend on it.
        `allow` (None = every row, today's call): row bitmaps of this index's rows as an int64 device tensor [W] or [F, W],
        W = ceil(n_rows / 64), in `ShardIndex.search(allow=...)`'s convention; only allowed rows are returned, with the scores they have
        without a filter (`arx_bm25_search_filtered`).  `filter_of`: int32 device tensor [nq], the bitmap of each query (None = bitmap 0
        for all; an index outside [0, F) leaves that query without rows)."""
        export = "arx_bm25_search_tuned" if allow is None else "arx_bm25_search_filtered_tuned"
        return self._search(export, n, MAX_N, self.QUERY_STEP, queries, allow, filter_of, tile_rows, max_blocks)

    def search_wide(self, queries, n: int, allow=None, filter_of=None, tile_rows: int = 0, max_blocks: int = 0):
        """`search` with `n` up to MAX_N_WIDE = 1024 (`arx_bm25_search_wide`): the same kernel, queries, scores, order, padding and filter
        arguments, so for n <= 32 the same bits, and the first m entries of an n-list are the m-list.  This shard only: a cross-rank
        merge of long lists is out of scope."""
        return self._search("arx_bm25_search_wide", n, MAX_N_WIDE, self.WIDE_QUERY_STEP, queries, allow, filter_of, tile_rows, max_blocks)

    def search_distributed(self, queries, n: int = MAX_N, group=None, allow=None, filter_of=None):
        """Every rank passes the SAME queries; returns the global keyword top-n on every rank (local top-n -> all-gather -> merge kernel,
        as `ShardIndex.search_distributed`).  `allow` / `filter_of`: THIS rank's own bitmaps, as in `search`; the merge is unchanged."""
        import torch.distributed as dist
        from .index import gather_partials, merge_partials
        s, i = self.search(queries, n, allow=allow, filter_of=filter_of)
        if not dist.is_initialized() or s.shape[0] == 0:
            return s, i
        all_s, all_i = gather_partials(s, i, group)
        return merge_partials(all_s, all_i, n)

    def scores(self, terms: Sequence[int], row_lo: int = 0, row_hi: Optional[int] = None, tile_rows: int = 0):
        """Debug tap: the f32 score of every row of [row_lo, row_hi) for ONE query's term list (0 = holds none of its terms)."""
        import torch
        from . import _lib
        row_hi = self.n_rows if row_hi is None else row_hi
        qt, qn = pack_query_terms([terms], self.vocab_size)
        out = torch.empty(row_hi - row_lo, dtype=torch.float32, device=self.device)
        qt_d = torch.from_numpy(qt).to(self.device)
        rc = self.lib.arx_bm25_scores(self.term_ptr.data_ptr(), self.post_row.data_ptr(), self.post_w.data_ptr(), self.vocab_size, self.n_rows,
                                      qt_d.data_ptr(), int(qn[0]), row_lo, row_hi, int(tile_rows), out.data_ptr(),
                                      torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "arx_bm25_scores")
        return out
