"""Product-quantised search: rank every row by the sum of a query's byte look-up tables over the row's 8-bit PQ codes, rescore the best
`n_candidates` exactly (`arx_pq_encode`, `arx_pq_lut`, `arx_pq_candidates`, include/arx.h; INTEGRATION.md "Product-quantised search").

    pi = PqIndex.build(index, dsub=8, centre="mean")                    # index: a ShardIndex; trains the codebooks, encodes the rows
    scores, ids, count = pi.search(q, k=10, n_candidates=128)          # q: fp16 device [nq, dim]

A code keeps one byte per `dsub` dimensions, the nearest of 256 trained sub-centroids: dim / dsub bytes per row, at dsub = 8 the
footprint of `binary.py`'s sign bits.  `candidates` is the exact list C(q) of the first `n_candidates` visible rows by (table sum desc,
row asc): sums are integers, so the list is defined bit for bit.  `search` is the exact top-k of C(q): the candidate lists go to
`arx_ivf_search` as inverted lists (`ivf._launch`), so every returned score has the bits of `ShardIndex.search` and the order is (score
desc, row asc); the answer equals `ShardIndex.search(allow=bitmap of C(q))`.  Which rows get scored is the only approximation;
`n_candidates >= ` the visible rows is the exact search.

`codes.launch` is the one place this module launches a kernel of the library through; the lifecycle of the code array, `search` and
the rescore are `codes.CodeIndex`'s, shared with `binary.BinaryIndex` (the rescore's launch is `ivf._launch`).  `encode_host`,
`lut_host`, `sums_host`, `candidates_host` and `search_host` restate the definitions with numpy (for the tests; the product path never
calls them); `check_args`, `check_dsub`, `check_codebooks` and `check_query_with_pq` are the refusals; a tensor of the wrong kind is a
ValueError too.  `train` is Lloyd's algorithm whose assign step is `arx_pq_encode`: its floats need not be reproducible; the codebooks
are stored, and everything after them is.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .binary import _require_tensor, _visible, check_dim
from .codes import MAX_CANDIDATES, MAX_K, RESCORE_QUERIES, CodeIndex, _is_int, check_candidate_args, check_centre, launch, rescore_host  # noqa: F401

N_CODES, MAX_M, DSUBS = 256, 256, (4, 8, 16, 32, 64)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_dsub(dim, dsub) -> int:
    """M = dim / dsub, or a ValueError: dim a multiple of 64 in [64, 8192], dsub a power of two in [4, 64], M in [1, 256]."""
    check_dim(dim)
    if not _is_int(dsub) or dsub not in DSUBS:
        raise ValueError(f"dsub={dsub!r} must be a power of two in [4, 64]")
    M = int(dim) // int(dsub)
    if not (1 <= M <= MAX_M):
        raise ValueError(f"M = dim / dsub = {M} must be in [1, {MAX_M}] (dim={dim}, dsub={dsub}): the look-up tables must fit in LDS")
    return M


def check_args(k, n_candidates, dim=None, dsub=None) -> None:
    """The refusals of `PqIndex.search` / `candidates` (k = None), each a ValueError before anything is launched."""
    check_candidate_args(k, n_candidates)
    if dim is not None:
        check_dim(dim) if dsub is None else check_dsub(dim, dsub)


def check_codebooks(codebooks, dim: int, dsub: int) -> np.ndarray:
    """`codebooks` (an array or a tensor) -> a contiguous float32 array [M, 256, dsub] of finite values, or a ValueError."""
    M = check_dsub(dim, dsub)
    c = np.asarray(codebooks.detach().cpu().numpy() if hasattr(codebooks, "detach") else codebooks)
    if c.shape != (M, N_CODES, dsub) or c.dtype.kind != "f":
        raise ValueError(f"codebooks must be a float array of shape ({M}, {N_CODES}, {dsub}), not {c.dtype} {tuple(c.shape)}")
    c = np.ascontiguousarray(c, dtype=np.float32)
    if not np.isfinite(c).all():
        raise ValueError("codebooks must hold finite values only")
    return c


def check_query_with_pq(pq_candidates, *, has_index: bool, per_query_filters: bool = False, hybrid_alpha=None, group_by=None, min_score=None,
                        nprobe=None, binary_candidates=None, boost_weight=None, world: int = 1, n_width: int = 1) -> None:
    """The refusals of `query(pq_candidates=...)`, `retrieve` and `search_queries`, each a ValueError naming the part, before any
    launch (`modes.check_mode`).  `n_width`: the rows the search returns per query (the reranker's or MMR's candidates, else n_results)."""
    from .modes import check_mode
    check_mode("pq_candidates", pq_candidates, has_index=has_index, per_query=per_query_filters, hybrid_alpha=hybrid_alpha, group_by=group_by,
               min_score=min_score, world=world, n_width=n_width,
               others={"nprobe": nprobe, "binary_candidates": binary_candidates, "boost_weight": boost_weight})


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def encode_host(X, codebooks, centre=None) -> np.ndarray:
    """uint8 [n, M]: what `arx_pq_encode` writes.  `X` fp16 [n, dim]; `codebooks` f32 [M, 256, dsub]; `centre` None or f32 [dim].  Every
    operation is one rounded f32 operation, in the kernel's order; the code is the first minimum among the non-NaN distances (0 when
    d_0 is NaN: nothing is below a NaN)."""
    X, cb = np.asarray(X), np.asarray(codebooks, dtype=np.float32)
    if X.dtype != np.float16 or X.ndim != 2:
        raise ValueError("X must be an fp16 [n, dim] array")
    M, _, dsub = cb.shape
    n = X.shape[0]
    codes = np.zeros((n, M), np.uint8)
    with np.errstate(all="ignore"):
        V = X.astype(np.float32)
        if centre is not None:
            V = V - np.asarray(centre, dtype=np.float32)[None, :]
        for m in range(M):
            acc = np.zeros((n, N_CODES), np.float32)
            for t in range(dsub):
                e = V[:, m * dsub + t, None] - cb[m, None, :, t]
                acc = acc + e * e
            first_nan = np.isnan(acc[:, 0])
            code = np.argmin(np.where(np.isnan(acc), np.float32(np.inf), acc), axis=1)
            codes[:, m] = np.where(first_nan, 0, code)
    return codes


def lut_float_host(Q, codebooks) -> np.ndarray:
    """f32 [nq, M, 256]: the inner products `arx_pq_lut` quantises, in its operation order."""
    Q, cb = np.asarray(Q), np.asarray(codebooks, dtype=np.float32)
    if Q.dtype != np.float16 or Q.ndim != 2:
        raise ValueError("Q must be an fp16 [nq, dim] array")
    M, _, dsub = cb.shape
    Qf = Q.astype(np.float32).reshape(Q.shape[0], M, dsub)
    f = np.zeros((Q.shape[0], M, N_CODES), np.float32)
    with np.errstate(all="ignore"):
        for t in range(dsub):
            f = f + Qf[:, :, t, None] * cb[None, :, :, t]
    return f


def quantise_host(f) -> np.ndarray:
    """uint8 [nq, M, 256] from the float tables [nq, M, 256], as `arx_pq_lut` maps them to bytes: one scale per query."""
    f = np.asarray(f, dtype=np.float32)
    out = np.zeros(f.shape, np.uint8)
    with np.errstate(all="ignore"):
        for q in range(f.shape[0]):
            if not np.isfinite(f[q]).all():
                continue
            lo = f[q].min(axis=1)
            span = np.float32((f[q].max(axis=1) - lo).max())
            if not (span > 0) or not np.isfinite(span):
                continue
            inv = np.float32(255.0) / span
            out[q] = np.minimum(np.float32(255.0), np.rint((f[q] - lo[:, None]) * inv)).astype(np.uint8)
    return out


def lut_host(Q, codebooks) -> np.ndarray:
    """uint8 [nq, M, 256]: what `arx_pq_lut` writes."""
    return quantise_host(lut_float_host(Q, codebooks))


def sums_host(codes, lut) -> np.ndarray:
    """int32 [nq, n]: s(q, r) = sum over m of lut[q][m][codes[r][m]]."""
    codes, lut = np.asarray(codes, dtype=np.uint8), np.asarray(lut, dtype=np.uint8)
    nq, M = lut.shape[0], lut.shape[1]
    at = codes.astype(np.int64) + (np.arange(M, dtype=np.int64) * N_CODES)[None, :]      # [n, M]: where a row's bytes point in a query's table
    flat = lut.reshape(nq, M * N_CODES)
    out = np.empty((nq, codes.shape[0]), np.int32)
    for q in range(nq):                                          # (a query at a time: one contiguous table, six times faster at M = 256)
        out[q] = flat[q][at].sum(axis=1, dtype=np.int32)
    return out


def candidates_host(codes, lut, n_candidates: int, allow=None):
    """(cand int32 [nq, R], sum int32 [nq, R], count int64 [nq]): what `arx_pq_candidates` returns, bit for bit.  `allow`: None, a bool
    mask [n_rows] or bitmap words."""
    codes, lut = np.asarray(codes), np.asarray(lut)
    n, nq, R = codes.shape[0], lut.shape[0], int(n_candidates)
    rows = np.nonzero(_visible(allow, n))[0]
    s = sums_host(codes[rows], lut)
    cand, sums, count = np.full((nq, R), -1, np.int32), np.full((nq, R), -1, np.int32), np.zeros(nq, np.int64)
    for q in range(nq):
        best = np.lexsort((rows, -s[q].astype(np.int64)))[:R]     # sum desc, row asc
        m = best.shape[0]
        cand[q, :m], sums[q, :m], count[q] = rows[best], s[q][best], m
    return cand, sums, count


def search_host(X, codes, lut, Q, k: int, n_candidates: int, allow=None):
    """(scores f32 [nq, k], ids int64 [nq, k], count int64 [nq]): what `PqIndex.search` returns with idx_base = 0, bit for bit: the
    `codes.rescore_host` of `candidates_host`'s lists."""
    cand, _, count = candidates_host(codes, lut, n_candidates, allow)
    return rescore_host(X, Q, cand, count, k)


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def _workspace_bytes(n_rows: int, nq: int, dim: int, dsub: int, R: int) -> int:
    """`arx_pq_workspace_bytes` (host arithmetic, nothing is launched); outside the limits an `ArxError`."""
    from . import _lib
    need = _lib.load().arx_pq_workspace_bytes(int(n_rows), max(int(nq), 1), int(dim), int(dsub), int(R))
    if need < 0:
        raise _lib.ArxError(f"arx_pq_candidates: unsupported shape n_rows={n_rows} nq={nq} dim={dim} dsub={dsub} n_candidates={R}")
    return int(need)


def _require_codebooks(codebooks, dim: int, dsub: int) -> int:
    import torch
    M = check_dsub(dim, dsub)
    _require_tensor(codebooks, "codebooks", (torch.float32,), 3, torch.is_tensor(codebooks) and tuple(codebooks.shape) == (M, N_CODES, dsub),
                    f" [{M}, {N_CODES}, {dsub}]")
    return M


def encode_device(x16, dsub: int, centre, codebooks):
    """`arx_pq_encode` on the current stream: `x16` fp16 device [n, dim] (dense), `centre` f32 device [dim] or None, `codebooks` f32
    device [M, 256, dsub] -> uint8 device [n, M]."""
    import torch
    _require_tensor(x16, "rows", (torch.float16,), 2)
    n, dim = int(x16.shape[0]), int(x16.shape[1])
    M = _require_codebooks(codebooks, dim, dsub)
    if centre is not None:
        _require_tensor(centre, "centre", (torch.float32,), 1, torch.is_tensor(centre) and tuple(centre.shape) == (dim,), f" [{dim}]")
    out = torch.empty((n, M), dtype=torch.uint8, device=x16.device)
    if n:
        launch("arx_pq_encode", x16.device, x16.data_ptr(), n, dim, int(dsub), None if centre is None else centre.data_ptr(),
                codebooks.data_ptr(), out.data_ptr())
    return out


def lut_device(q16, dsub: int, codebooks):
    """`arx_pq_lut` on the current stream: `q16` fp16 device [nq, dim] -> uint8 device [nq, M, 256]."""
    import torch
    _require_tensor(q16, "queries", (torch.float16,), 2)
    nq, dim = int(q16.shape[0]), int(q16.shape[1])
    M = _require_codebooks(codebooks, dim, dsub)
    out = torch.empty((nq, M, N_CODES), dtype=torch.uint8, device=q16.device)
    if nq:
        launch("arx_pq_lut", q16.device, q16.data_ptr(), nq, dim, int(dsub), codebooks.data_ptr(), out.data_ptr())
    return out


def candidates_device(codes, lut, dsub: int, n_candidates: int, allow=None, rows_per_block: Optional[int] = None, ws=None,
                      want_sum: bool = True):
    """`arx_pq_candidates` (or, with `rows_per_block` given, `arx_pq_candidates_tuned`) on the current stream.  `codes` uint8 device
    [n_rows, M], `lut` uint8 device [nq, M, 256], `allow` int64 / uint64 device [ceil(n_rows / 64)] or None -> (cand int32 [nq, R],
    sum int32 [nq, R] or None, count int64 [nq]) on the device.  `ws`: a device uint8 tensor used if it is large enough.  The library
    checks the contract; a tensor of another kind is a ValueError naming it."""
    import torch
    _require_tensor(codes, "codes", (torch.uint8,), 2)
    n_rows, M, R = int(codes.shape[0]), int(codes.shape[1]), int(n_candidates)
    _require_tensor(lut, "lut", (torch.uint8,), 3, torch.is_tensor(lut) and lut.dim() == 3 and tuple(lut.shape[1:]) == (M, N_CODES),
                    f" [nq, {M}, {N_CODES}]")
    nq = int(lut.shape[0])
    if allow is not None:
        _require_tensor(allow, "allow", (torch.int64, torch.uint64), 1,
                        torch.is_tensor(allow) and allow.dim() == 1 and allow.shape[0] == (n_rows + 63) // 64,
                        f" [{(n_rows + 63) // 64}] (one bit per row of the {n_rows})")
    dev = lut.device
    cand = torch.empty((nq, max(R, 0)), dtype=torch.int32, device=dev)
    sums = torch.empty((nq, max(R, 0)), dtype=torch.int32, device=dev) if want_sum else None
    count = torch.empty((nq,), dtype=torch.int64, device=dev)
    if nq == 0:
        return cand, sums, count
    dim = M * int(dsub)
    if ws is None:                                               # (a workspace given is the caller's figure: the library checks its size)
        ws = torch.empty(_workspace_bytes(n_rows, nq, dim, dsub, R), dtype=torch.uint8, device=dev)
    args = [codes.data_ptr() if n_rows else None, n_rows, dim, int(dsub), lut.data_ptr(), nq, None if allow is None else allow.data_ptr(), R,
            cand.data_ptr(), None if sums is None else sums.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size()]
    if rows_per_block is None:
        launch("arx_pq_candidates", dev, *args)
    else:
        launch("arx_pq_candidates_tuned", dev, *args, int(rows_per_block))
    return cand, sums, count


def train(X16, dsub: int, centre=None, iters: int = 10, seed: int = 0, n_codes: int = N_CODES):
    """Codebooks f32 device [M, 256, dsub] by Lloyd's algorithm over the sample `X16` (fp16 device [n, dim], n >= 1), every subspace
    on its own.  The assign step IS `arx_pq_encode` (one definition of "nearest"); the update is the per-(m, code) mean of the centred
    rows, an empty code keeps its centroid.  The initial centroids are min(n, n_codes) rows chosen by a seeded numpy permutation
    (`topics.default_init_rows`); the remaining entries of the 256 repeat them, which is legal because ties go to the lowest code.
    Training is plumbing: its floats need not be reproducible.  A ValueError if a codebook value is not finite."""
    import torch
    from .topics import default_init_rows
    _require_tensor(X16, "rows", (torch.float16,), 2)
    n, dim = int(X16.shape[0]), int(X16.shape[1])
    M = check_dsub(dim, dsub)
    if n < 1:
        raise ValueError("train needs at least one row")
    if not _is_int(n_codes) or not (1 <= n_codes <= N_CODES) or not _is_int(iters) or iters < 0:
        raise ValueError(f"n_codes={n_codes!r} must be in [1, {N_CODES}] and iters={iters!r} >= 0")
    dev = X16.device
    V = X16.float() if centre is None else X16.float() - centre[None, :]
    V = V.reshape(n, M, dsub)
    kk = min(n, int(n_codes))
    first = torch.from_numpy(default_init_rows(n, kk, seed)).to(dev)
    repeat = torch.arange(N_CODES, device=dev) % kk              # entries kk .. 255 repeat the first kk, before and after every update
    cb = V[first[repeat]].permute(1, 0, 2).contiguous()          # [M, 256, dsub]
    flat_m = (torch.arange(M, device=dev, dtype=torch.int64) * N_CODES)[None, :]
    for _ in range(int(iters)):
        codes = encode_device(X16, dsub, centre, cb)
        idx = (codes.to(torch.int64) + flat_m).reshape(-1)
        sums = torch.zeros((M * N_CODES, dsub), dtype=torch.float32, device=dev).index_add_(0, idx, V.reshape(n * M, dsub))
        cnt = torch.bincount(idx, minlength=M * N_CODES).to(torch.float32)[:, None]
        mean = (sums / cnt.clamp(min=1.0)).reshape(M, N_CODES, dsub)
        cb = torch.where(cnt.reshape(M, N_CODES, 1) > 0, mean, cb)[:, repeat].contiguous()
    if not bool(torch.isfinite(cb).all()):
        raise ValueError("training gave a codebook value that is not finite (do the rows hold NaN or inf?)")
    return cb


class PqIndex(CodeIndex):
    """The PQ codes of a `ShardIndex`'s rows: `codes` (uint8 device [n_rows, dim / dsub]), `codebooks` (f32 device [M, 256, dsub]) and
    `centre` (f32 device [dim] or None), all kept as given: nothing recomputes them."""

    def __init__(self, index, codes, codebooks, centre, dsub: int):
        super().__init__(index, codes, centre)
        self.codebooks, self.dsub = codebooks, int(dsub)

    @classmethod
    def build(cls, index, dsub: int = 8, centre="mean", codebooks=None, train_rows: int = 65536, iters: int = 10, seed: int = 0) -> "PqIndex":
        """Encode the rows of `index`.  `centre`: "mean" (the f32 column mean of the rows, computed once here and stored), None (0) or
        an f32 array / tensor [dim].  `codebooks`: f32 [M, 256, dsub] kept unchanged, or None: trained here (`train`) on at most
        `train_rows` rows chosen by a seeded numpy permutation.  ValueError before any launch: a bad dim / dsub / M, n_rows >= 2^31, a
        centre or codebooks of another shape, codebooks with a value that is not finite, nothing to train on."""
        import torch
        dim, n = int(index.dim), int(index.n_rows)
        check_dsub(dim, dsub)
        centre = cls.check_build(index, centre)
        if codebooks is not None:
            codebooks = check_codebooks(codebooks, dim, dsub)
        elif n == 0:
            raise ValueError("an empty index has no rows to train the codebooks on: pass codebooks")
        elif not _is_int(train_rows) or train_rows < 1:
            raise ValueError(f"train_rows={train_rows!r} must be a positive integer")
        c = cls.device_centre(index, centre)
        dev, rows = index.corpus.device, index.corpus[:n]
        if codebooks is None:
            sample = rows
            if n > train_rows:
                pick = np.sort(np.random.default_rng(seed).permutation(n)[:train_rows]).astype(np.int64)
                sample = rows[torch.from_numpy(pick).to(dev)].contiguous()
            cb = train(sample.contiguous(), dsub, c, iters=iters, seed=seed)
        else:
            cb = torch.from_numpy(codebooks).to(dev)
        return cls(index, encode_device(rows.contiguous(), dsub, c, cb), cb, c, dsub)

    def encode(self, x16):
        """The codes of fp16 device rows [n, dim] under the index's codebooks and centre."""
        return encode_device(x16.contiguous(), self.dsub, self.centre, self.codebooks)

    encode_rows = encode

    def lut(self, q16):
        """The byte tables of fp16 device queries [nq, dim]."""
        return lut_device(q16.contiguous(), self.dsub, self.codebooks)

    def check(self, k, n_candidates) -> None:
        check_args(k, n_candidates, int(self.index.dim), self.dsub)

    def _scan_bytes(self, nq: int, R: int) -> int:
        return _workspace_bytes(int(self.codes.shape[0]), nq, int(self.index.dim), self.dsub, int(R))

    def candidates(self, q16, n_candidates: int, allow=None, rows_per_block: Optional[int] = None):
        """(cand int32 [nq, R], sum int32 [nq, R], count int64 [nq]) on the device: per query the first `n_candidates` visible rows by
        (table sum desc, row asc), padded with -1; rows are local.  `allow`: the row bitmap `ShardIndex.search(allow=...)` takes, or
        None."""
        self.check(None, n_candidates)
        self._require_rows()
        return candidates_device(self.codes, self.lut(q16), self.dsub, int(n_candidates), allow=allow, rows_per_block=rows_per_block,
                                 ws=self._workspace(int(q16.shape[0]), n_candidates))
