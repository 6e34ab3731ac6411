"""Binary-code search: rank every row by the Hamming distance between sign bits, rescore the best `n_candidates` exactly
(`arx_binary_pack`, `arx_binary_candidates`, include/arx.h; INTEGRATION.md "Binary-code search").

    bi = BinaryIndex.build(index, centre="mean")                        # index: a ShardIndex; one pack of its rows, no training
    scores, ids, count = bi.search(q, k=10, n_candidates=128)          # q: fp16 device [nq, dim]

A code keeps one bit per dimension, `(float)x[j] > centre[j]`: dim / 8 bytes per row, 1/16 of the fp16 row.  `candidates` is the exact
list C(q) of the first `n_candidates` visible rows by (Hamming distance asc, row asc): distances are integers, so the list is defined
bit for bit.  `search` is the exact top-k of C(q): the candidate lists go to `arx_ivf_search` as inverted lists (`ivf._launch`), so
every returned score has the bits of `ShardIndex.search` and the order is (score desc, row asc); the answer equals
`ShardIndex.search(allow=bitmap of C(q))`.  Which rows get scored is the only approximation; `n_candidates >= ` the visible rows is
the exact search.

`codes.launch` is the one place this module launches anything through; the workspace sizes (`_workspace_bytes`, and
`arx_ivf_workspace_bytes` for the rescore) are host arithmetic.  What the index shares with `pq.PqIndex` is `codes.CodeIndex`: the
lifecycle of the code array, the cached workspaces, `search` and the rescore (`codes.rescore_candidates`, whose launch is
`ivf._launch`).  `pack_host`, `candidates_host` and `search_host` restate the definitions with numpy (for the tests; the product path
never calls them); `check_args` and `check_query_with_binary` are the refusals; a tensor of the wrong kind is a ValueError too.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .codes import MAX_CANDIDATES, MAX_K, RESCORE_QUERIES, CodeIndex, _is_int, check_candidate_args, check_centre, launch, rescore_host  # noqa: F401

MAX_DIM = 8192


def check_dim(dim) -> None:
    if not _is_int(dim) or dim < 64 or dim % 64 or dim > MAX_DIM:
        raise ValueError(f"dim={dim!r} must be a multiple of 64 in [64, {MAX_DIM}] (one 64-bit word per 64 dimensions)")


def check_args(k, n_candidates, dim=None) -> None:
    """The refusals of `BinaryIndex.search` / `candidates` (k = None), each a ValueError before anything is launched."""
    check_candidate_args(k, n_candidates)
    if dim is not None:
        check_dim(dim)


def check_query_with_binary(binary_candidates, *, has_index: bool, per_query_filters: bool = False, hybrid_alpha=None, group_by=None,
                            min_score=None, nprobe=None, world: int = 1, n_width: int = 1, pq_candidates=None) -> None:
    """The refusals of `query(binary_candidates=...)`, `retrieve` and `search_queries`, each a ValueError naming the part, before any
    launch (`modes.check_mode`).  `n_width`: the rows the search returns per query (the reranker's or MMR's candidates, else n_results)."""
    from .modes import check_mode
    check_mode("binary_candidates", binary_candidates, has_index=has_index, per_query=per_query_filters, hybrid_alpha=hybrid_alpha,
               group_by=group_by, min_score=min_score, world=world, n_width=n_width, others={"nprobe": nprobe, "pq_candidates": pq_candidates})


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def pack_host(X, centre=None) -> np.ndarray:
    """uint64 [n, dim / 64]: what `arx_binary_pack` writes.  `X` fp16 [n, dim]; `centre` None (0) or f32 [dim].  Bit j & 63 of word
    j >> 6 is `float32(x[j]) > centre[j]` (False for NaN)."""
    X = np.asarray(X)
    if X.dtype != np.float16 or X.ndim != 2:
        raise ValueError("X must be an fp16 [n, dim] array")
    check_dim(int(X.shape[1]))
    c = np.zeros(X.shape[1], np.float32) if centre is None else np.asarray(centre, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        bits = X.astype(np.float32) > c[None, :]
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").astype(np.uint64, copy=False).reshape(X.shape[0], X.shape[1] // 64)


def _visible(allow, n_rows: int) -> np.ndarray:
    """bool [n_rows] from None, a bool mask or bitmap words (bits at or beyond n_rows ignored)."""
    if allow is None:
        return np.ones(n_rows, bool)
    allow = np.asarray(allow)
    if allow.dtype == bool:
        return allow[:n_rows].copy()
    from .mutation import unpack_rows
    return unpack_rows(allow, n_rows)


def distances_host(codes, qcodes) -> np.ndarray:
    """int32 [nq, n]: the Hamming distances of every (query, row) pair of uint64 code arrays."""
    codes, qcodes = np.ascontiguousarray(codes, dtype=np.uint64), np.ascontiguousarray(qcodes, dtype=np.uint64)
    out = np.zeros((qcodes.shape[0], codes.shape[0]), np.int32)
    for q in range(qcodes.shape[0]):
        x = np.ascontiguousarray(codes ^ qcodes[q][None, :])
        out[q] = np.unpackbits(x.view(np.uint8), axis=1).sum(axis=1, dtype=np.int32) if codes.shape[0] else 0
    return out


def candidates_host(codes, qcodes, n_candidates: int, allow=None):
    """(cand int32 [nq, R], dist int32 [nq, R], count int64 [nq]): what `arx_binary_candidates` returns, bit for bit.  `allow`: None,
    a bool mask [n_rows] or bitmap words."""
    codes, qcodes = np.asarray(codes), np.asarray(qcodes)
    n, nq, R = codes.shape[0], qcodes.shape[0], int(n_candidates)
    rows = np.nonzero(_visible(allow, n))[0]
    d = distances_host(codes[rows], qcodes)
    cand, dist, count = np.full((nq, R), -1, np.int32), np.full((nq, R), -1, np.int32), np.zeros(nq, np.int64)
    for q in range(nq):
        best = np.lexsort((rows, d[q]))[:R]                      # distance asc, row asc
        m = best.shape[0]
        cand[q, :m], dist[q, :m], count[q] = rows[best], d[q][best], m
    return cand, dist, count


def search_host(X, codes, qcodes, Q, k: int, n_candidates: int, allow=None):
    """(scores f32 [nq, k], ids int64 [nq, k], count int64 [nq]): what `BinaryIndex.search` returns with idx_base = 0, bit for bit:
    `codes.rescore_host` of `candidates_host`'s lists."""
    cand, _, count = candidates_host(codes, qcodes, n_candidates, allow)
    return rescore_host(X, Q, cand, count, k)


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def _require_tensor(t, what: str, dtypes, ndim: int, shape_ok: bool = True, detail: str = "") -> None:
    """ValueError naming `what` unless `t` is a dense device tensor of one of `dtypes` with `ndim` dimensions (and `shape_ok`)."""
    import torch
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in dtypes and t.dim() == ndim and t.is_contiguous() and shape_ok):
        names = " / ".join(str(d).replace("torch.", "") for d in dtypes)
        got = f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be a contiguous {names} device tensor with {ndim} dimension{'s' if ndim > 1 else ''}{detail}, not {got}")


def _workspace_bytes(n_rows: int, nq: int, dim: int, R: int) -> int:
    """`arx_binary_workspace_bytes` (host arithmetic, nothing is launched); outside the limits an `ArxError`."""
    from . import _lib
    need = _lib.load().arx_binary_workspace_bytes(int(n_rows), max(int(nq), 1), int(dim), int(R))
    if need < 0:
        raise _lib.ArxError(f"arx_binary_candidates: unsupported shape n_rows={n_rows} nq={nq} dim={dim} n_candidates={R}")
    return int(need)


def pack_device(x16, centre=None):
    """`arx_binary_pack` on the current stream: `x16` fp16 device [n, dim] (dense), `centre` f32 device [dim] or None -> int64 device
    [n, dim / 64] (the words' bits are the uint64 codes')."""
    import torch
    _require_tensor(x16, "rows / queries", (torch.float16,), 2)
    n, dim = int(x16.shape[0]), int(x16.shape[1])
    check_dim(dim)
    if centre is not None:
        _require_tensor(centre, "centre", (torch.float32,), 1, torch.is_tensor(centre) and tuple(centre.shape) == (dim,), f" [{dim}]")
    out = torch.empty((n, dim // 64), dtype=torch.int64, device=x16.device)
    if n:
        launch("arx_binary_pack", x16.device, x16.data_ptr(), n, dim, None if centre is None else centre.data_ptr(), out.data_ptr())
    return out


def candidates_device(codes, qcodes, n_candidates: int, allow=None, rows_per_block: Optional[int] = None, ws=None, want_dist: bool = True):
    """`arx_binary_candidates` (or, with `rows_per_block` given, `arx_binary_candidates_tuned`) on the current stream.  `codes` int64 /
    uint64 device [n_rows, W], `qcodes` the same [nq, W], `allow` int64 / uint64 device [ceil(n_rows / 64)] or None -> (cand int32
    [nq, R], dist int32 [nq, R] or None, count int64 [nq]) on the device.  `ws`: a device uint8 tensor used if it is large enough.  The
    library checks the contract; a tensor of another kind is a ValueError naming it."""
    import torch
    words = (torch.int64, torch.uint64)
    _require_tensor(codes, "codes", words, 2)
    _require_tensor(qcodes, "qcodes", words, 2, torch.is_tensor(qcodes) and qcodes.dim() == 2 and qcodes.shape[1] == codes.shape[1],
                    f" [nq, {int(codes.shape[1])}]")
    n_rows, W, nq, R = int(codes.shape[0]), int(codes.shape[1]), int(qcodes.shape[0]), int(n_candidates)
    if allow is not None:
        _require_tensor(allow, "allow", words, 1, torch.is_tensor(allow) and allow.dim() == 1 and allow.shape[0] == (n_rows + 63) // 64,
                        f" [{(n_rows + 63) // 64}] (one bit per row of the {n_rows})")
    dev = qcodes.device
    cand = torch.empty((nq, max(R, 0)), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, max(R, 0)), dtype=torch.int32, device=dev) if want_dist else None
    count = torch.empty((nq,), dtype=torch.int64, device=dev)
    if nq == 0:
        return cand, dist, count
    if ws is None:                                               # (a workspace given is the caller's figure: the library checks its size)
        ws = torch.empty(_workspace_bytes(n_rows, nq, W * 64, R), dtype=torch.uint8, device=dev)
    args = [codes.data_ptr() if n_rows else None, n_rows, W * 64, qcodes.data_ptr(), nq, None if allow is None else allow.data_ptr(), R,
            cand.data_ptr(), None if dist is None else dist.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size()]
    if rows_per_block is None:
        launch("arx_binary_candidates", dev, *args)
    else:
        launch("arx_binary_candidates_tuned", dev, *args, int(rows_per_block))
    return cand, dist, count


class BinaryIndex(CodeIndex):
    """The sign-bit codes of a `ShardIndex`'s rows: `codes` (int64 device [n_rows, dim / 64]) and `centre` (f32 device [dim] or None),
    kept as given."""

    @classmethod
    def build(cls, index, centre="mean") -> "BinaryIndex":
        """Pack the rows of `index`.  `centre`: "mean" (the f32 column mean of the rows, computed once here and stored), None (0) or
        an f32 array / tensor [dim].  ValueError before any launch: dim not a multiple of 64 in [64, 8192], n_rows >= 2^31, a centre
        of another shape."""
        check_dim(int(index.dim))
        c = cls.device_centre(index, cls.check_build(index, centre))
        return cls(index, pack_device(index.corpus[:int(index.n_rows)], c), c)

    def pack(self, x16):
        """The codes of fp16 device rows or queries [n, dim] under the index's centre."""
        return pack_device(x16.contiguous(), self.centre)

    encode_rows = pack

    def check(self, k, n_candidates) -> None:
        check_args(k, n_candidates, int(self.index.dim))

    def _scan_bytes(self, nq: int, R: int) -> int:
        return _workspace_bytes(int(self.codes.shape[0]), nq, int(self.index.dim), int(R))

    def candidates(self, q16, n_candidates: int, allow=None, rows_per_block: Optional[int] = None):
        """(cand int32 [nq, R], dist int32 [nq, R], count int64 [nq]) on the device: per query the first `n_candidates` visible rows by
        (Hamming distance asc, row asc), padded with -1; rows are local.  `allow`: the row bitmap `ShardIndex.search(allow=...)`
        takes, or None."""
        self.check(None, n_candidates)
        self._require_rows()
        return candidates_device(self.codes, self.pack(q16), int(n_candidates), allow=allow, rows_per_block=rows_per_block,
                                 ws=self._workspace(int(q16.shape[0]), n_candidates))
