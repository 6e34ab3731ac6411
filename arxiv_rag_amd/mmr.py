"""Maximal marginal relevance over a query's search candidates (INTEGRATION.md "MMR"): a diversified re-ordering of the n <= 32 rows
the exact top-k search returned, computed where the rows already are.

* `mmr_reference_f64` — the definition in numpy float64 (tests, and the host path `tools/mmr_bench.py` times).
* `mmr_select` — gather the candidates' fp16 rows out of this rank's shard (`arx_gather_rows`), add the ranks' buffers up
  (`exchange_candidate_rows`), run the greedy pass (`arx_mmr_select`); returns `(order, mmr)` on the device.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

MAX_CANDIDATES = 32        # slots of arx_mmr_select (one 32 x 32 Gram tile) = the search's k limit


def mmr_reference_f64(q, cand, ids, m: int, lam: float, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """The definition, per query, in float64: q [Q, D], cand [Q, n, D], ids [Q, n] (a slot with id < 0 is never picked), 1 <= m <= n,
    lam in [0, 1] -> (order int32 [Q, m] of slot positions, mmr float64 [Q, m] = the objective at the time of the pick; (-1, -inf) in
    the tail when fewer than m slots are valid).
    rel[i] = cos(q, c_i), sim[i][j] = cos(c_i, c_j), 0 where a norm is 0; pick 0 = argmax lam rel[i]; pick t = argmax over valid unpicked i
    of lam rel[i] - (1 - lam) max_{j picked} sim[i][j]; ties to the lower slot.
    `dtype`: the arithmetic's precision; float64 is the definition, float32 what a caller's own host loop would run (tools/mmr_bench.py)."""
    q = np.asarray(q, dtype)
    cand = np.asarray(cand, dtype)
    ids = np.asarray(ids)
    if q.ndim == 1:
        q, cand, ids = q[None], cand[None], ids[None]
    nq, n, _ = cand.shape
    if not (1 <= m <= n):
        raise ValueError(f"m={m} must be in [1, {n}]")
    if not (0.0 <= lam <= 1.0):
        raise ValueError(f"lam={lam} must be in [0, 1]")
    order = np.full((nq, m), -1, np.int32)
    val = np.full((nq, m), -np.inf, np.float64)
    for b in range(nq):
        rel, sim = cosines_f64(q[b], cand[b], dtype)
        free = ids[b] >= 0
        worst = np.full(n, -np.inf, dtype)
        for t in range(m):
            if not free.any():
                break
            obj = dtype(lam) * rel if t == 0 else dtype(lam) * rel - dtype(1.0 - lam) * worst
            pick = int(np.argmax(np.where(free, obj, -np.inf)))      # (first maximum = the lower slot; a valid objective is finite)
            order[b, t], val[b, t] = pick, obj[pick]
            free[pick] = False
            worst = np.maximum(worst, sim[:, pick])
    return order, val


def cosines_f64(q, cand, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """(rel [n], sim [n, n]) of one query in float64 (or `dtype`): true cosines, 0 where a norm is 0."""
    q = np.asarray(q, dtype)
    cand = np.asarray(cand, dtype)
    qq = float(q @ q)
    nn = np.einsum("id,id->i", cand, cand)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where((nn > 0) & (qq > 0), (cand @ q) / np.sqrt(qq * nn), 0.0).astype(dtype)
        sim = np.where((nn[:, None] > 0) & (nn[None, :] > 0), (cand @ cand.T) / np.sqrt(nn[:, None] * nn[None, :]), 0.0).astype(dtype)
    return rel, sim


def exchange_candidate_rows(rows, group=None):
    """Sum the ranks' `[Q, n, D]` fp16 candidate buffers (RCCL `all_reduce` on device tensors, gloo on CPU tensors): exactly one rank
    holds each row and the others hold zeros there, so the sum is exact (a -0 of the owner may come out as +0: the same number) and every
    rank ends up with all the rows.  Without an
    initialised process group: the identity.  At world size 1 the collective still runs (one code path, as `search_distributed`)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return rows
    rows = rows.contiguous()
    dist.all_reduce(rows, op=dist.ReduceOp.SUM, group=group)
    return rows


def gather_rows(index, ids):
    """fp16 [..., D] (device) = the shard rows of `index` named by the global `ids` (device int64, any shape), zeros where the row is
    not this shard's (`arx_gather_rows`)."""
    import torch
    from . import _lib
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
    out = torch.empty(tuple(ids.shape) + (index.dim,), dtype=torch.float16, device=ids.device)
    _lib.check(index.lib.arx_gather_rows(index.corpus.data_ptr() if index.n_rows else None, index.n_rows, index.dim, index.idx_base,
                                         ids.data_ptr(), ids.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "arx_gather_rows")
    return out


def mmr_select(index, q_f16, ids, m: int, lam: float, group=None):
    """`index`: this rank's `ShardIndex`; q fp16 [Q, D] and ids int64 [Q, n] on its device (the queries and the id list of a search over
    it, `search_distributed` under a process group) -> (order int32 [Q, m], mmr f32 [Q, m]) on the device.
    Gather (each rank the rows it owns), exchange (`exchange_candidate_rows`), select (`arx_mmr_select`).  No host synchronisation."""
    import torch
    from . import _lib
    assert q_f16.is_cuda and q_f16.dtype == torch.float16 and q_f16.dim() == 2 and q_f16.is_contiguous() and q_f16.shape[1] == index.dim
    assert ids.dim() == 2 and ids.shape[0] == q_f16.shape[0]
    nq, n = ids.shape
    ids = ids.contiguous()
    rows = exchange_candidate_rows(gather_rows(index, ids), group)
    order = torch.empty((nq, m), dtype=torch.int32, device=ids.device)
    val = torch.empty((nq, m), dtype=torch.float32, device=ids.device)
    _lib.check(index.lib.arx_mmr_select(q_f16.data_ptr(), rows.data_ptr(), ids.data_ptr(), nq, n, index.dim, m, float(lam), order.data_ptr(),
                                        val.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_mmr_select")
    return order, val
