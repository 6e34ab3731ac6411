"""Topic clustering: spherical k-means over fp16 rows on the device (`arx_cluster_assign`, `arx_cluster_sums`, `arx_cluster_finish`,
include/arx.h; INTEGRATION.md "Topics").

    res = kmeans(X, n_clusters=64, iters=20, seed=0)          # X: fp16 device tensor [n, dim]
    res["labels"], res["sizes"], res["centroids"], res["objective"]

A Lloyd iteration is an assign and an update:
  assign   label[i] = the lowest centroid that maximises the exact score of row i (`exact_scores_host` is the definition), score[i]
           that f32 value: `arx_cluster_assign`, an fp16 MFMA pass whose certificate sends near ties to an exhaustive exact pass.
           `assign="search"` computes the same bits as `ShardIndex(centroids_f16, prefilter=None).search(X[i], k=1)`: the exact search
           with the roles turned round (the centroids are the shard, the rows the queries, in batches of at most 65 536).
  update   the members of every cluster are summed in one fixed order (`arx_cluster_sums`: runs of 256 members in ascending row order,
           then the runs in order, every add a plain f32 add) and normalised (`arx_cluster_finish`).  No float atomics anywhere, so the
           centroids are the same bits on every run and under every launch shape.
The member list comes from torch on the device: a stable sort of the labels is `order`, `bincount` the sizes, their cumulative sum
`start`.  Each iteration reads one number back, how many labels the assign changed; the loop stops after `iters` assigns or once an
assign changes none.  The result holds the labels of the last assign and the centroids that assign used, so sizes and objective
describe one state.

Initial centroids: `init` (f32 [C, dim]), or rows `numpy.random.default_rng(seed).choice(n, C, replace=False)` of X, sorted ascending.
Identical rows then give identical centroids; every row ties between them, the lower one takes them all, and the higher one is
empty and keeps its value.  Empty clusters are not relocated; a kept centroid can still win rows in a later assign (one that is a
row of X scores 1 against that row, more than the lower centroid does once the update has moved it).

`predict(X, centroids)` labels rows against given centroids with the same kernel (new rows after a fit, `HipCollection.assign_topics`).

`exact_scores_host`, `assign_exact_host`, `sums_host`, `finish_host` and `kmeans_host` restate the definitions with numpy (for the tests; the product path never calls them).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

RUN = 256                       # members of a run of the ordered sum
MAX_CLUSTERS, MAX_DIM = 4096, 8192
ASSIGN_BATCH = 65536            # rows per search call of the assign
UNIT_NORM_BOUND = 1.0 + 1.0 / 512.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def check_args(n: int, dim: int, n_clusters, iters, init=None) -> Optional[np.ndarray]:
    """Every refusal of `kmeans`, each a ValueError before anything is launched.  -> `init` as a contiguous f32 array, or None."""
    if dim < 64 or dim > MAX_DIM or dim % 64 != 0:
        raise ValueError(f"dim={dim} must be a multiple of 64 in [64, {MAX_DIM}] (the contract of arx_cluster_sums)")
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or not (1 <= n_clusters <= min(n, MAX_CLUSTERS)):
        raise ValueError(f"n_clusters={n_clusters!r} must be an integer in [1, min(rows, {MAX_CLUSTERS})] = [1, {min(n, MAX_CLUSTERS)}]")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
        raise ValueError(f"iters={iters!r} must be an integer >= 1")
    if init is None:
        return None
    a = np.asarray(init)
    if a.shape != (int(n_clusters), dim) or a.dtype.kind not in "fiu":
        raise ValueError(f"init must be a numeric [n_clusters, dim] = [{int(n_clusters)}, {dim}] array, got shape {tuple(a.shape)}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError("init holds a value that is not finite")
    return a


def default_init_rows(n: int, n_clusters: int, seed: int) -> np.ndarray:
    """The rows of X the default initial centroids are: int64 [n_clusters], ascending."""
    return np.sort(np.random.default_rng(seed).choice(n, n_clusters, replace=False)).astype(np.int64)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def clamp_starts(start, n_members: int) -> np.ndarray:
    """`start` clamped into [0, n_members] and made non-decreasing, as the kernels read it."""
    return np.maximum.accumulate(np.clip(np.asarray(start, dtype=np.int64), 0, n_members))


def sums_host(X, order, start) -> np.ndarray:
    """f32 [C, dim]: what `arx_cluster_sums` leaves, bit for bit.  `X` fp16 [n_rows, dim], `order` the member rows sorted by
    (cluster, row), `start` int64 [C + 1].  Per run of 256 entries `np.cumsum(..., dtype=np.float32)[-1]`, then the same over the
    partials; an entry outside [0, n_rows) keeps its place in its run and adds nothing."""
    X = np.asarray(X)
    order = np.asarray(order, dtype=np.int64)
    n_rows, dim = X.shape
    s = clamp_starts(start, order.shape[0])
    out = np.zeros((s.shape[0] - 1, dim), dtype=np.float32)
    for c in range(s.shape[0] - 1):
        partials = []
        for a in range(int(s[c]), int(s[c + 1]), RUN):
            rows = order[a:min(a + RUN, int(s[c + 1]))]
            rows = rows[(rows >= 0) & (rows < n_rows)]
            if rows.size == 0:
                partials.append(np.zeros(dim, np.float32))
            else:
                partials.append(np.cumsum(X[rows].astype(np.float32), axis=0, dtype=np.float32)[-1])
        if partials:
            out[c] = np.cumsum(np.stack(partials), axis=0, dtype=np.float32)[-1]
    return out


def sum_squares_host(S) -> np.ndarray:
    """f32 [C]: the sum of squares of every row of `S` (f32 [C, dim], dim % 64 == 0) in the order `arx_cluster_finish` fixes: lane l of
    64 adds S[d]^2 over d = l, l + 64, ... ascending, then six butterfly steps v_l + v_(l ^ o), o = 32 .. 1."""
    S = np.asarray(S, dtype=np.float32)
    C, dim = S.shape
    sq = (S * S).reshape(C, dim // 64, 64)
    v = np.cumsum(sq, axis=1, dtype=np.float32)[:, -1, :]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def finish_host(sums, start, prev):
    """(f32 [C, dim], fp16 [C, dim]): what `arx_cluster_finish` leaves, bit for bit: S / sqrt(sum of squares) in f32, `prev` for a
    cluster that is empty or whose norm is 0 or not finite; the fp16 copy rounded to nearest even."""
    S = np.asarray(sums, dtype=np.float32)
    prev = np.asarray(prev, dtype=np.float32)
    s = np.maximum.accumulate(np.maximum(np.asarray(start, dtype=np.int64), 0))
    with np.errstate(all="ignore"):
        norm = np.sqrt(sum_squares_host(S))
        keep = (s[1:] == s[:-1]) | ~(norm > 0) | ~np.isfinite(norm)
        out = np.where(keep[:, None], prev, S / np.where(keep, np.float32(1), norm)[:, None]).astype(np.float32)
        return out, out.astype(np.float16)


def members_host(labels, n_clusters: int):
    """(order int32, start int64 [C + 1], sizes int64 [C]) of int labels in [0, C): rows sorted by (label, row)."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable").astype(np.int32)
    sizes = np.bincount(labels, minlength=n_clusters).astype(np.int64)
    return order, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), sizes


def assign_host(X, centroids_f16):
    """(labels int32 [n], scores f64 [n]): the nearest centroid of every row by the float64 dot product of the fp16 values, ties to
    the lower centroid.  The definition the device assign (an exact search) answers; its scores are the search's f32 bits."""
    sc = np.asarray(X, dtype=np.float64) @ np.asarray(centroids_f16, dtype=np.float64).T
    labels = np.argmax(sc, axis=1).astype(np.int32)           # (argmax returns the first maximum: the lower centroid)
    return labels, sc[np.arange(sc.shape[0]), labels]


def exact_scores_host(X, C16) -> np.ndarray:
    """f32 [n, C]: `exact_row_score` (csrc/exact_score.h) of every (centroid, row) pair, bit for bit.  `X` fp16 [n, dim], `C16` fp16
    [C, dim], dim % 64 == 0.  Lane l of 8 takes the 16-byte chunks l, l + 8, ... in ascending order and keeps two chains, a0 over the
    even and a1 over the odd elements of a chunk; then a0 + a1 and the butterfly v_l + v_(l ^ o), o = 4, 2, 1.  An fp16 x fp16
    product is exact in f32 (22 significant bits, exponents from 2^-48 to 2^32), so the kernel's `fmaf(c, q, a)`, one rounding of
    a + c q, equals the f32 sum `a + c * q` computed here.  Every pair is computed on its own: the bits of a pair do not depend on
    what else is in the batch."""
    X, Cn = np.asarray(X), np.asarray(C16)
    if X.dtype != np.float16 or Cn.dtype != np.float16 or X.ndim != 2 or Cn.ndim != 2 or X.shape[1] != Cn.shape[1] or X.shape[1] % 64:
        raise ValueError("X and C16 must be fp16 [n, dim] and [C, dim] arrays with dim % 64 == 0")
    n, dim = X.shape
    C, G = Cn.shape[0], dim // 64
    xf = X.astype(np.float32).reshape(n, G, 8, 4, 2)            # [row, chunk round, lane, element pair, even / odd]
    cf = Cn.astype(np.float32).reshape(C, G, 8, 4, 2)
    out = np.empty((n, C), np.float32)
    step = max(1, (1 << 21) // (C * 16))
    lane = np.arange(8)
    for a in range(0, n, step):
        xb = xf[a:a + step]
        acc = np.zeros((xb.shape[0], C, 8, 2), np.float32)
        for g in range(G):
            for j in range(4):
                acc += xb[:, None, g, :, j, :] * cf[None, :, g, :, j, :]
        v = acc[..., 0] + acc[..., 1]
        for o in (4, 2, 1):
            v = v + v[..., lane ^ o]
        out[a:a + step] = v[..., 0]
    return out


def assign_exact_host(X, C16):
    """(labels int32 [n], scores f32 [n]): what `arx_cluster_assign` and the exact k = 1 search give, bit for bit: the lowest centroid
    that maximises `exact_scores_host`, and that value."""
    sc = exact_scores_host(X, C16)
    labels = np.argmax(sc, axis=1).astype(np.int32)           # (the first maximum: the lower centroid; -0.0 == +0.0 is a tie)
    return labels, sc[np.arange(sc.shape[0]), labels]


def kmeans_host(X, n_clusters: int, iters: int = 20, seed: int = 0, init=None) -> Dict:
    """`kmeans` with numpy in the device's place, from the same definitions (the assign in float64).  `X` fp16 [n, dim] on the host.
    -> the same fields as `kmeans`, numpy arrays, and `labels_history` (the labels of every assign)."""
    X = np.asarray(X)
    if X.dtype != np.float16 or X.ndim != 2:
        raise ValueError("X must be an fp16 [n, dim] array")
    n, dim = X.shape
    init = check_args(n, dim, n_clusters, iters, init)
    c32 = X[default_init_rows(n, n_clusters, seed)].astype(np.float32) if init is None else init
    c16 = c32.astype(np.float16)
    prev = np.full(n, -1, np.int32)
    changed, history = [], []
    for it in range(int(iters)):
        labels, scores = assign_host(X, c16)
        changed.append(int((labels != prev).sum()))
        history.append(labels)
        order, start, sizes = members_host(labels, n_clusters)
        if changed[-1] == 0 or it == iters - 1:
            break
        c32, c16 = finish_host(sums_host(X, order, start), start, c32)
        prev = labels
    return {"centroids": c32, "centroids_f16": c16, "labels": labels, "sizes": sizes, "objective": float(scores.mean()),
            "iterations": len(changed), "changed": changed, "labels_history": history}


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def cluster_sums(X, order, start, n_clusters: int, tuned=None, out=None, ws=None):
    """`arx_cluster_sums` (or, with `tuned = (block_threads, runs_per_block)`, `arx_cluster_sums_tuned`) on the current stream.  `X` fp16
    device [n_rows, dim], `order` int32 device [n_members], `start` int64 device [C + 1] -> f32 device [C, dim].  The library checks
    the contract; a refusal is an `ArxError` naming the field."""
    import torch
    from . import _lib
    lib = _lib.load()
    n_rows, dim = int(X.shape[0]), int(X.shape[1])
    assert X.is_cuda and X.dtype == torch.float16 and X.is_contiguous()
    assert order.is_cuda and order.dtype == torch.int32 and order.is_contiguous() and order.dim() == 1
    assert start.is_cuda and start.dtype == torch.int64 and start.is_contiguous() and start.shape == (n_clusters + 1,)
    n_members = int(order.shape[0])
    need = lib.arx_cluster_sums_workspace_bytes(n_members, n_clusters, dim)
    if need < 0:
        raise _lib.ArxError(f"arx_cluster_sums: unsupported shape n_members={n_members} C={n_clusters} dim={dim}")
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=X.device)
    if out is None:
        out = torch.empty((n_clusters, dim), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        stream = torch.cuda.current_stream(X.device).cuda_stream
        head = (X.data_ptr() if n_rows else None, n_rows, dim, order.data_ptr() if n_members else None, n_members, start.data_ptr(),
                n_clusters, ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr())
        if tuned is None:
            _lib.check(lib.arx_cluster_sums(*head, stream), "arx_cluster_sums")
        else:
            _lib.check(lib.arx_cluster_sums_tuned(*head, int(tuned[0]), int(tuned[1]), stream), "arx_cluster_sums_tuned")
    return out


def cluster_finish(sums, start, prev):
    """`arx_cluster_finish` on the current stream -> (f32 device [C, dim], fp16 device [C, dim])."""
    import torch
    from . import _lib
    C, dim = int(sums.shape[0]), int(sums.shape[1])
    assert sums.is_cuda and sums.dtype == torch.float32 and sums.is_contiguous()
    assert prev.is_cuda and prev.dtype == torch.float32 and prev.is_contiguous() and prev.shape == sums.shape
    assert start.is_cuda and start.dtype == torch.int64 and start.is_contiguous() and start.shape == (C + 1,)
    out32 = torch.empty_like(sums)
    out16 = torch.empty((C, dim), dtype=torch.float16, device=sums.device)
    with torch.cuda.device(sums.device):
        _lib.check(_lib.load().arx_cluster_finish(sums.data_ptr(), start.data_ptr(), prev.data_ptr(), C, dim, out32.data_ptr(), out16.data_ptr(),
                                                  torch.cuda.current_stream(sums.device).cuda_stream), "arx_cluster_finish")
    return out32, out16


def members(labels, n_clusters: int):
    """(order int32, start int64 [C + 1], sizes int64 [C]) of int32 device labels in [0, C), with torch on the device: a stable sort
    gives the rows by (label, row)."""
    import torch
    order = torch.sort(labels, stable=True).indices.to(torch.int32)
    sizes = torch.bincount(labels, minlength=n_clusters)
    start = torch.zeros(n_clusters + 1, dtype=torch.int64, device=labels.device)
    start[1:] = torch.cumsum(sizes, 0)
    return order, start, sizes


def allowed_rows(allow, n_rows: int):
    """int64 device [count]: the rows a bitmap (int64 device words, `where.pack_bitmap`'s convention) allows, ascending."""
    import torch
    bits = (allow[:, None] >> torch.arange(64, dtype=torch.int64, device=allow.device)[None, :]) & 1
    return torch.nonzero(bits.reshape(-1)[:n_rows]).reshape(-1)


def gather(index, rows):
    """fp16 device [count, dim]: shard rows `rows` (int64 device, local) of a `ShardIndex`, in a buffer of their own
    (`arx_gather_rows`)."""
    import torch
    from . import _lib
    out = torch.empty((int(rows.shape[0]), index.dim), dtype=torch.float16, device=index.corpus.device)
    if rows.shape[0]:
        ids = (rows + index.idx_base).contiguous()
        with torch.cuda.device(out.device):
            _lib.check(index.lib.arx_gather_rows(index.corpus.data_ptr(), index.n_rows, index.dim, index.idx_base, ids.data_ptr(), int(ids.numel()),
                                                 out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream), "arx_gather_rows")
    return out


def cluster_assign(X, centroids_f16, norm_bound: float = UNIT_NORM_BOUND, tau_mult: Optional[float] = None, rows_per_block: int = 0,
                   stats=None, ws=None, out=None):
    """`arx_cluster_assign` (or, with `tau_mult` given, `arx_cluster_assign_tuned`) on the current stream.  `X` fp16 device [n, dim],
    `centroids_f16` fp16 device [C, dim] -> (labels int32 [n], scores f32 [n]) on the device.  `stats`: an int64 device tensor [2]
    the call sets to (rows flagged, exact scores of the slow path); `ws`: a device tensor to use as the workspace if it is large
    enough; `out`: (labels, scores) to write into.  The library checks the contract; a refusal is an `ArxError` naming the field."""
    import torch
    from . import _lib
    lib = _lib.load()
    n, dim, C = int(X.shape[0]), int(X.shape[1]), int(centroids_f16.shape[0])
    assert X.is_cuda and X.dtype == torch.float16 and X.is_contiguous()
    assert centroids_f16.is_cuda and centroids_f16.dtype == torch.float16 and centroids_f16.is_contiguous() and centroids_f16.shape[1] == dim
    assert stats is None or (stats.is_cuda and stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() == 2)
    need = lib.arx_cluster_assign_workspace_bytes(n, C, dim)
    if need < 0:
        raise _lib.ArxError(f"arx_cluster_assign: unsupported shape n_rows={n} C={C} dim={dim}")
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need // 4, dtype=torch.int32, device=X.device)
    labels, scores = out if out is not None else (torch.empty(n, dtype=torch.int32, device=X.device),
                                                  torch.empty(n, dtype=torch.float32, device=X.device))
    with torch.cuda.device(X.device):
        stream = torch.cuda.current_stream(X.device).cuda_stream
        head = (X.data_ptr() if n else None, n, dim, centroids_f16.data_ptr(), C, float(norm_bound), labels.data_ptr() if n else None,
                scores.data_ptr() if n else None, None if stats is None else stats.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
        if tau_mult is None and not rows_per_block:
            _lib.check(lib.arx_cluster_assign(*head, stream), "arx_cluster_assign")
        else:
            _lib.check(lib.arx_cluster_assign_tuned(*head, float(tau_mult or 0.0), int(rows_per_block), stream), "arx_cluster_assign_tuned")
    return labels, scores


def assign_workspace(n: int, n_clusters: int, dim: int, device):
    """A workspace `cluster_assign` can reuse for every call of at most `n` rows."""
    import torch
    from . import _lib
    need = _lib.load().arx_cluster_assign_workspace_bytes(n, n_clusters, dim)
    if need < 0:
        raise _lib.ArxError(f"arx_cluster_assign: unsupported shape n_rows={n} C={n_clusters} dim={dim}")
    return torch.empty(need // 4, dtype=torch.int32, device=device)


def assign(X, centroids_f16, norm_bound: float = UNIT_NORM_BOUND, how: str = "kernel", ws=None):
    """(labels int32 [n], scores f32 [n]) on the device: the nearest centroid of every row of `X` by the exact score, ties to the
    lower centroid.  `how="kernel"`: `arx_cluster_assign` (`ws`: a workspace to reuse, `assign_workspace`).  `how="search"`: the exact
    k = 1 search of every row over the centroids, in batches of at most 65 536 rows.  The two give the same bits.  `norm_bound`: a
    bound on the centroids' norms (the certificates scale with it), given by the caller so that no iteration reads it back."""
    import torch
    if how == "kernel":
        return cluster_assign(X, centroids_f16, norm_bound, ws=ws)
    if how != "search":
        raise ValueError(f"how={how!r} must be 'kernel' or 'search'")
    from .index import ShardIndex
    n = int(X.shape[0])
    idx = ShardIndex(centroids_f16, prefilter=None, max_row_norm=norm_bound)
    scores = torch.empty((n, 1), dtype=torch.float32, device=X.device)
    ids = torch.empty((n, 1), dtype=torch.int64, device=X.device)
    for a in range(0, n, ASSIGN_BATCH):
        b = min(n, a + ASSIGN_BATCH)
        idx.search(X[a:b], 1, out=(scores[a:b], ids[a:b]))
    return ids[:, 0].to(torch.int32), scores[:, 0]


_assign_rows = assign            # (`kmeans` has a parameter of that name)


def centroid_norm_bound(c16) -> float:
    """The norm bound `kmeans` and `predict` give the assign: the largest fp16 centroid norm (one host read) with a margin for its
    own rounding, at least the unit-row bound."""
    import torch
    return max(float(c16.to(torch.float32).norm(dim=1).max().item()) * (1.0 + 1e-3), UNIT_NORM_BOUND)


def check_centroids(centroids, dim: int):
    """The refusals of `predict` about its centroids, each a ValueError before anything is launched -> (C, is_fp16)."""
    import torch
    c = centroids
    is_t = torch.is_tensor(c)
    if not is_t:
        c = np.asarray(c)
    if c.ndim != 2 or int(c.shape[1]) != dim:
        raise ValueError(f"centroids must be [C, dim] = [C, {dim}], got shape {tuple(c.shape)}")
    f16, f32 = (torch.float16, torch.float32) if is_t else (np.float16, np.float32)
    if c.dtype not in (f16, f32):
        raise ValueError(f"centroids must be f32 or fp16, got {c.dtype}")
    check_args(MAX_CLUSTERS, dim, int(c.shape[0]), 1)
    if not bool((torch.isfinite(c) if is_t else np.isfinite(c)).all()):
        raise ValueError("centroids hold a value that is not finite")
    return int(c.shape[0]), c.dtype == f16


def predict(X, centroids, norm_bound: Optional[float] = None):
    """Label rows against given centroids: (labels int32 [n], scores f32 [n]) on the device, `label[i]` the lowest centroid that
    maximises the exact score of row i (`assign_exact_host` is the definition), `score[i]` that f32 value.  `X` a dense fp16 device
    tensor [n, dim]; `centroids` f32 or fp16 [C, dim] (numpy or torch, e.g. `kmeans(...)["centroids"]`), f32 rounded to fp16 as `kmeans`
    rounds its own, so `predict(X, res["centroids"])` returns `res["labels"]`.  `norm_bound`: a bound on the fp16 centroids' norms;
    None measures it (one host read).  ValueError before any launch: the refusals of `check_args` about dim and C, centroids of the
    wrong shape or dtype or with a value that is not finite, a `norm_bound` that is not positive and finite."""
    import torch
    if not (torch.is_tensor(X) and X.dtype == torch.float16 and X.dim() == 2 and X.is_contiguous()):
        raise ValueError("X must be a dense fp16 device tensor [n, dim]")
    dim = int(X.shape[1])
    check_args(MAX_CLUSTERS, dim, 1, 1)
    check_centroids(centroids, dim)
    if norm_bound is not None and not (isinstance(norm_bound, (int, float, np.floating)) and 0 < float(norm_bound) < float("inf")):
        raise ValueError(f"norm_bound={norm_bound!r} must be positive and finite, or None")
    if not X.is_cuda:
        raise ValueError("X must be a dense fp16 device tensor [n, dim]")
    with torch.cuda.device(X.device):
        c = centroids if torch.is_tensor(centroids) else torch.from_numpy(np.ascontiguousarray(centroids))
        c16 = c.to(X.device).to(torch.float16).contiguous()
        bound = centroid_norm_bound(c16) if norm_bound is None else float(norm_bound)
        return cluster_assign(X, c16, bound)


def label_shard(index, allow, centroids) -> Dict:
    """What `HipCollection.assign_topics` runs: `predict` over the rows of a `ShardIndex` that the bitmap `allow` (None: every row)
    allows, gathered as `fit_shard` gathers them.  -> {labels numpy int32 [index.n_rows] (-1 for an excluded row), scores numpy f32
    (nan for an excluded row), sizes numpy int64 [C]}."""
    import torch
    n = index.n_rows
    C, _ = check_centroids(centroids, index.dim)
    rows = None if allow is None else allowed_rows(allow, n)
    X = index.corpus[:n] if rows is None else gather(index, rows)
    labels = np.full(n, -1, np.int32)
    scores = np.full(n, np.nan, np.float32)
    if X.shape[0]:
        lab, sc = predict(X.contiguous(), centroids)
        sel = slice(None) if rows is None else rows.cpu().numpy()
        labels[sel], scores[sel] = lab.cpu().numpy(), sc.cpu().numpy()
    return {"labels": labels, "scores": scores, "sizes": np.bincount(labels[labels >= 0], minlength=C).astype(np.int64)}


def check_representatives(representatives) -> int:
    if isinstance(representatives, bool) or not isinstance(representatives, (int, np.integer)) or not (0 <= representatives <= 32):
        raise ValueError(f"representatives={representatives!r} must be an integer in [0, 32] (the search's k limit)")
    return int(representatives)


def fit_shard(index, allow, n_topics, iters: int = 20, seed: int = 0, representatives: int = 3) -> Dict:
    """What `HipCollection.topics` and the CLI's `--topics` share: `kmeans` over the rows of a `ShardIndex` that the bitmap `allow`
    (None: every row) allows, gathered once into a buffer of their own, and the topics' representatives from one exact
    `index.search(centroids_f16, k, allow=allow)`.  -> {labels (numpy int32 [index.n_rows], -1 for an excluded row), sizes, centroids
    (numpy), objective, iterations, rep_scores f32 / rep_rows int64 [n_topics, representatives] (global row ids, -1 pads)}."""
    import torch
    k = check_representatives(representatives)
    n = index.n_rows
    check_args(max(n, 1), index.dim, 1, iters)                   # (dim and iters, before anything is gathered)
    rows = None if allow is None else allowed_rows(allow, n)
    check_args(n if rows is None else int(rows.shape[0]), index.dim, n_topics, iters)
    res = kmeans(index.corpus if rows is None else gather(index, rows), n_topics, iters=iters, seed=seed)
    labels = res["labels"]
    if rows is not None:
        labels = torch.full((n,), -1, dtype=torch.int32, device=index.corpus.device)
        labels[rows] = res["labels"]
    C = int(n_topics)
    if k > 0:
        s, i = index.search(res["centroids_f16"], k, allow=allow)
        s, i = s.cpu().numpy(), i.cpu().numpy()
    else:
        s, i = np.zeros((C, 0), np.float32), np.zeros((C, 0), np.int64)
    return {"labels": labels.cpu().numpy(), "sizes": res["sizes"].cpu().numpy(), "centroids": res["centroids"].cpu().numpy(),
            "objective": res["objective"], "iterations": res["iterations"], "rep_scores": s, "rep_rows": i}


def kmeans(X, n_clusters: int, iters: int = 20, seed: int = 0, init=None, assign: str = "kernel") -> Dict:
    """Spherical k-means of the rows of `X` (fp16 device tensor [n, dim], dense) as the module docstring defines it.
    -> {centroids (f32 device [C, dim]), centroids_f16, labels (int32 device [n]), sizes (int64 device [C]), objective (the mean
    score, summed in float64 on the device and read once), iterations (assigns run), changed (labels changed by each assign)}.
    `assign`: "kernel" (`arx_cluster_assign`, the default because the two paths give the same bits) or "search" (the exact k = 1 search
    over the centroids, kept for A/B runs).
    ValueError before any launch: `n_clusters` outside [1, min(n, 4096)], `iters < 1`, an `init` of the wrong shape or not finite, a
    `dim` that is not a multiple of 64 in [64, 8192]."""
    import torch
    if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float16 and X.dim() == 2 and X.is_contiguous()):
        raise ValueError("X must be a dense fp16 device tensor [n, dim]")
    n, dim = int(X.shape[0]), int(X.shape[1])
    init = check_args(n, dim, n_clusters, iters, init)
    if assign not in ("kernel", "search"):
        raise ValueError(f"assign={assign!r} must be 'kernel' or 'search'")
    n_clusters, iters = int(n_clusters), int(iters)
    with torch.cuda.device(X.device):
        if init is None:
            rows = torch.from_numpy(default_init_rows(n, n_clusters, seed)).to(X.device)
            c32 = X.index_select(0, rows).to(torch.float32)
        else:
            c32 = torch.from_numpy(init).to(X.device)
        c16 = c32.to(torch.float16)
        # the one read before the loop: kept centroids (empty clusters) carry the initial norms through every iteration
        bound = centroid_norm_bound(c16)
        prev = torch.full((n,), -1, dtype=torch.int32, device=X.device)
        ws = sums = None
        assign_ws = assign_workspace(n, n_clusters, dim, X.device) if assign == "kernel" else None
        changed = []
        for it in range(iters):
            labels, scores = _assign_rows(X, c16, bound, how=assign, ws=assign_ws)
            changed.append(int((labels != prev).sum().item()))            # the iteration's one host read
            if changed[-1] == 0 or it == iters - 1:
                break
            order, start, _ = members(labels, n_clusters)
            if ws is None:
                need = (((n + RUN - 1) // RUN) + n_clusters) * dim
                ws = torch.empty(need, dtype=torch.float32, device=X.device)
            sums = cluster_sums(X, order, start, n_clusters, out=sums, ws=ws)
            c32, c16 = cluster_finish(sums, start, c32)
            prev = labels
        sizes = torch.bincount(labels, minlength=n_clusters)
        objective = float(scores.to(torch.float64).mean().item())
    return {"centroids": c32, "centroids_f16": c16, "labels": labels, "sizes": sizes, "objective": objective,
            "iterations": len(changed), "changed": changed}
