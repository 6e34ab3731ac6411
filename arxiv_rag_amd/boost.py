"""Boosted search: the exact top-k of cosine plus a weighted row prior (`arx_topk_search_boosted`, `arx_prior_info`, include/arx.h;
INTEGRATION.md "Boosted search").

    prior = prior_from_metadata(metadatas, {"key": "quality_score", "missing": 0.0})     # f32 [rows]
    scores, base, ids = index.search_boosted(q, 10, prior_dev, weight=0.05)              # index: a ShardIndex

For query q and row r, `base(q, r)` is the f32 cosine `ShardIndex.search` gives the pair and

    boosted(q, r) = float32(base(q, r) + float32(weight[q] * prior[r]))

two separately rounded f32 operations.  A row is visible when the bitmap (if any) allows it and its prior is finite; the answer is the
k best visible rows by (boosted desc, row asc).  `boosted_host` restates that with numpy (for the tests; the product path never calls
it); `check_args` and `check_query_with_boost` are the refusals; `prior_from_metadata` builds the prior column from a metadata key.
This module launches nothing: the launch is `ShardIndex.search_boosted`.
"""
from __future__ import annotations

import math

import numpy as np

MAX_K, MAX_DIM = 32, 8192


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def weights_of(weight, n_queries: int) -> np.ndarray:
    """`weight` (a number, or one per query) -> float32 [n_queries]; a wrong shape, a non-number or a non-finite value is a ValueError."""
    if hasattr(weight, "detach"):
        weight = weight.detach().cpu().numpy()
    try:
        w = np.asarray(weight, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"boost weight must be a number or one number per query, not {type(weight).__name__}") from None
    if w.ndim == 0:
        w = np.full(n_queries, float(w))
    if w.shape != (n_queries,):
        raise ValueError(f"boost weight has shape {tuple(w.shape)}: one number, or one per query ({n_queries},)")
    with np.errstate(over="ignore"):
        w32 = w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError("boost weight must be finite (as a float32)")
    return w32


def check_args(k, weight, n_queries: int, max_abs_prior: float = 0.0, dim=None) -> np.ndarray:
    """The refusals of `ShardIndex.search_boosted`, each a ValueError before anything is launched -> the weights as float32
    [n_queries].  `max_abs_prior`: the largest |finite prior| (`arx_prior_info`)."""
    if not _is_int(k) or not (1 <= k <= MAX_K):
        raise ValueError(f"k={k!r} must be an integer in [1, {MAX_K}] (the search's k limit)")
    if dim is not None and (not _is_int(dim) or dim < 64 or dim % 64 or dim > MAX_DIM):
        raise ValueError(f"dim={dim!r} must be a multiple of 64 in [64, {MAX_DIM}]")
    w = weights_of(weight, n_queries)
    m = float(max_abs_prior)
    if not (m >= 0.0 and math.isfinite(m)):
        raise ValueError(f"max_abs_prior={max_abs_prior!r} must be a finite bound on |prior|")
    if w.size:
        with np.errstate(over="ignore"):
            top = np.float32(np.abs(w).max()) * np.float32(m)
        if not np.isfinite(top):
            raise ValueError(f"|boost weight| * max|prior| = {float(np.abs(w).max())} * {m} is not finite in float32")
    return w


def check_query_with_boost(boost_weight, *, has_prior: bool, per_query_filters: bool = False, hybrid_alpha=None, group_by=None,
                           min_score=None, nprobe=None, binary_candidates=None, world: int = 1, n_width: int = 1, n_queries: int = 1,
                           max_abs_prior: float = 0.0, pq_candidates=None) -> np.ndarray:
    """The refusals of `query(boost_weight=...)`, `retrieve` and `search_queries`, each a ValueError naming the part, before any launch
    (`modes.check_mode`) -> the weights as float32 [n_queries].  `n_width`: the rows the search returns per query (the reranker's or
    MMR's candidates, else n_results)."""
    from .modes import check_mode
    return check_mode("boost_weight", boost_weight, has_index=has_prior, per_query=per_query_filters, hybrid_alpha=hybrid_alpha,
                      group_by=group_by, min_score=min_score, world=world, n_width=n_width, n_queries=n_queries, max_abs_prior=max_abs_prior,
                      others={"nprobe": nprobe, "binary_candidates": binary_candidates, "pq_candidates": pq_candidates})


# ---- the prior column ----------------------------------------------------------------------------------------------------------------
def prior_from_metadata(metadatas, spec) -> np.ndarray:
    """float32 [len(metadatas)] from a metadata key.  `spec`:
        {"key": K, "missing": 0.0}                                                  the numeric value as it is (bools become 0 / 1)
        {"key": K, "decay": "exp", "origin": o, "half_life": h, "missing": 0.0}     exp(-ln 2 * |v - o| / h), computed in float64
    `missing` (default 0.0) is the PRIOR of a row without the key (or with None), not a value fed to the decay.  A string (or any other
    non-number) value, an unknown entry of the spec, a missing "key" and half_life <= 0 are ValueErrors."""
    if not isinstance(spec, dict) or "key" not in spec:
        raise ValueError("a boost spec is a dict with a \"key\" entry")
    unknown = set(spec) - {"key", "missing", "decay", "origin", "half_life"}
    if unknown:
        raise ValueError(f"unknown boost spec entries: {', '.join(sorted(unknown))}")
    key, missing, decay = spec["key"], spec.get("missing", 0.0), spec.get("decay")
    if isinstance(missing, (str, bytes)) or not isinstance(missing, (int, float, np.integer, np.floating)):
        raise ValueError(f"boost spec: missing={missing!r} must be a number")
    if decay is None:
        if "origin" in spec or "half_life" in spec:
            raise ValueError("boost spec: origin and half_life belong to decay=\"exp\"")
    elif decay == "exp":
        if "origin" not in spec or "half_life" not in spec:
            raise ValueError("boost spec: decay=\"exp\" needs origin and half_life")
        origin, half_life = float(spec["origin"]), float(spec["half_life"])
        if not (half_life > 0.0 and math.isfinite(half_life)) or not math.isfinite(origin):
            raise ValueError(f"boost spec: half_life={spec['half_life']!r} must be positive and finite, origin finite")
    else:
        raise ValueError(f"boost spec: decay={decay!r} must be \"exp\" or absent")
    out = np.empty(len(metadatas), np.float64)
    for i, md in enumerate(metadatas):
        v = (md or {}).get(key)
        if v is None:
            out[i] = float(missing)
            continue
        if not isinstance(v, (bool, int, float, np.bool_, np.integer, np.floating)):
            raise ValueError(f"boost spec: metadata {key!r} of row {i} is {type(v).__name__} {v!r}, not a number")
        v = float(v)
        out[i] = v if decay is None else math.exp(-math.log(2.0) * abs(v - origin) / half_life)      # (NaN stays NaN: the row is hidden)
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def _visible(allow, n_rows: int) -> np.ndarray:
    """bool [n_rows] from None, a bool mask or bitmap words (bits at or beyond n_rows ignored)."""
    if allow is None:
        return np.ones(n_rows, bool)
    allow = np.asarray(allow)
    if allow.dtype == bool:
        return allow[:n_rows].copy()
    from .mutation import unpack_rows
    return unpack_rows(allow, n_rows)


def boosted_host(X, Q, prior, weight, k: int, allow=None, base=None):
    """(scores f32 [nq, k], base f32 [nq, k], ids int64 [nq, k]): what `arx_topk_search_boosted` returns with idx_base = 0.  `X` fp16
    [n, dim], `Q` fp16 [nq, dim], `prior` f32 [n], `weight` a number or f32 [nq], `allow` None, a bool mask or bitmap words.  base =
    `topics.exact_scores_host`; boosted = base + float32(w) * prior in float32 (a rounded product, then a rounded sum); rows with a
    non-finite prior or outside `allow` are dropped; order by `lexsort` on (row asc, boosted desc); (-inf, -inf, -1) pads.  `base`: the
    [n, nq] matrix of `exact_scores_host(X, Q)` if the caller has it already."""
    from .topics import exact_scores_host
    X, Q = np.asarray(X), np.asarray(Q)
    n, nq = X.shape[0], Q.shape[0]
    prior = np.asarray(prior, dtype=np.float32)
    if prior.shape != (n,):
        raise ValueError(f"prior has shape {tuple(prior.shape)}, the {n} rows need ({n},)")
    w = check_args(k, weight, nq)
    rows = np.flatnonzero(_visible(allow, n) & np.isfinite(prior))
    B = exact_scores_host(X, Q) if base is None else np.asarray(base, dtype=np.float32)
    scores = np.full((nq, k), -np.inf, np.float32)
    bases = np.full((nq, k), -np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        b = B[rows, q].astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            p = (np.float32(w[q]) * prior[rows]).astype(np.float32)
            s = (b + p).astype(np.float32)
        ok = np.isfinite(p)                                      # a product that overflows hides the row, as on the device
        r, b, s = rows[ok], b[ok], s[ok]
        best = np.lexsort((r, -s))[:k]
        m = best.shape[0]
        scores[q, :m], bases[q, :m], ids[q, :m] = s[best], b[best], r[best]
    return scores, bases, ids
