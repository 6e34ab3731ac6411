"""Score-threshold queries (`min_score`): what `HipCollection.query`, `search_queries` and the CLI share on the host.  The search itself
is `ShardIndex.search_range` (csrc/range.hip)."""
from __future__ import annotations

from typing import Optional

import numpy as np

RANGE_MAX_RESULTS = 1024      # arx_range_search: rows per query
RERANK_BATCH = 32             # pairs the cross-encoder scores per batch, whatever the length of the range list


def thresholds(min_score, n_queries: int, each: str = "float") -> np.ndarray:
    """`min_score` (a float or one float per query) -> float32 [n_queries].  `each`: the noun of the refusal ("one float per query"
    from the front ends, "one entry per query" from the searches themselves)."""
    ms = np.asarray(min_score, dtype=np.float32)
    if ms.ndim == 0:
        return np.full(n_queries, ms, np.float32)
    if ms.shape != (n_queries,):
        raise ValueError(f"min_score has shape {tuple(ms.shape)}: a float or one {each} per query ({n_queries},)")
    return np.ascontiguousarray(ms)


def device_thresholds(min_score, n_queries: int, device):
    """`min_score` (a float, anything numpy converts, or a tensor on the host or the device; one value or one per query) ->
    contiguous float32 device [n_queries], as `ShardIndex.search_range` and `IvfIndex.search_many` hand it to the library."""
    import torch
    if not torch.is_tensor(min_score):
        return torch.from_numpy(thresholds(min_score, n_queries, each="entry")).to(device)
    ms = min_score.to(device=device, dtype=torch.float32)
    if ms.dim() == 0:
        ms = ms.expand(n_queries)
    if ms.shape != (n_queries,):
        raise ValueError(f"min_score has shape {tuple(ms.shape)}: a float or one entry per query ({n_queries},)")
    return ms.contiguous()


def check_range_query(n_results: int, *, ranged: bool, reranker=None, n_candidates: int = 32, hybrid_alpha: Optional[float] = None,
                      mmr_lambda: Optional[float] = None, group_by=None, per_query_filters: bool = False, world: int = 1) -> None:
    """The refusals of a `min_score` query, each a ValueError with its reason; nothing to check when `ranged` is false."""
    if not ranged:
        return
    if hybrid_alpha is not None:
        raise ValueError("min_score cannot be combined with hybrid_alpha: the BM25 keyword search has no score threshold")
    if mmr_lambda is not None:
        raise ValueError("min_score cannot be combined with mmr_lambda: MMR picks among at most 32 candidates of the top-k search")
    if group_by:
        raise ValueError("min_score cannot be combined with group_by: the grouped search ranks papers, not rows above a threshold")
    if per_query_filters:
        raise ValueError("min_score cannot be combined with per-query filter lists: the range search takes one bitmap per call")
    if world > 1:
        raise ValueError("min_score needs world == 1: a cross-rank merge of lists of up to 1024 rows is out of scope")
    if not (1 <= int(n_results) <= RANGE_MAX_RESULTS):
        raise ValueError(f"n_results={n_results} must be in [1, {RANGE_MAX_RESULTS}] with min_score")
    if reranker is not None and not (int(n_results) <= int(n_candidates) <= RANGE_MAX_RESULTS):
        raise ValueError(f"n_candidates={n_candidates} must be in [n_results, {RANGE_MAX_RESULTS}] with min_score and reranker")
