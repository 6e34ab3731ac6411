"""Host side of the grouped search (`arx_topk_search_grouped`, INTEGRATION.md "Grouped results"): the runs of a metadata key, the
numbers S and K of the exactness argument (csrc/grouped.hip), and the argument checks `HipCollection.query(group_by=True)` and the
CLI's `--group-by-paper` share."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

GROUPS_MAX = 32          # papers per query (the search's k limit)
CHUNKS_MAX = 8           # chunks returned per paper
KSEL_MAX = 512           # the scan selects among at most this many 64-row group maxima; beyond: the exhaustive path


def runs_from_keys(keys: Sequence, base: int = 0) -> Tuple[np.ndarray, List]:
    """Consecutive equal keys are one run -> (`group_of` int32 [n], the run's number for every row, ascending from 0; the key of every
    run).  A key that reappears after its run ended is a ValueError naming the key and the two rows (`base` + position): a paper
    whose chunks are not consecutive cannot be a group."""
    group_of = np.empty(len(keys), dtype=np.int32)
    run_keys: List = []
    last_row: Dict = {}                                      # key -> the last row of its run
    prev = object()
    for r, key in enumerate(keys):
        if not run_keys or key != prev:
            if key in last_row:
                raise ValueError(f"group key {key!r} appears at row {base + last_row[key]} and again at row {base + r} after its run "
                                 f"ended: a group must be consecutive rows")
            run_keys.append(key)
            prev = key
        last_row[key] = r
        group_of[r] = len(run_keys) - 1
    return group_of, run_keys


def continue_runs(group_of: np.ndarray, run_keys: Sequence, keys: Sequence, base: int = 0) -> Tuple[np.ndarray, List]:
    """`runs_from_keys` continued over rows appended to a shard (`HipCollection.add`): `group_of` int32 [n] and `run_keys` (the key of
    every `group_of` value; values need not be dense, a value no row holds any more is a run that was deleted) describe the rows there
    are, `keys` are the new rows' -> (`group_of` of the new rows, the extended `run_keys`; the arguments are not changed).  A first new
    row with the key of the last row continues that run; a key whose run already ended is `runs_from_keys`' ValueError, naming the
    key, the run's last row and the new row (`base` + position among all rows); a new run takes the next unused value."""
    group_of = np.asarray(group_of, dtype=np.int32)
    n = len(group_of)
    out = np.empty(len(keys), dtype=np.int32)
    run_keys = list(run_keys)
    live = np.unique(group_of)
    last_row: Dict = {run_keys[int(g)]: int(np.searchsorted(group_of, g, side="right")) - 1 for g in live}
    cur = int(group_of[-1]) if n else -1
    prev = run_keys[cur] if n else object()
    for j, key in enumerate(keys):
        if cur < 0 or key != prev:
            if key in last_row:
                raise ValueError(f"group key {key!r} appears at row {base + last_row[key]} and again at row {base + n + j} after its run "
                                 f"ended: a group must be consecutive rows")
            run_keys.append(key)
            cur, prev = len(run_keys) - 1, key
        last_row[key] = n + j
        out[j] = cur
    return out, run_keys


def groups_touched(max_run_rows: int) -> int:
    """S: the 64-row groups a run of at most `max_run_rows` rows can touch, whatever its offset."""
    return (int(max_run_rows) + 62) // 64 + 1


def select_count(n_groups: int, max_run_rows: int) -> int:
    """K = P S: the group maxima the scan selects among."""
    return int(n_groups) * groups_touched(max_run_rows)


def check_grouped_query(n_results: int, chunks_per_group: int, *, grouped: bool, has_group_key: bool = True, reranker=None,
                        hybrid_alpha: Optional[float] = None, mmr_lambda: Optional[float] = None, per_query_filters: bool = False,
                        world: int = 1) -> None:
    """The refusals of a grouped query, each a ValueError with its reason; nothing to check when `grouped` is false."""
    if not grouped:
        return
    if not has_group_key:
        raise ValueError("group_by needs a collection built with group_key (e.g. group_key=\"paper_id\")")
    if reranker is not None:
        raise ValueError("group_by cannot be combined with reranker: the cross-encoder ranks chunks, not papers")
    if hybrid_alpha is not None:
        raise ValueError("group_by cannot be combined with hybrid_alpha: the BM25 keyword search has no groups")
    if mmr_lambda is not None:
        raise ValueError("group_by cannot be combined with mmr_lambda: MMR re-orders the cosine search's chunk candidates only")
    if per_query_filters:
        raise ValueError("group_by cannot be combined with per-query filter lists: the grouped search takes one bitmap per call")
    if world > 1:
        raise ValueError("group_by needs world == 1: a paper may straddle two ranks, and a cross-rank fold is out of scope")
    if not (1 <= int(n_results) <= GROUPS_MAX):
        raise ValueError(f"n_results={n_results} must be in [1, {GROUPS_MAX}] papers with group_by")
    if not (1 <= int(chunks_per_group) <= CHUNKS_MAX):
        raise ValueError(f"chunks_per_group={chunks_per_group} must be in [1, {CHUNKS_MAX}]")
