"""Host side of the search with a different filter per query (`ShardIndex.search_filtered_many`, `arx_topk_search_filtered_multi`): which
queries of a batch share a filter, and how a batch with more distinct filters than one call takes is cut into calls.

    wheres = per_query_list(where, n_queries, "where")                  # a list with one filter dict or None per query
    pairs, filter_of = distinct_filters(wheres, where_documents)        # the distinct (where, where_document) pairs, one index per query
    for positions, filters, local_of in filter_groups(filter_of):       # calls of at most MAX_FILTERS distinct filters each
        ...search the queries at `positions` with the bitmaps of `filters` and the indices `local_of`...

No GPU and no torch in here.
"""
from __future__ import annotations

import json
from typing import List, Optional, Sequence, Tuple

MAX_FILTERS = 64      # bitmaps one arx_topk_search_filtered_multi call takes (include/arx.h)


def is_per_query(arg) -> bool:
    """A list or tuple is one filter per query; a dict (or None) is one filter for the call."""
    return isinstance(arg, (list, tuple))


def per_query_list(arg, n_queries: int, name: str) -> List[Optional[dict]]:
    """`arg` as one entry per query: a list / tuple must have `n_queries` entries, each a dict or None; a dict or None is repeated."""
    if not is_per_query(arg):
        if arg is not None and not isinstance(arg, dict):
            raise ValueError(f"{name} must be a filter dict, None, or a list with one of those per query, got {type(arg).__name__}")
        return [arg] * n_queries
    if len(arg) != n_queries:
        raise ValueError(f"{name} has {len(arg)} entries for {n_queries} queries: a list needs one entry (a filter or None) per query")
    for j, f in enumerate(arg):
        if f is not None and not isinstance(f, dict):
            raise ValueError(f"{name}[{j}] must be a filter dict or None, got {type(f).__name__}")
    return list(arg)


def canonical_pair(where, where_document) -> str:
    """The key under which two queries share a bitmap: the pair as JSON with sorted keys (`{"a": 1, "b": 2}` and `{"b": 2, "a": 1}` are
    one filter; lists keep their order)."""
    return json.dumps([where, where_document], sort_keys=True)


def distinct_filters(wheres: Sequence, where_documents: Sequence) -> Tuple[List[Tuple], List[int]]:
    """-> (the distinct (where, where_document) pairs in order of first appearance, for every query the index of its pair)."""
    if len(wheres) != len(where_documents):
        raise ValueError(f"{len(wheres)} where entries for {len(where_documents)} where_document entries")
    seen, pairs, filter_of = {}, [], []
    for w, d in zip(wheres, where_documents):
        key = canonical_pair(w, d)
        if key not in seen:
            seen[key] = len(pairs)
            pairs.append((w, d))
        filter_of.append(seen[key])
    return pairs, filter_of


def filter_groups(filter_of: Sequence[int], max_filters: int = MAX_FILTERS) -> List[Tuple[List[int], List[int], List[int]]]:
    """Cut a batch into calls of at most `max_filters` distinct filters: distinct filter f goes to call f // max_filters.  -> per call
    (the positions of its queries in the batch, ascending; the filters it uses, ascending; for each of its queries the index of its
    filter within that list).  Every query is in exactly one call, so writing call c's j-th result to position
    `positions[j]` puts the results back in batch order (`index.search_filtered_grouped`)."""
    if max_filters < 1:
        raise ValueError(f"max_filters={max_filters}")
    calls = {}
    for pos, f in enumerate(filter_of):
        calls.setdefault(int(f) // max_filters, []).append(pos)
    out = []
    for c in sorted(calls):
        positions = calls[c]
        filters = sorted({int(filter_of[p]) for p in positions})
        local = {f: j for j, f in enumerate(filters)}
        out.append((positions, filters, [local[int(filter_of[p])] for p in positions]))
    return out
