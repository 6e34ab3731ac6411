"""Graph search: a beam search over a fixed-degree k-NN graph of the shard's rows, every score exact (`arx_graph_search`,
include/arx.h; INTEGRATION.md "Graph search").

    g = GraphIndex.build(index, degree=32)                    # index: a ShardIndex; exact k-NN lists, reverse edges, medoid entries
    scores, ids, scored = g.search(q, k=10, ef=64)            # q: fp16 device [nq, dim]

One block walks one query: from its entry rows it repeatedly expands the best row of a beam of `ef` rows that it has not expanded yet,
scoring the neighbours it has not seen.  Which rows get visited is the only approximation: a row's score is `exact_row_score`, the order
is (score desc, row asc), so what comes back has the score bits and the order of every other search here.  A query scores a few
thousand rows whatever the shard's size, and its answer does not depend on the batch it is in.

`graph_search` is the one place that calls the library.  `search_host` and `assemble_host` restate the kernel and the graph assembly
with numpy (for the tests; the product path never calls them); `check_search_args`, `check_build_args` and `check_query_with_graph` are
the refusals, each a ValueError before any launch.

A built graph follows the rows only where that is asked for (`HipCollection.build_graph(maintain=True)`): `GraphIndex.insert` links new
rows in (a graph search and an exact search of the batch for their candidates, then one `arx_graph_link` that offers them to the tails
of their nearest rows' lists), `GraphIndex.remap` renumbers the graph after a compaction (`arx_graph_remap`).  `graph_link` and
`graph_remap` are the only callers of those two entry points; `link_host`, `remap_host` and `insert_host` restate them with numpy.
`rows_added` and `rows_compacted` are what `HipCollection.add` and `compact` call: with `maintain` they insert and remap, without it they
mark the graph stale and `build_graph` has to run again.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np

MAX_K, MAX_EF, MAX_ITERS, MAX_ENTRIES, MAX_DEGREE = 32, 512, 1024, 64, 64
MAX_VISITED = 8192              # rows the kernel's visited table holds (16384 slots at a load factor of one half)
KNN = 32                        # width of the k-NN search of a build: 31 neighbours a row once its own id is dropped
MAX_BUILD_DEGREE, MAX_ENTRY_LISTS, MAX_QUERY_ENTRIES = 32, 4096, 32
BUILD_BATCH = 4096              # queries per k-NN search of a build
ASSEMBLE_ROWS = 1 << 20         # rows per slice of the assembly's last step


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def max_iters_for(degree: int, n_entries: int) -> int:
    """The largest `max_iters` the visited table admits for this degree and number of entries (at most `MAX_ITERS`)."""
    return max(0, min(MAX_ITERS, (MAX_VISITED - int(n_entries)) // int(degree)))


def check_search_args(k, ef, max_iters, degree, n_entries) -> None:
    """The refusals of `graph_search` / `GraphIndex.search` about the walk's parameters, each a ValueError before anything is launched."""
    if not _is_int(k) or not (1 <= k <= MAX_K):
        raise ValueError(f"k={k!r} must be an integer in [1, {MAX_K}] (the search's k limit)")
    if not _is_int(ef) or not (k <= ef <= MAX_EF):
        raise ValueError(f"ef={ef!r} must be an integer in [k, {MAX_EF}] = [{k}, {MAX_EF}] (the beam's width)")
    if not _is_int(degree) or not (8 <= degree <= MAX_DEGREE) or degree % 8:
        raise ValueError(f"degree={degree!r} must be a multiple of 8 in [8, {MAX_DEGREE}]")
    if not _is_int(n_entries) or not (1 <= n_entries <= MAX_ENTRIES):
        raise ValueError(f"n_entries={n_entries!r} must be an integer in [1, {MAX_ENTRIES}]")
    if not _is_int(max_iters) or not (1 <= max_iters <= MAX_ITERS):
        raise ValueError(f"max_iters={max_iters!r} must be an integer in [1, {MAX_ITERS}]")
    if n_entries + max_iters * degree > MAX_VISITED:
        raise ValueError(f"n_entries + max_iters * degree = {n_entries + max_iters * degree} exceeds the visited table's {MAX_VISITED} rows: "
                         f"at degree {degree} max_iters may be at most {max_iters_for(degree, n_entries)}")


def check_build_args(n_rows: int, dim: int, degree, n_entry_lists, iters, nprobe=None, has_ivf: bool = False) -> int:
    """The refusals of `GraphIndex.build`, each a ValueError before anything is launched -> the number of entry lists."""
    from .topics import check_args
    if not _is_int(degree) or not (8 <= degree <= MAX_BUILD_DEGREE) or degree % 8:
        raise ValueError(f"degree={degree!r} must be a multiple of 8 in [8, {MAX_BUILD_DEGREE}] (a build has {KNN - 1} neighbours a row)")
    if n_rows < 1:
        raise ValueError("a graph needs at least one row: the collection is empty")
    if n_rows >= 1 << 31:
        raise ValueError(f"n_rows={n_rows} must be below 2^31 (the graph holds int32 rows)")
    if (nprobe is None) != (not has_ivf):
        raise ValueError("ivf= and nprobe= go together: the approximate build takes its k-NN lists from IvfIndex.search(nprobe)")
    if n_entry_lists is None:
        n_entry_lists = max(1, min(MAX_ENTRY_LISTS, n_rows, int(round(n_rows ** 0.5))))
    if not _is_int(n_entry_lists) or not (1 <= n_entry_lists <= min(MAX_ENTRY_LISTS, n_rows)):
        raise ValueError(f"n_entry_lists={n_entry_lists!r} must be an integer in [1, min({MAX_ENTRY_LISTS}, rows)], or None")
    check_args(n_rows, dim, int(n_entry_lists), iters)
    return int(n_entry_lists)


def check_query_args(n_width, graph_ef, stale: bool = False, n_entries=8, n_entry_lists: int = MAX_ENTRY_LISTS, degree: int = 32) -> None:
    """The refusals of a query's `graph_ef` / `graph_entries` against a graph that is there (`modes.MODES`): a stale graph, then
    the walk's parameters at the width `n_width` the search returns."""
    if stale:
        raise ValueError("the graph index is stale: rows were added or compacted since build_graph(); run build_graph() again "
                         "(build_graph(maintain=True) keeps the graph usable across add and compact)")
    if not _is_int(n_entries) or not (1 <= n_entries <= min(MAX_QUERY_ENTRIES, n_entry_lists)):
        raise ValueError(f"graph_entries={n_entries!r} must be an integer in [1, min({MAX_QUERY_ENTRIES}, entry lists = {n_entry_lists})]")
    if not _is_int(n_width) or not (1 <= n_width <= MAX_K):
        raise ValueError(f"the search returns {n_width} rows a query: the graph search's width must be in [1, {MAX_K}]")
    if not _is_int(graph_ef) or not (n_width <= graph_ef <= MAX_EF):
        raise ValueError(f"graph_ef={graph_ef!r} must be an integer in [width, {MAX_EF}] = [{n_width}, {MAX_EF}]: it lies below k={n_width} or "
                         f"above the limit")
    check_search_args(n_width, graph_ef, max(1, min(int(graph_ef), max_iters_for(degree, n_entries))), degree, n_entries)


def check_query_with_graph(graph_ef, *, has_index: bool, stale: bool = False, n_entries=8, n_entry_lists: int = MAX_ENTRY_LISTS, degree: int = 32,
                           per_query_filters: bool = False, hybrid_alpha=None, group_by=None, min_score=None, boost_weight=None, nprobe=None,
                           binary_candidates=None, pq_candidates=None, world: int = 1, n_width: int = 1) -> None:
    """The refusals of `query(graph_ef=...)`, `retrieve` and `search_queries`, each a ValueError naming the part, before any launch
    (`modes.check_mode`)."""
    from .modes import check_mode
    check_mode("graph_ef", graph_ef, has_index=has_index, per_query=per_query_filters, hybrid_alpha=hybrid_alpha, group_by=group_by,
               min_score=min_score, world=world, n_width=n_width, stale=stale, n_entries=n_entries, n_entry_lists=n_entry_lists, degree=degree,
               others={"boost_weight": boost_weight, "nprobe": nprobe, "binary_candidates": binary_candidates, "pq_candidates": pq_candidates})


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def order_words(scores) -> np.ndarray:
    """uint32: the order-preserving word of every f32 score (the high word of the kernel's keys): larger is better, a NaN 0."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = s.view(np.uint32)
    w = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    w[np.isnan(s)] = 0
    return w


def _key_score(key: int) -> np.float32:
    w = key >> 32
    bits = 0x7FC00000 if w == 0 else ((w & 0x7FFFFFFF) if w & 0x80000000 else (~w & 0xFFFFFFFF))
    return np.array([bits], np.uint32).view(np.float32)[0]


def search_host(X, neighbors, Q, entries, k: int, ef: int, max_iters: int, allow=None, pair_scores=None):
    """(scores f32 [nq, k], ids int64 [nq, k], scored int64 [nq], expanded int64 [nq]): what `arx_graph_search` returns with
    idx_base = 0, bit for bit.  `X` fp16 [n_rows, dim], `neighbors` int [n_rows, degree], `Q` fp16 [nq, dim], `entries` int
    [nq, n_entries]; `allow`: None, a bool mask [n_rows] or bitmap words (int64 / uint64 [ceil(n_rows / 64)]).  The visited set is a
    Python set, a score is `topics.exact_scores_host`, a pair is the integer  order word << 32 | (0xffffffff - row)  (larger is
    better: score desc, row asc, a NaN below every number), the beam a descending list of them cut at `ef`.  `pair_scores`: f32
    [n_rows, nq], `exact_scores_host(X, Q)` computed once by the caller (a pair's bits do not depend on what it is computed with)."""
    from .mutation import unpack_rows
    from .topics import exact_scores_host
    X, Q, neighbors, entries = np.asarray(X), np.asarray(Q), np.asarray(neighbors), np.asarray(entries)
    n_rows, nq = X.shape[0], Q.shape[0]
    check_search_args(k, ef, max_iters, int(neighbors.shape[1]), int(entries.shape[1]))
    mask = None
    if allow is not None:
        allow = np.asarray(allow)
        mask = allow if allow.dtype == bool else unpack_rows(allow, n_rows)
    scores = np.full((nq, k), -np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    scored, expanded = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        visited, beam, done, best = set(), [], set(), []

        def offer(rows):
            new = []
            for r in (int(v) for v in rows):
                if 0 <= r < n_rows and r not in visited:
                    visited.add(r)
                    new.append(r)
            if not new:
                return
            sc = exact_scores_host(X[new], Q[q:q + 1])[:, 0] if pair_scores is None else pair_scores[new, q]
            keys = [(int(w) << 32) | (0xFFFFFFFF - r) for w, r in zip(order_words(sc), new)]
            scored[q] += len(new)
            beam[:] = sorted(beam + keys, reverse=True)[:ef]
            if mask is not None:
                best[:] = sorted(best + [key for key, r in zip(keys, new) if mask[r]], reverse=True)[:k]

        offer(entries[q])
        for _ in range(max_iters):
            parent = next((key for key in beam if key not in done), None)
            if parent is None:
                break
            done.add(parent)
            expanded[q] += 1
            offer(neighbors[0xFFFFFFFF - (parent & 0xFFFFFFFF)])
        res = (beam if mask is None else best)[:k]
        for j, key in enumerate(res):
            scores[q, j], ids[q, j] = _key_score(key), 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return scores, ids, scored, expanded


def _valid_lists(knn, n: int):
    """Per row the valid entries of its k-NN list, in order: inside [0, n), not the row itself.  ValueError if one repeats."""
    out = []
    for i, row in enumerate(np.asarray(knn).tolist()):
        v = [int(r) for r in row if 0 <= r < n and r != i]
        if len(set(v)) != len(v):
            raise ValueError(f"knn[{i}] names a row twice: the k-NN lists must hold distinct rows")
        out.append(v)
    return out


def assemble_host(knn, degree: int) -> np.ndarray:
    """int32 [n, degree]: the fixed-degree graph of the k-NN lists `knn` (int [n, w]; an entry outside [0, n) or equal to its row is
    no neighbour; a row's valid entries are distinct).  With H = degree / 2:  fwd(i) = the first H valid entries of knn[i];  rev(i) = the
    rows j with i in fwd(j), by (position of i in fwd(j) asc, j asc);  neighbors[i] = fwd(i), then the first H entries of rev(i) not in
    fwd(i), then the later valid entries of knn[i] not already present, until `degree` are filled; the rest -1."""
    knn = np.asarray(knn)
    n, H = knn.shape[0], degree // 2
    valid = _valid_lists(knn, n)
    rev = [[] for _ in range(n)]
    for p in range(H):                                            # (position asc, j asc)
        for j in range(n):
            if p < len(valid[j]):
                rev[valid[j][p]].append(j)
    out = np.full((n, degree), -1, np.int32)
    for i in range(n):
        row = valid[i][:H]
        row += [j for j in rev[i] if j not in row][:H]
        for r in valid[i][H:]:
            if len(row) >= degree:
                break
            if r not in row:
                row.append(r)
        out[i, :len(row)] = row[:degree]
    return out


def _keys_of(scores, rows):
    """The kernel's integer keys of (score, row) pairs: order word << 32 | (0xffffffff - row)."""
    return [(int(w) << 32) | (0xFFFFFFFF - int(r)) for w, r in zip(order_words(scores), rows)]


def link_host(X, neighbors, targets, offer_start, offers, n_rows: Optional[int] = None) -> np.ndarray:
    """int32 [rows, degree]: `neighbors` after `arx_graph_link`, bit for bit (include/arx.h has the definition).  `X` fp16 [>= n_rows,
    dim], `neighbors` int [>= n_rows, degree], `targets` int [T], `offer_start` int [T + 1], `offers` int [n_offers]; `n_rows`: the
    rows there are (None: all of `X`).  Per live slot: the head stays, the pool is the old tail and the offers without the target, the
    head's rows and repeats, the new tail its H largest keys.  A slot is live when its target lies in [0, n_rows), is above every
    earlier slot's target inside [0, n_rows) and its `offer_start` pair is ascending inside [0, n_offers]."""
    from .topics import exact_scores_host
    X = np.asarray(X)
    out = np.array(neighbors, dtype=np.int32, copy=True)
    n = int(X.shape[0]) if n_rows is None else int(n_rows)
    H = out.shape[1] // 2
    targets, start, offers = (np.asarray(v).astype(np.int64).tolist() for v in (targets, offer_start, offers))
    top = -1
    for s, t in enumerate(targets):
        before, top = top, (max(top, t) if t < n else top)
        a, b = start[s], start[s + 1]
        if not (0 <= t < n) or t <= before or a < 0 or b < a or b > len(offers):
            continue
        head = {int(r) for r in out[t, :H] if 0 <= r < n}
        pool = sorted({int(r) for r in out[t, H:].tolist() + offers[a:b] if 0 <= r < n and r != t and r not in head})
        keys = sorted(_keys_of(exact_scores_host(X[pool], X[t:t + 1])[:, 0], pool), reverse=True)[:H] if pool else []
        out[t, H:] = [0xFFFFFFFF - (key & 0xFFFFFFFF) for key in keys] + [-1] * (H - len(keys))
    return out


def remap_host(neighbors, keep, n_old: Optional[int] = None) -> np.ndarray:
    """int32 [count, degree]: the moved neighbour rows `neighbors` (those of the kept rows, in order) after `arx_graph_remap`.
    `keep`: bool [n_old] or bitmap words (then `n_old` is needed).  An entry that names a kept row becomes that row's new number
    (`mutation.old_to_new`), every other entry is dropped; the survivors move to the row's front in order, the rest is -1."""
    from .mutation import old_to_new, unpack_rows
    keep = np.asarray(keep)
    mask = keep if keep.dtype == bool else unpack_rows(keep, int(n_old))
    new = old_to_new(mask)
    nb = np.asarray(neighbors)
    out = np.full(nb.shape, -1, np.int32)
    for i, row in enumerate(nb.tolist()):
        v = [int(new[e]) for e in row if 0 <= e < mask.shape[0] and mask[e]]
        out[i, :len(v)] = v
    return out


def orphans_host(neighbors, lo: int, hi: int) -> int:
    """The rows of [lo, hi) that no row's list names."""
    nb = np.asarray(neighbors)[:hi]
    return int(hi - lo - np.unique(nb[(nb >= lo) & (nb < hi)]).shape[0])


def insert_host(X, neighbors, lo: int, hi: int, entries, insert_ef: int = 64, batch: Optional[int] = None, pair_scores=None):
    """(int32 [hi, degree], {inserted, offers, orphans}): what `GraphIndex.insert(lo, hi, insert_ef)` leaves, edge for edge.  `X` fp16
    [>= hi, dim], `neighbors` int [lo, degree] (the graph over [0, lo)), `entries` int [hi - lo, E]: the entry rows of every new
    row's walk (`GraphIndex.entries` of the rows), `batch`: rows per batch (None: `BUILD_BATCH`).  Per batch [a, b): `search_host`
    over the a rows before it (k = 31), the exact scores of the batch against itself (the 32 best a row, its own id dropped as
    `knn_lists` drops it), the 31 best of the two by key, the new rows' lists, and one `link_host` of the offers over b rows.
    `pair_scores`: f32 [hi, hi - lo], `exact_scores_host(X[:hi], X[lo:hi])` computed once by the caller."""
    from .topics import exact_scores_host
    X, entries = np.asarray(X), np.asarray(entries)
    degree = int(np.asarray(neighbors).shape[1])
    check_insert_args(degree, int(np.asarray(neighbors).shape[0]), lo, hi, int(X.shape[0]), insert_ef)
    H, batch = degree // 2, BUILD_BATCH if batch is None else int(batch)
    E = int(entries.shape[1])
    max_iters = max(1, min(int(insert_ef), max_iters_for(degree, E)))
    nb = np.full((hi, degree), -1, np.int32)
    nb[:lo] = np.asarray(neighbors)[:lo]
    n_offers = 0
    for a in range(lo, hi, batch):
        b = min(hi, a + batch)
        m = b - a
        P = None if pair_scores is None else pair_scores[:, a - lo:b - lo]
        so, io, _, _ = search_host(X[:a], nb[:a], X[a:b], entries[a - lo:b - lo], KNN - 1, int(insert_ef), max_iters,
                                   pair_scores=None if P is None else P[:a])
        S = exact_scores_host(X[a:b], X[a:b]) if P is None else P[a:b]                      # [row, query]
        by_target: Dict[int, list] = {}
        for j in range(m):
            own = sorted(_keys_of(S[:, j], range(m)), reverse=True)[:KNN]
            me = next((p for p, key in enumerate(own) if 0xFFFFFFFF - (key & 0xFFFFFFFF) == j), None)
            if me is not None:
                del own[me]
            elif len(own) == KNN:
                del own[-1]
            own = [((key >> 32) << 32) | (0xFFFFFFFF - (0xFFFFFFFF - (key & 0xFFFFFFFF) + a)) for key in own]
            old = _keys_of(so[j][io[j] >= 0], io[j][io[j] >= 0])
            knn = [0xFFFFFFFF - (key & 0xFFFFFFFF) for key in sorted(old + own, reverse=True)[:KNN - 1]]
            nb[a + j, :min(degree, len(knn))] = knn[:degree]
            for t in knn[:H]:
                by_target.setdefault(t, []).append(a + j)
        targets = sorted(by_target)
        start = np.zeros(len(targets) + 1, np.int64)
        start[1:] = np.cumsum([len(by_target[t]) for t in targets])
        offers = [r for t in targets for r in by_target[t]]
        n_offers += len(offers)
        nb = link_host(X, nb, targets, start, offers, n_rows=b)
    return nb, {"inserted": hi - lo, "offers": n_offers, "orphans": orphans_host(nb, lo, hi)}


def check_insert_args(degree: int, n_rows: int, lo, hi, corpus_rows: int, insert_ef) -> None:
    """The refusals of `GraphIndex.insert` (and `insert_host`), each a ValueError before anything is launched."""
    if degree > MAX_BUILD_DEGREE:
        raise ValueError(f"degree={degree} is above {MAX_BUILD_DEGREE}: an insert has {KNN - 1} candidates a row, as a build has")
    if not _is_int(lo) or lo != n_rows:
        raise ValueError(f"lo={lo!r} must be the graph's row count {n_rows}: rows are inserted behind the rows the graph covers")
    if not _is_int(hi) or hi < lo or hi > corpus_rows:
        raise ValueError(f"hi={hi!r} must lie in [lo, rows of the corpus] = [{lo}, {corpus_rows}]")
    if hi >= 1 << 31:
        raise ValueError(f"hi={hi} must be below 2^31 (the graph holds int32 rows)")
    if not _is_int(insert_ef) or not (KNN - 1 <= insert_ef <= MAX_EF):
        raise ValueError(f"insert_ef={insert_ef!r} must be an integer in [{KNN - 1}, {MAX_EF}] (the walk returns {KNN - 1} candidates a row)")


# ---- the device path ---------------------------------------------------------------------------------------------------------------
def graph_link(corpus, neighbors, targets, offer_start, offers, n_rows: Optional[int] = None, threads: Optional[int] = None) -> None:
    """`arx_graph_link` (with `threads`: `arx_graph_link_tuned`) on the current stream, its one caller: `neighbors` (int32 device
    [>= n_rows, degree]) is rewritten in place.  `corpus` fp16 device [>= n_rows, dim]; `targets` int32 device [T], `offer_start` int32
    device [T + 1], `offers` int32 device [n_offers].  The library checks the contract: an `ArxError` naming the field, before any launch."""
    import torch
    from . import _lib
    lib = _lib.load()
    n_rows = int(corpus.shape[0]) if n_rows is None else int(n_rows)
    assert corpus.is_cuda and corpus.dtype == torch.float16 and corpus.dim() == 2 and corpus.is_contiguous() and corpus.shape[0] >= n_rows
    assert neighbors.is_cuda and neighbors.dtype == torch.int32 and neighbors.dim() == 2 and neighbors.shape[0] >= n_rows and neighbors.is_contiguous()
    for t in (targets, offer_start, offers):
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    assert offer_start.shape[0] == targets.shape[0] + 1
    name = "arx_graph_link"
    args = [corpus.data_ptr(), n_rows, int(corpus.shape[1]), neighbors.data_ptr(), int(neighbors.shape[1]), targets.data_ptr(), int(targets.shape[0]),
            offer_start.data_ptr(), offers.data_ptr(), int(offers.shape[0])]
    if threads is not None:
        name, args = name + "_tuned", args + [int(threads)]
    with torch.cuda.device(corpus.device):
        _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream(corpus.device).cuda_stream), name)


def graph_remap(neighbors, count: int, keep_words, word_rank, n_old: int) -> None:
    """`arx_graph_remap` on the current stream, its one caller: the first `count` rows of `neighbors` (int32 device, the kept rows
    already moved) are renumbered in place.  `keep_words`, `word_rank`: the bitmap and `mutation.plan_device`'s plan over `n_old` rows."""
    import torch
    from . import _lib
    assert neighbors.is_cuda and neighbors.dtype == torch.int32 and neighbors.dim() == 2 and neighbors.is_contiguous() and neighbors.shape[0] >= count
    assert keep_words.is_cuda and keep_words.dtype in (torch.int64, torch.uint64) and keep_words.shape[0] >= (n_old + 63) // 64
    assert word_rank.is_cuda and word_rank.dtype == torch.int64 and word_rank.shape[0] >= (n_old + 63) // 64 + 1
    with torch.cuda.device(neighbors.device):
        _lib.check(_lib.load().arx_graph_remap(neighbors.data_ptr(), int(count), int(neighbors.shape[1]), keep_words.data_ptr(), word_rank.data_ptr(),
                                               int(n_old), torch.cuda.current_stream(neighbors.device).cuda_stream), "arx_graph_remap")


def best_of(scores, ids, width: int):
    """int64 device [m, width]: per row the ids of the `width` best (score, id) pairs by the kernel's key order (score desc by order
    word, id asc; an id < 0 is no pair), -1 padded.  `scores` f32 device [m, w], `ids` int64 device [m, w].  Two stable torch sorts."""
    import torch
    u = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    word = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)
    word = torch.where(torch.isnan(scores), torch.zeros_like(word), word)
    word = torch.where(ids >= 0, word, torch.full_like(word, -1))
    by_id = torch.sort(torch.where(ids >= 0, ids, torch.full_like(ids, 1 << 40)), dim=1, stable=True).indices
    by_word = torch.sort(word.gather(1, by_id), dim=1, descending=True, stable=True).indices
    out = ids.gather(1, by_id).gather(1, by_word)[:, :width]
    if out.shape[1] < width:
        out = torch.cat([out, torch.full((out.shape[0], width - out.shape[1]), -1, dtype=torch.int64, device=out.device)], dim=1)
    return out.contiguous()


def graph_search(corpus, neighbors, q, entries, k: int, ef: int, max_iters: int, allow=None, idx_base: int = 0, threads: Optional[int] = None,
                 ws=None, n_rows: Optional[int] = None):
    """`arx_graph_search` (or, with `threads` given, `arx_graph_search_tuned`) on the current stream, the one call into the library.
    `corpus` fp16 device [n_rows, dim], `neighbors` int32 device [n_rows, degree], `q` fp16 device [nq, dim], `entries` int32 device
    [nq, n_entries], `allow` int64 / uint64 device words or None -> (scores f32 [nq, k], ids int64 [nq, k], scored int64 [nq],
    expanded int64 [nq]) on the device.  `ws`: a device uint8 tensor to use as the workspace if it is large enough.  The library checks
    the contract; a refusal is an `ArxError` naming the field, before any launch."""
    import torch
    from . import _lib
    lib = _lib.load()
    n_rows = int(corpus.shape[0]) if n_rows is None else int(n_rows)
    dim, nq, degree, n_entries = int(corpus.shape[1]), int(q.shape[0]), int(neighbors.shape[1]), int(entries.shape[1])
    assert corpus.is_cuda and corpus.dtype == torch.float16 and corpus.is_contiguous() and corpus.shape[0] >= n_rows
    assert q.is_cuda and q.dtype == torch.float16 and q.dim() == 2 and q.shape[1] == dim and q.is_contiguous()
    assert neighbors.is_cuda and neighbors.dtype == torch.int32 and neighbors.dim() == 2 and neighbors.shape[0] >= n_rows and neighbors.is_contiguous()
    assert entries.is_cuda and entries.dtype == torch.int32 and entries.shape == (nq, n_entries) and entries.is_contiguous()
    if allow is not None:
        assert allow.is_cuda and allow.dtype in (torch.int64, torch.uint64) and allow.is_contiguous()
        assert allow.dim() == 1 and allow.shape[0] == (n_rows + 63) // 64
    out = [torch.empty((nq, k), dtype=torch.float32, device=q.device), torch.empty((nq, k), dtype=torch.int64, device=q.device),
           torch.empty((nq,), dtype=torch.int64, device=q.device), torch.empty((nq,), dtype=torch.int64, device=q.device)]
    if nq == 0:
        return tuple(out)
    need = lib.arx_graph_workspace_bytes(n_rows, nq, dim, degree, int(k), int(ef), int(max_iters), n_entries)
    if need < 0:
        raise _lib.ArxError(f"arx_graph_search: unsupported shape n_rows={n_rows} nq={nq} dim={dim} degree={degree} k={k} ef={ef} "
                            f"max_iters={max_iters} n_entries={n_entries}")
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
    name = "arx_graph_search"
    args = [corpus.data_ptr(), n_rows, dim, neighbors.data_ptr(), degree, q.data_ptr(), nq, entries.data_ptr(), n_entries,
            None if allow is None else allow.data_ptr(), int(k), int(ef), int(max_iters)] + [t.data_ptr() for t in out] + \
           [int(idx_base), ws.data_ptr(), ws.numel() * ws.element_size()]
    if threads is not None:
        name, args = name + "_tuned", args + [int(threads)]
    with torch.cuda.device(q.device):
        _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream(q.device).cuda_stream), name)
    return tuple(out)


def _front(values, keep):
    """The kept entries of every row moved to its front in order (`values`, `keep` device [n, w]) -> (values, keep) so arranged."""
    import torch
    order = torch.sort((~keep).to(torch.uint8), dim=1, stable=True).indices
    return values.gather(1, order), keep.gather(1, order)


def assemble_device(knn, degree: int):
    """int32 device [n, degree]: `assemble_host` of the device k-NN lists `knn` (int32 / int64 [n, w], a row's valid entries distinct),
    with torch sorts: exactly the restatement's graph."""
    import torch
    n, H = int(knn.shape[0]), degree // 2
    dev = knn.device
    knn = knn.long()
    me = torch.arange(n, device=dev)[:, None]
    V, ok = _front(knn, (knn >= 0) & (knn < n) & (knn != me))
    fwd, fok = V[:, :H], ok[:, :H]
    # the forward edges (j -> i at position p) in (p asc, j asc) order, then a stable sort by i: rev(i) in (p asc, j asc) order
    src = me.expand(n, fwd.shape[1]).t()[fok.t()]
    dst = fwd.t()[fok.t()]
    mutual = torch.isin(dst * n + src, src * n + dst)             # j -> i where i -> j is a forward edge too: j is in fwd(i) already
    src, dst = src[~mutual], dst[~mutual]
    by_dst = torch.sort(dst, stable=True)
    dst, src = by_dst.values, src[by_dst.indices]
    first = torch.searchsorted(dst, torch.arange(n, device=dev))
    rank = torch.arange(dst.shape[0], device=dev) - first[dst]
    rev = torch.full((n, H), -1, dtype=torch.long, device=dev)
    rev[dst[rank < H], rank[rank < H]] = src[rank < H]
    out = torch.empty((n, degree), dtype=torch.int32, device=dev)
    for a in range(0, n, ASSEMBLE_ROWS):
        b = min(n, a + ASSEMBLE_ROWS)
        later, lok = V[a:b, H:], ok[a:b, H:]
        lok = lok & ~(later[:, :, None] == rev[a:b, None, :]).any(dim=2)
        row, rok = _front(torch.cat([fwd[a:b], rev[a:b], later], dim=1), torch.cat([fok[a:b], rev[a:b] >= 0, lok], dim=1))
        row = torch.where(rok, row, torch.full_like(row, -1))[:, :degree]
        if row.shape[1] < degree:
            row = torch.cat([row, torch.full((b - a, degree - row.shape[1]), -1, dtype=torch.long, device=dev)], dim=1)
        out[a:b] = row.to(torch.int32)
    return out


def knn_lists(index, ivf=None, nprobe: Optional[int] = None):
    """int32 device [n, KNN - 1]: every row's nearest other rows, local row numbers, -1 padded.  `index.search(X[a:b], KNN)` in batches
    (with `ivf` and `nprobe`: `ivf.search`, the approximate build); the row's own id is dropped where it is present, else the last entry."""
    import torch
    n = int(index.n_rows)
    X = index.corpus[:n]
    out = torch.empty((n, KNN - 1), dtype=torch.int32, device=X.device)
    for a in range(0, n, BUILD_BATCH):
        b = min(n, a + BUILD_BATCH)
        ids = (index.search(X[a:b], KNN)[1] if ivf is None else ivf.search(X[a:b], KNN, int(nprobe))[1])
        ids = torch.where(ids >= 0, ids - index.idx_base, ids)
        own = ids == torch.arange(a, b, device=X.device)[:, None]
        drop = torch.where(own.any(dim=1), own.to(torch.int32).argmax(dim=1), torch.full((b - a,), KNN - 1, device=X.device))
        keep = torch.arange(KNN, device=X.device)[None, :] != drop[:, None]
        out[a:b] = ids[keep].reshape(b - a, KNN - 1).to(torch.int32)
    return out


class GraphIndex:
    """The graph of a `ShardIndex`: `neighbors` (int32 device [n_rows, degree], -1 = no edge), `centroids` (a `ShardIndex` over the fp16
    entry centroids) and `medoid` (int32 device [n_entry_lists]: the row nearest every centroid)."""

    def __init__(self, index, neighbors, centroids_f16, medoid, info: Optional[Dict] = None):
        from .index import ShardIndex
        self.index = index
        self.neighbors = neighbors.contiguous()
        self.n_rows, self.degree = (int(v) for v in self.neighbors.shape)
        self.centroids_f16 = centroids_f16.contiguous()
        self.centroids = ShardIndex(self.centroids_f16, prefilter=None)
        self.n_entry_lists = int(self.centroids_f16.shape[0])
        self.medoid = medoid.contiguous()
        self.info = dict(info or {})
        self.stale = False                                       # set by `rows_added` / `rows_compacted`: the rows changed under the graph
        self.maintain, self.insert_ef = False, 64                # `HipCollection.build_graph(maintain=True, insert_ef=...)`: follow the rows
        self._ws = None
        self._buf, self._spare = self.neighbors, None            # `neighbors` is the first n_rows rows of `_buf` (`reserve`)
        self.inserted = self.orphans = 0                         # totals over every `insert`

    @classmethod
    def build(cls, index, degree: int = 32, n_entry_lists: Optional[int] = None, iters: int = 10, seed: int = 0, ivf=None,
              nprobe: Optional[int] = None) -> "GraphIndex":
        """k-NN lists (`knn_lists`: the exact self-join, n^2 work, or with `ivf=` and `nprobe=` the IVF search, approximate and what
        makes a large build affordable), `assemble_device`, and the entry points: `n_entry_lists` centroids (None: about sqrt(rows),
        in [1, 4096]) by `topics.kmeans` on a sample drawn as `IvfIndex.build` draws it (an `ivf` passed in has its centroids reused,
        unless `n_entry_lists` asks for another number), `medoid[c]` the row `index.search(centroids, 1)` names.  Deterministic: two
        builds with one seed give the same graph.  ValueError before any launch: `check_build_args`."""
        import torch
        from . import topics as T
        n = int(index.n_rows)
        reuse = ivf is not None and n_entry_lists in (None, ivf.n_lists)
        n_lists = check_build_args(n, int(index.dim), degree, ivf.n_lists if reuse else n_entry_lists, iters, nprobe=nprobe, has_ivf=ivf is not None)
        t0 = time.perf_counter()
        X = index.corpus[:n]
        knn = knn_lists(index, ivf=ivf, nprobe=nprobe)
        neighbors = assemble_device(knn, int(degree))
        if reuse:
            c16 = ivf.centroids_f16
        else:
            m = min(n, 256 * n_lists)
            if m == n:
                sample = X
            else:
                rows = np.sort(np.random.default_rng(seed).choice(n, m, replace=False)).astype(np.int64)
                sample = T.gather(index, torch.from_numpy(rows).to(X.device))
            c16 = T.kmeans(sample, n_lists, iters=int(iters), seed=seed)["centroids_f16"].contiguous()
        medoid = index.search(c16, 1)[1][:, 0]
        medoid = torch.where(medoid >= 0, medoid - index.idx_base, medoid).to(torch.int32)
        self = cls(index, neighbors, c16, medoid, {"approximate": ivf is not None})
        torch.cuda.synchronize(X.device)
        self.info["seconds"] = time.perf_counter() - t0
        return self

    def summary(self) -> Dict:
        """{rows, degree, edges, entry_lists, inserted, orphans, approximate, seconds}: `edges` the neighbour slots filled, `inserted`
        and `orphans` the totals of every `insert` (an orphan: an inserted row no list named when its insert ended)."""
        return {"rows": self.n_rows, "degree": self.degree, "edges": int((self.neighbors >= 0).sum().item()),
                "entry_lists": self.n_entry_lists, "inserted": self.inserted, "orphans": self.orphans, **self.info}

    def reserve(self, rows: int) -> None:
        """Make room for `rows` neighbour rows: `neighbors` stays a view of the first `n_rows` rows of the buffer."""
        import torch
        if self._buf.shape[0] < rows:
            buf = torch.full((int(rows), self.degree), -1, dtype=torch.int32, device=self._buf.device)
            buf[:self.n_rows] = self.neighbors
            self._buf, self._spare, self.neighbors = buf, None, buf[:self.n_rows]

    def insert(self, lo: int, hi: int, insert_ef: int = 64, n_entries: int = 8) -> Dict:
        """Link the rows [lo, hi) of `index.corpus` into the graph over [0, lo) (INTEGRATION.md "Keeping the graph"), in batches
        [a, b) of at most `BUILD_BATCH` rows: the candidates of a new row are the 31 best of its graph search over the a rows before the
        batch (k = 31, ef = `insert_ef`, from the medoids of its `n_entries` nearest entry centroids) and of the exact search of the
        batch among itself; its list is their first `degree`; its H = degree / 2 best are offered the row, one `arx_graph_link` over b
        rows a batch.  Nothing is rebuilt: the old rows' heads, the centroids and the medoids stay.  -> {inserted, offers, orphans,
        seconds}, `orphans` the inserted rows no row's list names afterwards (the walk cannot reach them; they are reported, not
        hidden).  ValueError before any launch: `check_insert_args`."""
        import torch
        from .index import ShardIndex
        X = self.index.corpus
        check_insert_args(self.degree, self.n_rows, lo, hi, int(X.shape[0]), insert_ef)
        E = min(int(n_entries), self.n_entry_lists) if _is_int(n_entries) else n_entries
        if not _is_int(E) or not (1 <= E <= MAX_QUERY_ENTRIES):
            raise ValueError(f"n_entries={n_entries!r} must be an integer in [1, {MAX_QUERY_ENTRIES}]")
        t0 = time.perf_counter()
        dev, H = X.device, self.degree // 2
        self.reserve(hi)
        nb = self._buf
        max_iters = max(1, min(int(insert_ef), max_iters_for(self.degree, E)))
        if self._ws is None:
            self._ws = torch.empty(256, dtype=torch.uint8, device=dev)
        n_offers = 0
        for a in range(lo, hi, BUILD_BATCH):
            b = min(hi, a + BUILD_BATCH)
            m, q = b - a, X[a:b]
            so, io, _, _ = graph_search(X, nb, q, self.entries(q, E), KNN - 1, int(insert_ef), max_iters, ws=self._ws, n_rows=a)
            sn, i_n = ShardIndex(q).search(q, KNN)
            own = i_n == torch.arange(m, device=dev)[:, None]                              # dropped as `knn_lists` drops it
            drop = torch.where(own.any(dim=1), own.to(torch.int32).argmax(dim=1), torch.full((m,), KNN - 1, device=dev))
            keep = torch.arange(KNN, device=dev)[None, :] != drop[:, None]
            sn, i_n = sn[keep].reshape(m, KNN - 1), i_n[keep].reshape(m, KNN - 1)
            knn = best_of(torch.cat([so, sn], dim=1), torch.cat([io, torch.where(i_n >= 0, i_n + a, i_n)], dim=1), KNN - 1)
            nb[a:b] = -1
            nb[a:b, :min(self.degree, KNN - 1)] = knn[:, :self.degree].to(torch.int32)
            # the offers (target = one of the row's H best, row) in the CSR form by target: a stable sort, as `assemble_device` sorts
            tgt = knn[:, :H]
            ok = tgt >= 0
            by_t = torch.sort(tgt[ok], stable=True)
            offers = torch.arange(a, b, device=dev)[:, None].expand(m, H)[ok][by_t.indices].to(torch.int32).contiguous()
            targets, counts = torch.unique_consecutive(by_t.values, return_counts=True)
            start = torch.zeros(targets.shape[0] + 1, dtype=torch.int32, device=dev)
            start[1:] = torch.cumsum(counts, 0)
            n_offers += int(offers.shape[0])
            graph_link(X, nb, targets.to(torch.int32).contiguous(), start, offers, n_rows=b)
        self.neighbors, self.n_rows = nb[:hi], int(hi)
        named = torch.zeros(hi + 1, dtype=torch.bool, device=dev)
        named[torch.where((self.neighbors >= lo) & (self.neighbors < hi), self.neighbors, torch.full_like(self.neighbors, hi)).long().flatten()] = True
        orphans = int(hi - lo - named[lo:hi].sum().item())
        self.inserted, self.orphans = self.inserted + (hi - lo), self.orphans + orphans
        torch.cuda.synchronize(dev)
        return {"inserted": hi - lo, "offers": n_offers, "orphans": orphans, "seconds": time.perf_counter() - t0}

    def remap(self, keep_words, word_rank, count: int, index=None) -> None:
        """Follow a stable compaction of the rows (`HipCollection.compact`): the kept rows' lists move (`arx_compact_rows`) and every
        entry is renumbered (`arx_graph_remap`: an edge to a removed row is dropped, the survivors move to the front).  `index`: the
        `ShardIndex` over the compacted rows.  The entry centroids are kept; the medoids are searched again, since rows moved."""
        import torch
        from .mutation import compact_rows_device
        n_old = self.n_rows
        if self._spare is None:
            self._spare = torch.empty_like(self._buf)
        compact_rows_device(self._buf, self._spare, n_old, keep_words, word_rank)
        graph_remap(self._spare, int(count), keep_words, word_rank, n_old)
        self._buf, self._spare = self._spare, self._buf
        self.neighbors, self.n_rows = self._buf[:int(count)], int(count)
        if index is not None:
            self.index = index
        medoid = self.index.search(self.centroids_f16, 1)[1][:, 0]
        self.medoid = torch.where(medoid >= 0, medoid - self.index.idx_base, medoid).to(torch.int32).contiguous()

    def rows_added(self, lo: int, hi: int, rows, index=None) -> None:
        """The shard grew by the rows [lo, hi) (`index`: the `ShardIndex` over it): with `maintain` they are linked in (`insert`, a walk
        of width `insert_ef`); without, they have no edges and the graph is stale until it is built again."""
        if not self.maintain:
            self.stale = True
            return
        if index is not None:
            self.index = index
        self.insert(lo, hi, insert_ef=self.insert_ef)

    def rows_compacted(self, keep_words, word_rank, count: int, index=None) -> None:
        """The shard's rows moved: with `maintain` the lists move and are renumbered (`remap`); without, the graph is stale."""
        if not self.maintain:
            self.stale = True
            return
        self.remap(keep_words, word_rank, count, index=index)

    def entries(self, q, n_entries: int):
        """int32 device [nq, n_entries]: the medoids of every query's `n_entries` nearest entry centroids (an exact search)."""
        import torch
        if not _is_int(n_entries) or not (1 <= n_entries <= min(MAX_QUERY_ENTRIES, self.n_entry_lists)):
            raise ValueError(f"n_entries={n_entries!r} must be an integer in [1, min({MAX_QUERY_ENTRIES}, entry lists = {self.n_entry_lists})]")
        _, ids = self.centroids.search(q, int(n_entries))
        return self.medoid[ids.clamp(min=0)].to(torch.int32).contiguous()

    def search(self, q, k: int, ef: int, allow=None, n_entries: int = 8, max_iters: Optional[int] = None, entries=None,
               threads: Optional[int] = None, counters: bool = False):
        """(scores f32 [nq, k], ids int64 [nq, k], scored int64 [nq]) on the device (`counters`: also `expanded` int64 [nq]): the
        beam search of width `ef` from the medoids of every query's `n_entries` nearest entry centroids (`entries`: int32 device
        [nq, E] to use instead; `n_entries` is lowered to the number of entry lists), at most `max_iters` iterations (None: `ef`,
        lowered to what the visited table admits: `max_iters_for`, 255 at degree 32, so an `ef` above that widens the beam but adds no iterations).  `allow` restricts what comes back as `ShardIndex.search(allow=)`
        does, not where the walk goes.  ids = local row + the index's idx_base.  Reuses a cached workspace."""
        import torch
        if entries is None:
            n_entries = min(int(n_entries), self.n_entry_lists) if _is_int(n_entries) else n_entries
            entries = self.entries(q, n_entries)
        E = int(entries.shape[1])
        if max_iters is None:
            max_iters = max(1, min(int(ef), max_iters_for(self.degree, E))) if _is_int(ef) else ef
        check_search_args(k, ef, max_iters, self.degree, E)
        if allow is not None:
            self.index._check_allow(allow)
        if self._ws is None:
            self._ws = torch.empty(256, dtype=torch.uint8, device=q.device)
        s, i, scored, expanded = graph_search(self.index.corpus, self.neighbors, q, entries, int(k), int(ef), int(max_iters), allow=allow,
                                              idx_base=self.index.idx_base, threads=threads, ws=self._ws, n_rows=self.index.n_rows)
        return (s, i, scored, expanded) if counters else (s, i, scored)
