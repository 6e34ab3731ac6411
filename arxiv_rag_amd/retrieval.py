"""The retrieval pipeline `HipCollection.query` and `search_queries` share, between "the queries are an fp16 device matrix" and "rerank":

    check_shared_query(...)                  the refusals both front ends state (each front end adds its own)
    filters = RowFilters(metadata, device, keep_mask=..., documents=..., columns=...)
    hit = retrieve(index, q, filters, n_results, where=..., mmr_lambda=..., hybrid_alpha=..., keyword=...)

`RowFilters` turns `where`, `where_document` and the keep-mask into the row bitmaps of the masked searches; `retrieve` picks the search
(`search_range`, `search_grouped`, `search_filtered_grouped`, `search_distributed`), re-orders by MMR and fuses with BM25, the keyword
side restricted by the dense side's bitmaps.  Index construction, reranking and the shape of the results stay with the front ends.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np


def check_shared_query(n_results: int, *, hybrid_alpha, hybrid_filters: bool, reranker, mmr_lambda, n_fetch: int, fetch_refusal: str,
                       filters_first: Sequence[Tuple[str, bool]] = (), filters: Sequence[Tuple[str, bool]] = ()) -> None:
    """The refusals both front ends have, each a ValueError: a row filter with `hybrid_alpha` (lifted by `hybrid_filters`), and the
    `mmr_lambda` checks.  `filters_first` / `filters`: the front end's row filters as (the subject of its refusal, e.g. "where cannot be
    combined" or "a collection built with dedup_threshold cannot be queried"; whether that filter is given), in the front end's order:
    those it refuses before the `mmr_lambda` checks and those after.  `n_fetch`: the candidates MMR picks from, `fetch_refusal`: what
    the front end says when it is not in [n_results, 32]."""
    def refuse_filters(subjects):
        for subject, given in subjects:
            if given and hybrid_alpha is not None and not hybrid_filters:
                raise ValueError(f"{subject} with hybrid_alpha: the BM25 keyword search has no row filter")
    refuse_filters(filters_first)
    if mmr_lambda is not None:
        if reranker is not None or hybrid_alpha is not None:
            raise ValueError("mmr_lambda cannot be combined with reranker or hybrid_alpha: MMR re-orders the cosine search's candidates only")
        if not (0.0 <= float(mmr_lambda) <= 1.0):
            raise ValueError(f"mmr_lambda={mmr_lambda} must be in [0, 1]")
        if not (1 <= n_results <= n_fetch <= 32):
            raise ValueError(fetch_refusal)
    refuse_filters(filters)


HYBRID_HOST_CANDIDATES = 32        # the candidate lists' length limit without `hybrid_on_device`
HYBRID_DEVICE_CANDIDATES = 1024    # ... and with it (`arx_bm25_search_wide`, `arx_range_search`, `arx_hybrid_fuse`)


def check_hybrid_on_device(n_candidates: int, *, per_query_filters: bool = False, world: int = 1) -> None:
    """The refusals of a hybrid search with `hybrid_on_device`, each a ValueError with its reason."""
    if n_candidates > HYBRID_DEVICE_CANDIDATES:
        raise ValueError(f"n_candidates={n_candidates} must be at most {HYBRID_DEVICE_CANDIDATES} with hybrid_on_device (the candidate "
                         f"lists' length limit on the device)")
    if n_candidates > HYBRID_HOST_CANDIDATES and per_query_filters:
        raise ValueError(f"n_candidates={n_candidates} > {HYBRID_HOST_CANDIDATES} cannot be combined with per-query filter lists: the range "
                         f"search that fetches the long dense list takes one bitmap per call")
    if n_candidates > HYBRID_HOST_CANDIDATES and world > 1:
        raise ValueError(f"n_candidates={n_candidates} > {HYBRID_HOST_CANDIDATES} needs a single GPU rank: a cross-rank merge of long "
                         f"candidate lists is out of scope")


class RowFilters:
    """The row bitmaps of one shard: `where` (evaluated on the host, or on the device with `where_on_device`), `where_document` and the
    keep-mask, and-ed.  A bitmap is a device int64 tensor of ceil(n_rows / 64) words in the convention of `where.pack_bitmap`; whichever
    way it is built, its bits are the same.  The count that comes with it only steers which path the masked search takes.

    `metadata`: the dicts `where` reads, rows [lo, hi) of it being the shard's.  `keep_mask`: host bool [n_rows], the rows to search at
    all (`keep_words`: its bitmap, where the front end has it on the device already).  `documents` / `columns`: callables returning the
    shard's `where_document.DocumentStore` / `where_device.MetadataColumns`, for a front end that keeps its own (one without texts
    raises its refusal there); without them the store is built from `texts()` and the columns from `metadata` when a filter first
    needs them.  `cache`: the dict `where.evaluate` keeps its columns in.  `count_both`: False leaves the count of a per-query bitmap
    that and-s a `where` with a `where_document` unknown (None) instead of waiting for the device to count it.  `document_regex`
    (False = nothing changes): `where_document` also takes `$regex` / `$not_regex` (`compile_where_document(f, regex=True)`)."""

    def __init__(self, metadata: Sequence[Dict], device, lo: int = 0, hi: Optional[int] = None, *, keep_mask=None, keep_words=None,
                 documents: Optional[Callable] = None, texts: Optional[Callable] = None, columns: Optional[Callable] = None,
                 where_on_device: bool = False, cache: Optional[Dict] = None, count_both: bool = True, document_regex: bool = False):
        self.metadata, self.device, self.lo, self.hi = metadata, device, lo, len(metadata) if hi is None else hi
        self.n_rows = self.hi - self.lo
        self.keep_mask = None if keep_mask is None else np.asarray(keep_mask, dtype=bool)
        self._keep_words = keep_words
        self._documents, self._texts, self._columns, self.where_on_device = documents, texts, columns, bool(where_on_device)
        self.cache = {} if cache is None else cache
        self.count_both = count_both
        self.document_regex = bool(document_regex)

    def documents(self):
        if self._documents is None:
            from .where_document import DocumentStore
            store = DocumentStore(self._texts(), device=self.device)
            self._documents = lambda: store
        return self._documents()

    def columns(self):
        if self._columns is None:
            from .where_device import MetadataColumns
            cols = MetadataColumns(self.metadata, self.lo, self.hi, self.device)
            self._columns = lambda: cols
        return self._columns()

    def _upload(self, mask):
        import torch
        from .where import pack_bitmap
        return torch.from_numpy(pack_bitmap(mask).view(np.int64)).to(self.device)

    def keep_words(self):
        if self._keep_words is None and self.keep_mask is not None:
            self._keep_words = self._upload(self.keep_mask)
        return self._keep_words

    def _doc_words(self, doc_tree, folds):
        """The bitmap of a compiled `where_document` (None: None), folded once per distinct tree and call (`folds`)."""
        if doc_tree is not None and doc_tree not in folds:
            folds[doc_tree] = self.documents().fold(doc_tree)
        return folds.get(doc_tree)

    def _and_with(self, doc_tree, folds):
        """What the device evaluation and-s into a `where` bitmap: the `where_document` bitmap and the keep-bitmap (None: neither)."""
        key = ("&", doc_tree)
        if key not in folds:
            docs, keep = self._doc_words(doc_tree, folds), self.keep_words()
            folds[key] = (docs & keep).contiguous() if docs is not None and keep is not None else (keep if docs is None else docs)
        return folds[key]

    def _allow(self, tree, doc_tree, folds, count=True):
        """(bitmap, allowed rows) of a compiled `where`, a compiled `where_document` and the keep-mask; (None, None): none of the three."""
        if tree is not None and self.where_on_device:
            bits, counts = self.columns().allow_many([tree], self._and_with(doc_tree, folds))
            return bits[0], counts[0]
        if tree is None:
            words = self._and_with(doc_tree, folds)
            if doc_tree is not None:
                return words, self.documents().count(words)
            return words, None if words is None else int(self.keep_mask.sum())
        from .where import evaluate
        mask = evaluate(tree, self.metadata, self.lo, self.hi, cache=self.cache)
        if self.keep_mask is not None:
            mask = mask & self.keep_mask
        words, n_allowed = self._upload(mask), int(mask.sum())
        if doc_tree is not None:
            words = (words & self._doc_words(doc_tree, folds)).contiguous()
            n_allowed = self.documents().count(words) if count else None
        return words, n_allowed

    def allow_of(self, where, where_document=None):
        """-> (bitmap or None, n_allowed or None) of one `where` dict, one `where_document` dict (either may be None) and the keep-mask."""
        from .where import compile_where
        from .where_document import compile_where_document
        tree = compile_where(where) if where is not None else None
        return self._allow(tree, compile_where_document(where_document, regex=self.document_regex) if where_document is not None else None, {})

    def per_query(self, nq: int, where, where_document=None):
        """`where` / `where_document` with one entry per query (a list or tuple of `nq` dicts or Nones; a dict or None is repeated) ->
        (bitmaps, filter_of, counts): the bitmap of every distinct (where, where_document) pair, the keep-mask and-ed in (a list of
        device tensors, or the one [F, W] tensor the device evaluation wrote when every pair has a `where`), for each query the index
        of its bitmap (host), and the bitmaps' allowed rows.  A pair without any filter gets every row of the shard."""
        import torch
        from .filter_sets import distinct_filters, per_query_list
        from .where import compile_where
        from .where_document import compile_where_document
        pairs, filter_of = distinct_filters(per_query_list(where, nq, "where"), per_query_list(where_document, nq, "where_document"))
        if any(d is not None for _, d in pairs):
            self.documents()
        trees = []
        for w, d in pairs:                                       # (a pair's where_document first: the same refusal comes first as ever)
            doc_tree = compile_where_document(d, regex=self.document_regex) if d is not None else None
            trees.append((compile_where(w) if w is not None else None, doc_tree))
        folds, evaluated = {}, {}
        mine = [j for j, (tree, _) in enumerate(trees) if tree is not None]
        if self.where_on_device and self.n_rows > 0 and mine:
            # every `where` of the batch in one `arx_where_eval` per 64, each with its own where_document / keep bitmap and-ed in
            ands = [self._and_with(trees[j][1], folds) for j in mine]
            if len({trees[j][1] for j in mine}) == 1:
                and_with = ands[0]
            else:
                ones = torch.full(((self.n_rows + 63) // 64,), -1, dtype=torch.int64, device=self.device)
                and_with = torch.stack([ones if a is None else a for a in ands]).contiguous()
            bits, counts = self.columns().allow_many([trees[j][0] for j in mine], and_with)
            if len(mine) == len(pairs):                          # the [F, W] tensor the kernel wrote is what the search reads, without a copy
                return bits, filter_of, counts
            evaluated = {j: (bits[t], counts[t]) for t, j in enumerate(mine)}
        bitmaps, counts = [], []
        for j, (tree, doc_tree) in enumerate(trees):
            words, n_allowed = evaluated[j] if j in evaluated else self._allow(tree, doc_tree, folds, count=self.count_both)
            if words is None:                                    # no filter for these queries: every row of the shard
                words, n_allowed = torch.full(((self.n_rows + 63) // 64,), -1, dtype=torch.int64, device=self.device), self.n_rows
            bitmaps.append(words)
            counts.append(n_allowed)
        return bitmaps, filter_of, counts


@dataclass
class Retrieved:
    """What `retrieve` found, as numpy arrays on the host: `scores` f32 / `ids` int64 [Q, width], (-inf or nan, -1) padded; the others
    None unless their mode ran."""
    scores: np.ndarray
    ids: np.ndarray
    groups: Optional[np.ndarray] = None          # grouped: int32 [Q, P], the `group_of` value of every returned group (-1 pads)
    group_sizes: Optional[np.ndarray] = None     # grouped: [Q, P], the chunks returned for each
    truncated: Optional[list] = None             # min_score: one bool per query, more rows qualified than were asked for
    mmr: Optional[np.ndarray] = None             # mmr_lambda: the objective at each pick
    hybrid: Optional[np.ndarray] = None          # hybrid_alpha: the fused scores ...
    keyword: Optional[np.ndarray] = None         # ... and the BM25 ones (nan where the row was not in the keyword list)
    ivf_scanned: Optional[np.ndarray] = None     # nprobe: int64 [Q], the rows scored for every query
    ivf_hits: Optional[np.ndarray] = None        # nprobe with per-query filters or min_score: int64 [Q], the rows at or above the threshold
    binary_count: Optional[np.ndarray] = None    # binary_candidates: int64 [Q], the Hamming candidates rescored for every query
    pq_count: Optional[np.ndarray] = None        # pq_candidates: int64 [Q], the PQ candidates rescored for every query
    graph_scored: Optional[np.ndarray] = None    # graph_ef: int64 [Q], the rows the graph walk scored for every query
    base: Optional[np.ndarray] = None            # boost_weight: the cosine of every returned row (`scores` holds the boosted values)


def _retrieve_ivf(ivf, q, k: int, nprobe: int, filters: RowFilters, where, where_document, per_query: bool, min_score, out: Retrieved):
    """The `nprobe` case of `retrieve` -> (scores, ids) on the device, `out.ivf_scanned` / `ivf_hits` / `truncated` filled: one dict and
    no `min_score` is `IvfIndex.search`, per-query filter lists or a `min_score` one `IvfIndex.search_many` call."""
    import torch
    nq = q.shape[0]
    if not per_query and min_score is None:
        s, i, scanned = ivf.search(q, k, nprobe, allow=filters.allow_of(where, where_document)[0])
        out.ivf_scanned = scanned.cpu().numpy()
        return s, i
    if per_query:                                                # one IVF call per batch, whatever the number of distinct filters
        bitmaps, filter_of, _ = filters.per_query(nq, where, where_document)
        allows = bitmaps if torch.is_tensor(bitmaps) else torch.stack(list(bitmaps)).contiguous()
        fo = torch.tensor(list(filter_of), dtype=torch.int32, device=q.device)
    else:
        allow, _ = filters.allow_of(where, where_document)
        allows = None if allow is None else allow[None].contiguous()
        fo = None if allow is None else torch.zeros(nq, dtype=torch.int32, device=q.device)
    if min_score is not None:
        from .ranging import thresholds
        min_score = thresholds(min_score, nq)
    s, i, scanned, hits = ivf.search_many(q, k, nprobe, allows=allows, filter_of=fo, min_score=min_score)
    out.ivf_scanned, out.ivf_hits = scanned.cpu().numpy(), hits.cpu().numpy()
    if min_score is not None:
        out.truncated = (out.ivf_hits > k).tolist()
    return s, i


def retrieve(index, q, filters: RowFilters, n_results: int, *, n_candidates: int = 32, reranked: bool = False, where=None, where_document=None,
             min_score=None, grouped: bool = False, chunks_per_group: int = 1, mmr_lambda: Optional[float] = None,
             hybrid_alpha: Optional[float] = None, keyword=None, query_texts: Optional[Sequence[str]] = None,
             hybrid_on_device: bool = False, world: int = 1, nprobe: Optional[int] = None, ivf=None,
             binary_candidates: Optional[int] = None, binary=None, boost_weight=None, prior=None,
             max_abs_prior: Optional[float] = None, pq_candidates: Optional[int] = None, pq=None,
             graph_ef: Optional[int] = None, graph=None, graph_entries: int = 8) -> Retrieved:
    """One search of the fp16 device queries `q` over `index` (a `ShardIndex`), in the mode the arguments name, every refusal behind it.
    The width: a range search (`min_score`) returns up to `n_candidates` rows with `reranked` and `n_results` without, a grouped search
    `n_results` groups, every other search `n_candidates` rows when something picks among them afterwards (`reranked`, `mmr_lambda`,
    `hybrid_alpha`) and `n_results` otherwise.  `where` / `where_document`: a dict each, or a list with one entry per query.
    `mmr_lambda`: `mmr.mmr_select` picks `n_results` of the candidates, which come back in pick order.  `hybrid_alpha`: `keyword` (a
    `keyword.KeywordIndex`, or a callable that builds one) fetches `n_candidates` rows for `query_texts`, restricted by the bitmaps the
    cosine search was given, and `keyword.fuse` keeps the best `n_candidates` (`reranked`) or `n_results`.
    `hybrid_on_device` (False = nothing changes; read only with `hybrid_alpha`): the fusion runs on the device and `n_candidates` may
    be up to 1024.  The dense list is the search above for `n_candidates <= 32` and `index.search_range(q, -inf, n_candidates)` beyond
    (the same score bits, by that kernel's contract), the keyword list is `KeywordIndex.search_wide`'s under the same bitmaps, the
    fusion is `keyword.fuse_device`, and the four result arrays cross to the host once.  For `n_candidates <= 32` the result is the
    default path's, bit for bit.  ValueError: `n_candidates > 1024`; `n_candidates > 32` with per-query filter lists (the range
    search takes one bitmap per call) or with `world > 1` ranks (a cross-rank merge of long lists is out of scope).
    `nprobe` (None = nothing changes) with `ivf` (an `ivf.IvfIndex` over `index`): the IVF probe search (INTEGRATION.md "IVF probe
    search"): the exact top-k of the rows of every query's `nprobe` nearest lists, under the one bitmap of `where`, `where_document`
    and the keep-mask; `ivf_scanned` holds the rows scored.  MMR and a reranker consume its candidate list as any other.  With
    per-query `where` / `where_document` lists (the bitmaps of `filters.per_query`, the keep-mask and-ed into each) or with `min_score`
    (a float or one per query; the width is the top-k search's, at most 32) the batch is one
    `IvfIndex.search_many` call whatever the number of distinct filters: only rows at or above the threshold come back, `ivf_hits`
    holds their exact number per query (without `min_score`: the rows scored) and, with `min_score`, `truncated` is
    `ivf_hits > width`.
    `binary_candidates` (None = nothing changes) with `binary` (a `binary.BinaryIndex` over `index`): the binary-code search
    (INTEGRATION.md "Binary-code search"): every query's first `binary_candidates` visible rows by (Hamming distance of the sign bits,
    row), under the one bitmap of `where`, `where_document` and the keep-mask, rescored exactly; `binary_count` holds the candidates
    rescored.  MMR and a reranker consume the list as any other.  `binary_candidates` lies in [width, 256].
    `boost_weight` (None = nothing changes; a number or one per query) with `prior` (device f32 [rows of `index`]) and
    `max_abs_prior` (its largest |finite value|, None = measured): the boosted search (INTEGRATION.md "Boosted search"): the exact
    top rows by cosine + weight * prior under the one bitmap of `where`, `where_document` and the keep-mask
    (`ShardIndex.search_boosted`); `scores` holds the boosted values and `base` the cosines of the same rows, in the same order
    (MMR's pick order included).  MMR and a reranker consume the list as any other.  The weight must be finite.
    `pq_candidates` (None = nothing changes) with `pq` (a `pq.PqIndex` over `index`): the product-quantised search (INTEGRATION.md
    "Product-quantised search"): every query's first `pq_candidates` visible rows by (sum of its byte tables over the row's PQ code,
    row), under the one bitmap of `where`, `where_document` and the keep-mask, rescored exactly; `pq_count` holds the candidates
    rescored.  MMR and a reranker consume the list as any other.  `pq_candidates` lies in [width, 256].
    `graph_ef` (None = nothing changes) with `graph` (a `graph.GraphIndex` over `index`) and `graph_entries`: the graph search
    (INTEGRATION.md "Graph search"): a beam search of width `graph_ef` over the k-NN graph from the medoids of every query's
    `graph_entries` nearest entry centroids; the one bitmap of `where`, `where_document` and the keep-mask restricts what comes back,
    not where the walk goes; `graph_scored` holds the rows scored.  MMR and a reranker consume the list as any other.  `graph_ef`
    lies in [width, 512]; a stale graph is refused.
    ValueError for each of these five modes (`modes.check_modes`, before anything is launched): what `modes.MODES` says it cannot be
    combined with (each other, `hybrid_alpha`, `grouped`, `min_score` and per-query filter lists, the last two let through for
    `nprobe`), `world > 1`, its index missing, a width above 32."""
    import torch
    from .filter_sets import is_per_query
    from .modes import check_modes
    nq = q.shape[0]
    k = n_candidates if (reranked or hybrid_alpha is not None or mmr_lambda is not None) else n_results
    per_query = is_per_query(where) or is_per_query(where_document)
    weights = check_modes(
        {"graph_ef": graph_ef, "pq_candidates": pq_candidates, "boost_weight": boost_weight, "binary_candidates": binary_candidates,
         "nprobe": nprobe},
        {"graph_ef": dict(has_index=graph is not None, stale=getattr(graph, "stale", False), n_entries=graph_entries,
                          n_entry_lists=getattr(graph, "n_entry_lists", 0), degree=getattr(graph, "degree", 32)),
         "pq_candidates": dict(has_index=pq is not None),
         "boost_weight": dict(has_index=prior is not None, n_queries=nq, max_abs_prior=0.0 if max_abs_prior is None else max_abs_prior),
         "binary_candidates": dict(has_index=binary is not None),
         "nprobe": dict(has_index=ivf is not None, n_lists=getattr(ivf, "n_lists", 0), let_through=("per_query", "min_score"))},
        per_query=per_query, hybrid_alpha=hybrid_alpha, group_by=grouped, min_score=min_score, world=world, n_width=k)
    boost_weight = boost_weight if weights is None else weights
    out = Retrieved(None, None)
    kw_filter_of = None
    on_device = hybrid_alpha is not None and bool(hybrid_on_device)
    if on_device:
        check_hybrid_on_device(n_candidates, per_query_filters=per_query, world=world)
    long_lists = on_device and n_candidates > HYBRID_HOST_CANDIDATES
    if graph_ef is not None:
        s, i, scored = graph.search(q, k, int(graph_ef), allow=filters.allow_of(where, where_document)[0], n_entries=int(graph_entries))
        out.graph_scored = scored.cpu().numpy()
    elif nprobe is not None:
        s, i = _retrieve_ivf(ivf, q, k, int(nprobe), filters, where, where_document, per_query, min_score, out)
    elif binary_candidates is not None:
        s, i, count = binary.search(q, k, int(binary_candidates), allow=filters.allow_of(where, where_document)[0])
        out.binary_count = count.cpu().numpy()
    elif pq_candidates is not None:
        s, i, count = pq.search(q, k, int(pq_candidates), allow=filters.allow_of(where, where_document)[0])
        out.pq_count = count.cpu().numpy()
    elif boost_weight is not None:
        allow, n_allowed = filters.allow_of(where, where_document)
        s, base, i = index.search_boosted(q, k, prior, boost_weight, allow=allow, n_allowed=n_allowed, max_abs_prior=max_abs_prior)
    elif per_query:
        from .index import search_filtered_grouped
        bitmaps, filter_of, counts = filters.per_query(nq, where, where_document)
        s, i = search_filtered_grouped(index, q, k, bitmaps, filter_of, counts)
        if hybrid_alpha is not None:
            allow = bitmaps if torch.is_tensor(bitmaps) else torch.stack(list(bitmaps)).contiguous()
            kw_filter_of = torch.tensor(list(filter_of), dtype=torch.int32, device=q.device)
    else:
        allow, n_allowed = filters.allow_of(where, where_document)
        if min_score is not None:
            from .ranging import thresholds
            s, i, counts = index.search_range(q, thresholds(min_score, nq), n_candidates if reranked else n_results, allow=allow,
                                              n_allowed=n_allowed)
            out.truncated = (counts > s.shape[1]).cpu().tolist()
        elif long_lists:                                         # every visible row qualifies: the exact top n_candidates
            from .ranging import thresholds
            s, i, _ = index.search_range(q, thresholds(float("-inf"), nq), n_candidates, allow=allow, n_allowed=n_allowed)
        elif grouped:
            s, i, grp = index.search_grouped(q, n_results, chunks_per_group, allow=allow, n_allowed=n_allowed)
            out.groups = grp.cpu().numpy()
            s, i = s.reshape(nq, -1), i.reshape(nq, -1)          # group by group; the padding stays (-inf, -1)
        else:
            s, i = index.search_distributed(q, k, allow=allow, n_allowed=n_allowed)
    if mmr_lambda is not None:
        from .mmr import mmr_select
        order, mmr_val = mmr_select(index, q, i, n_results, float(mmr_lambda))
        pos = order.clamp(min=0).long()                          # (-1 where fewer than n_results rows were found: masked here)
        s = torch.where(order >= 0, s.gather(1, pos), torch.full_like(mmr_val, float("-inf")))
        i = torch.where(order >= 0, i.gather(1, pos), torch.full_like(pos, -1))
        if boost_weight is not None:
            base = torch.where(order >= 0, base.gather(1, pos), torch.full_like(mmr_val, float("-inf")))
        out.mmr = mmr_val.cpu().numpy()
    if on_device:
        from .keyword import fuse_device
        kw = keyword() if callable(keyword) else keyword
        if world > 1:                                            # (n_candidates <= 32: the cross-rank merge of the short lists)
            ks, ki = kw.search_distributed(list(query_texts), n_candidates, allow=allow, filter_of=kw_filter_of)
        else:
            ks, ki = kw.search_wide(list(query_texts), n_candidates, allow=allow, filter_of=kw_filter_of)
        fused = fuse_device(s.float(), i, ks, ki, float(hybrid_alpha), n_candidates if reranked else n_results)
        out.hybrid, out.ids, out.scores, out.keyword = (t.cpu().numpy() for t in fused)
        return out
    out.scores, out.ids = s.cpu().numpy(), i.cpu().numpy()
    if boost_weight is not None:
        out.base = base.cpu().numpy()
    if grouped:
        out.group_sizes = (out.ids.reshape(nq, n_results, chunks_per_group) >= 0).sum(axis=2)
    if hybrid_alpha is not None:
        from .keyword import fuse
        kw = keyword() if callable(keyword) else keyword
        ks, ki = kw.search_distributed(list(query_texts), n_candidates, allow=allow, filter_of=kw_filter_of)
        out.hybrid, out.ids, out.scores, out.keyword = fuse(out.scores, out.ids, ks.cpu().numpy(), ki.cpu().numpy(), float(hybrid_alpha),
                                                            n_candidates if reranked else n_results)
    return out
