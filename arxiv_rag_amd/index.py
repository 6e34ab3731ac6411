"""HBM-resident brute-force cosine top-k (`retrieval.top_k: 10`, 3-chunks/pipeline/config.yaml:63-64).

One `ShardIndex` per process/GPU holds that rank's rows of the fp16 corpus (the rows it encoded; they
never move).  `search` = local exact top-k through the C ABI; `search_distributed` adds the single
exchange step of the path: an all-gather of the per-shard [Q, k] partial results over RCCL, then a
merge kernel (ties -> lower global row id).
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional, Tuple

import torch

from . import _lib
from .ranging import device_thresholds


class ShardIndex:
    def __init__(self, corpus_f16: torch.Tensor, idx_base: int = 0, prefilter: Optional[str] = None, adaptive: bool = False,
                 i8_max_queries: Optional[int] = None, max_row_norm: Optional[float] = None, centre_query: Optional[bool] = None):
        """`prefilter="int8"` (dim % 128 == 0, <= 1024): also keep an int8 representation of the rows (+50 % memory) and run the first
        pass of every search over it — the same exact top-k (`arx_topk_search_i8`), 1.4-1.8x the queries per second on rows that
        quantise well (the index quantises rows minus the shard's mean and, `centre_query`, queries minus their component along it, so rows
        sharing a common component of any size still do; profiles/r04/int8_centred_index.md).  `adaptive=True` (the CLI and `HipCollection` pass it): the index reads the certificate counters after its
        first searches (a 16-byte copy + stream sync each) and switches the pre-filter OFF for good when more than a quarter of a
        batch's queries overflowed their candidate lists — clustered / outlier-heavy rows on which the int8 bound is too slack to
        pay (answers are exact either way; this only picks the faster first pass).
        `i8_max_queries`: THIS index's crossover (query batches above it take the fp16 first pass; None = the library default, 0 = never
        int8) — a per-index policy passed with every call, not a library setting.
        `centre_query`: the int8 pass also quantises the QUERY minus its component along the shard's mean direction (ARX_TOPK_I8_CENTRE_QUERY: one
        more instruction per value in pass A's epilogue, same exact answers) — what keeps the pre-filter useful on strongly anisotropic rows
        (mean pairwise cosine beyond ~0.75).  None (default) = decided from the built index: on when |mean|^2 >= 0.25.
        `max_row_norm`: a bound on the rows' L2 norms the caller vouches for; None (default) = measured on the device
        (`arx_rows_max_norm_f16`, again whenever the tensor was written to) — the exactness certificate's tolerance scales with it, so
        the answers are the exact top-k of the dot products for rows of ANY norm, cosine when they are unit."""
        assert corpus_f16.is_cuda and corpus_f16.dtype == torch.float16 and corpus_f16.dim() == 2
        assert corpus_f16.stride(1) == 1 and corpus_f16.stride(0) == corpus_f16.shape[1], "corpus must be dense row-major"
        assert prefilter in (None, "int8")
        self.lib = _lib.load()
        self.corpus = corpus_f16
        self.n_rows, self.dim = corpus_f16.shape
        self.idx_base = int(idx_base)
        self._ws: Optional[torch.Tensor] = None            # workspace of plain `search` calls (and of the LAST call: certificate_stats)
        self._last_ws: Optional[torch.Tensor] = None
        self._ws_masked = {}                               # the index's own workspaces of `search(allow=...)` ("filtered"), of
        self._last_ws_masked = {}                          # `search_prefix` / `nearest_earlier` ("prefix") and of `search_filtered_many`
                                                           # ("filtered_multi") calls, and those of the LAST calls
        self._i8: Optional[torch.Tensor] = None
        self._i8_version = -1
        self._adaptive, self._i8_searches, self.prefilter_disabled = bool(adaptive), 0, False
        self.i8_max_queries = i8_max_queries
        self._norm_given = None if max_row_norm is None else float(max_row_norm)
        self._norm, self._norm_version = None, -1
        self._pipe = None                                  # search_many's streams / workspaces
        self._centre_query_given, self.centre_query, self.i8_mean_norm = centre_query, bool(centre_query), 0.0
        if prefilter == "int8" and self.n_rows > 0:
            self.build_int8()

    # ---- state derived from the rows (refreshed when the tensor was written to) -------------------------------------------
    def build_int8(self):
        """(Re)build the int8 pre-filter from the current fp16 rows.  `search` calls it by itself when the corpus tensor was written
        to since the last build (torch's version counter): int8 values of rows that no longer exist are not upper bounds of anything,
        and a certificate computed from them could certify a wrong answer."""
        need = self.lib.arx_topk_i8_index_bytes(self.n_rows, self.dim)
        if need < 0:
            raise _lib.ArxError(f"int8 pre-filter needs dim % 128 == 0 and dim <= 1024 (dim={self.dim})")
        if self._i8 is None or self._i8.numel() != need:
            self._i8 = torch.empty(need, dtype=torch.uint8, device=self.corpus.device)
        _lib.check(self.lib.arx_topk_build_i8(self.corpus.data_ptr(), self.n_rows, self.dim, self._i8.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "arx_topk_build_i8")
        self._i8_version = self.corpus._version
        info = (C.c_float * 3)()
        _lib.check(self.lib.arx_topk_i8_index_info(self._i8.data_ptr(), self.n_rows, self.dim, info, torch.cuda.current_stream().cuda_stream),
                   "arx_topk_i8_index_info")
        self.i8_mean_norm = float(info[0])
        self.centre_query = (self.i8_mean_norm ** 2 >= 0.25) if self._centre_query_given is None else bool(self._centre_query_given)

    def max_row_norm(self) -> float:
        """Upper bound on the L2 norm of the shard's rows (measured on the device unless the caller gave one)."""
        if self._norm_given is not None:
            return self._norm_given
        if self._norm is None or self._norm_version != self.corpus._version or self._norm_version < 0:
            out = torch.empty(1, dtype=torch.float32, device=self.corpus.device)
            _lib.check(self.lib.arx_rows_max_norm_f16(self.corpus.data_ptr(), self.n_rows, self.dim, out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "arx_rows_max_norm_f16")
            v = float(out.item())
            if not (v == v and v < float("inf")):
                raise _lib.ArxError("the shard holds a non-finite row (inf / NaN): top-k over it is undefined")
            # rows at most the unit bound keep the library's default tolerance (1 + 2^-9); an all-zero shard still needs a positive bound
            self._norm, self._norm_version = max(v, 1e-30), self.corpus._version
        return self._norm

    def _refresh(self):
        """Bring the int8 copy and the norm bound up to date with the rows ON THE CURRENT STREAM, before any search kernel that reads
        them is enqueued on any stream (search_many dispatches to side streams: ADVICE r3)."""
        if self.n_rows == 0:
            return
        self.max_row_norm()
        if self._i8 is not None and not self.prefilter_disabled and self.corpus._version != self._i8_version:
            self.build_int8()

    def invalidate(self):
        """Tell the index its rows were written BEHIND torch's back (through a raw pointer: the encoder kernels filling a slice of the shard
        via `device_f16_out`, another library): the tensor's version counter does not see such writes, so the int8 copy and the norm
        bound would silently describe rows that no longer exist.  The next search re-derives both.  (Writes through torch ops are noticed
        without this.)"""
        self._norm_version = -1
        self._i8_version = -1

    def _use_i8(self) -> bool:
        return self._i8 is not None and not self.prefilter_disabled and self.i8_max_queries != 0

    def _options(self, cu_limit: int = 0, flags: int = 0, **debug) -> "_lib.TopkOptionsC":
        o = _lib.TopkOptionsC()
        o.i8_max_queries = 0 if self.i8_max_queries is None else (-1 if self.i8_max_queries <= 0 else int(self.i8_max_queries))
        o.max_row_norm = self._norm_bound()
        o.cu_limit, o.flags = int(cu_limit), int(flags) | (_lib.TOPK_I8_CENTRE_QUERY if (self.centre_query and self._use_i8()) else 0)
        o.debug_tau_mult = float(debug.get("tau_mult", 0.0))
        o.debug_drop_best = int(debug.get("drop_best", 0))
        return o

    def workspace_bytes(self, nq: int, k: int) -> int:
        """Bytes of workspace THIS index's searches of nq queries need (the int8 pass needs the larger layout)."""
        fn = self.lib.arx_topk_workspace_bytes_i8 if self._use_i8() else self.lib.arx_topk_workspace_bytes
        need = fn(self.n_rows, nq, self.dim, k)
        if need < 0:
            raise _lib.ArxError(f"unsupported search shape n_rows={self.n_rows} nq={nq} dim={self.dim} k={k}")
        return int(need)

    def alloc_workspace(self, nq: int, k: int) -> torch.Tensor:
        return torch.empty(self.workspace_bytes(nq, k), dtype=torch.uint8, device=self.corpus.device)

    def _workspace(self, nq: int, k: int) -> torch.Tensor:
        need = self.workspace_bytes(nq, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.corpus.device)
        return self._ws

    def _norm_bound(self) -> float:
        """The rows' norm bound the searches pass to the library: never below the encoder's unit-row bound."""
        return max(self.max_row_norm(), 1.0 + 1.0 / 512.0)

    def _check_allow(self, allow: torch.Tensor):
        n_words = (self.n_rows + 63) // 64
        assert allow.is_cuda and allow.dtype in (torch.int64, torch.uint64) and allow.dim() == 1 and allow.is_contiguous()
        assert allow.shape[0] == n_words, f"allow has {allow.shape[0]} words, the shard's {self.n_rows} rows need {n_words}"

    def _masked_workspace(self, kind: str, need: int) -> torch.Tensor:
        """The index's cached workspace of the masked searches of `kind`, at least `need` bytes."""
        ws = self._ws_masked.get(kind)
        if ws is None or ws.numel() < need:
            ws = self._ws_masked[kind] = torch.empty(need, dtype=torch.uint8, device=self.corpus.device)
        return ws

    # ---- one batch ------------------------------------------------------------------------------------------------------
    def search(self, queries_f16: torch.Tensor, k: int = 10, ws: Optional[torch.Tensor] = None, out=None,
               _opt: Optional["_lib.TopkOptionsC"] = None, _stream: Optional[int] = None, allow: Optional[torch.Tensor] = None,
               n_allowed: Optional[int] = None, **debug) -> Tuple[torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D] (device) -> (scores f32 [Q, k], ids int64 [Q, k]); ids are global
        (local row + idx_base); score desc, ties -> lower id; (-inf, -1) pads when k > n_rows.
        `ws`: the device workspace this call uses (default: the index's own, which makes the index one-caller-at-a-time; callers that
        search one index from several host threads or streams pass their own, `alloc_workspace`).  `out = (scores, ids)` preallocated.
        `tau_mult` / `drop_best`: the certificate's test hooks, `flags`: ARX_TOPK_* (include/arx.h) — all per call; any other keyword is a
        TypeError (a misspelled hook would otherwise be dropped and leave the caller's test vacuous).
        `allow` (a device int64 / uint64 tensor of ceil(n_rows / 64) words, bit r & 63 of word r >> 6 = local row r may be returned; see
        `where.pack_bitmap`): the exact top-k of the ALLOWED rows only (`arx_topk_search_filtered`), ids still those of the original
        rows, (-inf, -1) pads when fewer than k rows are allowed.  `n_allowed`: the number of allowed rows if the caller knows it (the
        library then scores very selective filters row by row instead of scanning).  A filtered search always runs on the fp16 rows:
        the int8 pre-filter is not used for it.  Its test hooks are `path` (1 = masked scan, 2 = exhaustive) and `cand_cap`;
        `filtered_stats` reads its counters.  Without `allow` nothing changes."""
        if allow is not None:
            return self._search_filtered(queries_f16, k, allow, n_allowed, ws, out, _stream, debug)
        unknown = set(debug) - {"tau_mult", "drop_best", "flags"}
        if unknown:
            raise TypeError(f"ShardIndex.search() got unexpected keyword argument(s): {', '.join(sorted(unknown))}")
        q = queries_f16
        assert q.is_cuda and q.dtype == torch.float16 and q.dim() == 2 and q.shape[1] == self.dim and q.is_contiguous()
        nq = q.shape[0]
        if out is None:
            scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        else:
            scores, ids = out
            assert scores.shape == (nq, k) and ids.shape == (nq, k) and scores.is_contiguous() and ids.is_contiguous()
        if nq == 0:
            return scores, ids
        if self.n_rows == 0:
            scores.fill_(float("-inf")); ids.fill_(-1)
            return scores, ids
        if _opt is None:
            self._refresh()                                  # rows written since the int8 copy / norm bound were made (ShardSink.put, the encoder)
            _opt = self._options(flags=debug.pop("flags", 0), **debug)
        if ws is None:
            ws = self._workspace(nq, k)
        use_i8 = self._use_i8()
        st = torch.cuda.current_stream().cuda_stream if _stream is None else _stream
        rc = self.lib.arx_topk_search_opt(self.corpus.data_ptr(), self._i8.data_ptr() if use_i8 else None, self.n_rows, q.data_ptr(), nq,
                                          self.dim, k, scores.data_ptr(), ids.data_ptr(), self.idx_base, ws.data_ptr(), ws.numel(),
                                          C.byref(_opt), st)
        _lib.check(rc, "arx_topk_search_opt")
        self._last_ws = ws
        if _opt.flags & (_lib.TOPK_SCAN_ONLY | _lib.TOPK_TAIL_ONLY):
            return scores, ids
        # the counters describe the int8 pass only where it ran: a batch above the crossover took the fp16 pass, whose counters count
        # uncertified selections, not overflowing candidate lists (the library decides per call the same way, search.hip use_i8)
        ran_i8 = use_i8 and nq <= self._i8_nq_limit()
        if ran_i8 and self._adaptive and (self._i8_searches < 4 or self._i8_searches % 64 == 0):
            flagged, _ = self.certificate_stats()
            if flagged * 4 > nq:
                import sys
                print(f"[arx] int8 pre-filter switched off for this index: {flagged} of {nq} queries overflowed their candidate lists "
                      f"(rows on which the int8 bound is too slack); the fp16 pass answers from here on", file=sys.stderr)
                self.prefilter_disabled = True
        self._i8_searches += 1 if ran_i8 else 0
        return scores, ids

    def _scan_search(self, kind, entry, q, dims, outs, workspace_bytes, call, check_mask=None, path=0, cand_cap=0, ws=None, out=None,
                     _stream=None, refuse_empty=False):
        """What the searches of the scan driver share (csrc/masked_topk.h).  `kind`: the key of the cached workspace and the word in
        messages; `entry`: the C function behind `call`, for error texts; `dims`: the search's own sizes by name, in the order the C
        functions take them (k / max_results / n_groups, chunks_per_group); `outs`: per output tensor (its shape after [Q], dtype, pad);
        `workspace_bytes`: the library's arx_*_workspace_bytes; `check_mask(nq)` asserts the mask's tensors; `call(...)`: the library's
        *_tuned function with its leading arguments, up to the queries, bound.  `refuse_empty`: a shape the library does not support is an
        ArxError for an empty shard or query set too."""
        assert q.is_cuda and q.dtype == torch.float16 and q.dim() == 2 and q.shape[1] == self.dim and q.is_contiguous()
        nq = q.shape[0]
        if check_mask is not None:
            check_mask(nq)
        if out is None:
            out = tuple(torch.empty((nq, *shape), dtype=dtype, device=q.device) for shape, dtype, _ in outs)
        else:
            out = tuple(out)
            assert len(out) == len(outs) and all(t.shape == (nq, *shape) and t.is_contiguous() for t, (shape, _, _) in zip(out, outs))
        empty = nq == 0 or self.n_rows == 0
        if refuse_empty or not empty:
            need = workspace_bytes(max(self.n_rows, 1), max(nq, 1), self.dim, *dims.values())
            if need < 0:
                raise _lib.ArxError(f"unsupported {kind} search shape n_rows={self.n_rows} nq={nq} dim={self.dim} "
                                    + " ".join(f"{name}={v}" for name, v in dims.items()))
        if empty:
            for t, (_, _, pad) in zip(out, outs):
                t.fill_(pad)
            return out
        if ws is None:
            ws = self._masked_workspace(kind, need)
        st = torch.cuda.current_stream().cuda_stream if _stream is None else _stream
        rc = call(nq, self.dim, *dims.values(), *(t.data_ptr() for t in out), self.idx_base, self._norm_bound(), ws.data_ptr(), ws.numel(),
                  int(path), int(cand_cap), st)
        _lib.check(rc, entry)
        self._last_ws_masked[kind] = ws
        return out

    def _search_masked(self, kind, who, workspace_bytes, q, k, ws, out, _stream, debug, check_mask, call):
        """The three masked top-k searches.  `kind`: "filtered" / "prefix" / "filtered_multi"; `who`: the public spelling; the test hooks
        `path` and `cand_cap` arrive in `debug`, any other keyword is a TypeError."""
        unknown = set(debug) - {"path", "cand_cap"}
        if unknown:
            raise TypeError(f"ShardIndex.{who} got unexpected keyword argument(s): {', '.join(sorted(unknown))}")
        return self._scan_search(kind, f"arx_topk_search_{kind}", q, {"k": k}, (((k,), torch.float32, float("-inf")), ((k,), torch.int64, -1)),
                                 workspace_bytes, call, check_mask, ws=ws, out=out, _stream=_stream, **debug)

    def _masked_stats(self, kind, stats, ws):
        """`stats`: the library's arx_topk_<kind>_stats."""
        ws = self._last_ws_masked.get(kind) if ws is None else ws
        if ws is None:
            return (0, 0)
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(stats(ws.data_ptr(), C.byref(a), C.byref(b), torch.cuda.current_stream().cuda_stream), f"arx_topk_{kind}_stats")
        return (int(a.value), int(b.value))

    def _search_filtered(self, q, k, allow, n_allowed, ws, out, _stream, debug):
        def call(*rest):
            return self.lib.arx_topk_search_filtered_tuned(self.corpus.data_ptr(), self.n_rows, allow.data_ptr(),
                                                           -1 if n_allowed is None else int(n_allowed), q.data_ptr(), *rest)
        return self._search_masked("filtered", "search(allow=...)", self.lib.arx_topk_filtered_workspace_bytes, q, k, ws, out, _stream, debug,
                                   lambda nq: self._check_allow(allow), call)

    def filtered_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search(allow=...)` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("filtered", self.lib.arx_topk_filtered_stats, ws)

    # ---- a different filter per query in one call -------------------------------------------------------------------------
    def search_filtered_many(self, queries_f16: torch.Tensor, allows: torch.Tensor, filter_of: torch.Tensor, k: int = 10, n_allowed=None,
                             ws: Optional[torch.Tensor] = None, out=None, **debug) -> Tuple[torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D], `allows` int64 / uint64 [F, ceil(n_rows / 64)] (F <= 64 bitmaps in the convention of `search(allow=...)`)
        and `filter_of` int32 [Q], all on the device -> (scores f32 [Q, k], ids int64 [Q, k]): for query q the exact top-k of the rows
        `allows[filter_of[q]]` allows (`arx_topk_search_filtered_multi`), bit for bit what `search(q, allow=allows[filter_of[q]])` returns
        for that query alone, with the shard read once for the whole batch instead of once per filter.  A `filter_of[q]` outside [0, F)
        means the query sees no row: all (-inf, -1).  `n_allowed`: a sequence of F counts of allowed rows (None or -1 = unknown) if the
        caller knows them.  Runs on the fp16 rows.  Test hooks as for `search(allow=...)`: `path` and `cand_cap`;
        `filtered_many_stats` reads the counters."""
        q = queries_f16
        if not (torch.is_tensor(allows) and allows.dim() == 2):
            raise ValueError("allows must be a 2-d device tensor [F, ceil(n_rows / 64)]")
        n_filters, n_words = int(allows.shape[0]), (self.n_rows + 63) // 64
        if not (1 <= n_filters <= 64):
            raise ValueError(f"allows holds {n_filters} filters: one call takes 1..64")
        if n_allowed is not None:
            counts = [-1 if c is None else int(c) for c in n_allowed]
            if len(counts) != n_filters:
                raise ValueError(f"n_allowed has {len(counts)} entries for {n_filters} filters")
            n_allowed_c = (C.c_int64 * n_filters)(*counts)
        else:
            n_allowed_c = None

        def check_mask(nq):
            assert allows.is_cuda and allows.dtype in (torch.int64, torch.uint64) and allows.is_contiguous()
            assert allows.shape[1] == n_words, f"allows has {allows.shape[1]} words per filter, the shard's {self.n_rows} rows need {n_words}"
            assert filter_of.is_cuda and filter_of.dtype == torch.int32 and filter_of.shape == (nq,) and filter_of.is_contiguous()

        def workspace_bytes(n_rows, nq, dim, kk):
            return self.lib.arx_topk_filtered_multi_workspace_bytes(n_rows, nq, n_filters, dim, kk)

        def call(*rest):
            return self.lib.arx_topk_search_filtered_multi_tuned(self.corpus.data_ptr(), self.n_rows, allows.data_ptr(), n_filters, n_allowed_c,
                                                                 filter_of.data_ptr(), q.data_ptr(), *rest)
        return self._search_masked("filtered_multi", "search_filtered_many()", workspace_bytes, q, k, ws, out, None, debug, check_mask, call)

    def filtered_many_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search_filtered_many` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("filtered_multi", self.lib.arx_topk_filtered_multi_stats, ws)

    # ---- a row limit per query (near-duplicate detection) -----------------------------------------------------------------
    def search_prefix(self, queries_f16: torch.Tensor, row_limit: torch.Tensor, k: int = 10, ws: Optional[torch.Tensor] = None,
                      **debug) -> Tuple[torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D] and `row_limit` int64 [Q] (both on the device) -> (scores f32 [Q, k], ids int64 [Q, k]): for query q the exact
        top-k of the LOCAL rows r < row_limit[q] (`arx_topk_search_prefix`; the limit is clamped to [0, n_rows]), score desc, ties -> lower
        row, ids = local row + idx_base, (-inf, -1) pads when fewer than k rows lie below the limit.  A (query, row) score has the bits
        `search` gives it.  `queries_f16` may be a view of the shard's own rows.  Runs on the fp16 rows (no int8 pre-filter).  Test hooks
        as for `search(allow=...)`: `path` (1 = masked scan, 2 = exhaustive) and `cand_cap`; `prefix_stats` reads the counters."""
        q = queries_f16

        def check_mask(nq):
            assert row_limit.is_cuda and row_limit.dtype == torch.int64 and row_limit.shape == (nq,) and row_limit.is_contiguous()

        def call(*rest):
            return self.lib.arx_topk_search_prefix_tuned(self.corpus.data_ptr(), self.n_rows, q.data_ptr(), row_limit.data_ptr(), *rest)
        return self._search_masked("prefix", "search_prefix()", self.lib.arx_topk_prefix_workspace_bytes, q, k, ws, None, None, debug,
                                   check_mask, call)

    def prefix_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search_prefix` / `nearest_earlier` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("prefix", self.lib.arx_topk_prefix_stats, ws)

    def nearest_earlier(self, row_lo: int = 0, row_hi: Optional[int] = None, k: int = 1, **debug) -> Tuple[torch.Tensor, torch.Tensor]:
        """The self-join: for every local row r in [row_lo, row_hi) the exact top-k of the rows BEFORE it (local rows < r) ->
        (scores f32 [m, k], ids int64 [m, k]) on the device, m = row_hi - row_lo; row 0 has no earlier row: (-inf, -1).  The queries are a
        view of the shard (no copy).  A row's answer does not depend on the range it was asked in."""
        row_hi = self.n_rows if row_hi is None else int(row_hi)
        row_lo = int(row_lo)
        if not (0 <= row_lo <= row_hi <= self.n_rows):
            raise ValueError(f"rows [{row_lo}, {row_hi}) are not a range of the shard's {self.n_rows} rows")
        limit = torch.arange(row_lo, row_hi, dtype=torch.int64, device=self.corpus.device)
        return self.search_prefix(self.corpus[row_lo:row_hi], limit, k, **debug)

    # ---- grouped search: the top papers with their best chunks --------------------------------------------------------------
    def set_groups(self, group_of) -> "ShardIndex":
        """`group_of`: int32 [n_rows] (a tensor, on the host or the device, or anything numpy converts), the group (the paper) of every
        local row: non-decreasing, non-negative, not necessarily dense, so that a group is a contiguous run of rows.  Uploads it and
        measures its runs once (`arx_group_runs_info`): ValueError when it decreases somewhere or holds a negative value; the longest
        run is cached as `max_run_rows`, the number of runs as `n_runs`.  `search_grouped` needs it."""
        g = group_of if torch.is_tensor(group_of) else torch.as_tensor(group_of)
        if g.dim() != 1 or g.shape[0] != self.n_rows:
            raise ValueError(f"group_of has shape {tuple(g.shape)}, the shard's {self.n_rows} rows need ({self.n_rows},)")
        if g.dtype.is_floating_point or g.dtype == torch.bool:
            raise ValueError(f"group_of must hold integers, got {g.dtype}")
        if g.numel() and g.dtype != torch.int32 and (int(g.max()) > 2 ** 31 - 1 or int(g.min()) < -2 ** 31):
            raise ValueError("group_of holds a value outside int32")
        g = g.to(device=self.corpus.device, dtype=torch.int32).contiguous()
        info = torch.zeros(2, dtype=torch.int64, device=self.corpus.device)
        if self.n_rows:
            _lib.check(self.lib.arx_group_runs_info(g.data_ptr(), self.n_rows, info.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "arx_group_runs_info")
        longest, runs = (int(v) for v in info.tolist())
        if longest < 0:
            raise ValueError("group_of must be non-decreasing and non-negative: a group is a contiguous run of rows")
        self.group_of, self.max_run_rows, self.n_runs = g, max(longest, 1), runs
        return self

    def search_grouped(self, queries_f16: torch.Tensor, n_groups: int, chunks_per_group: int = 1, allow: Optional[torch.Tensor] = None,
                       n_allowed: Optional[int] = None, path: int = 0, cand_cap: int = 0, ws: Optional[torch.Tensor] = None,
                       max_run_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D] (device) -> (scores f32 [Q, P, m], ids int64 [Q, P, m], groups int32 [Q, P]) on the device, P = `n_groups`
        <= 32, m = `chunks_per_group` <= 8 (`arx_topk_search_grouped`; `set_groups` first).  A group's score is the best score of its
        visible rows; the P best groups come by (score desc, row of the best chunk asc), each with its m best visible chunks by (score
        desc, row asc); ids = local row + idx_base, `groups` = the `group_of` value; (-inf, -1) and -1 pad.  A (query, row) score has the
        bits `search` gives it.  `allow` / `n_allowed` as for `search(allow=...)`, None = every row.  Runs on the fp16 rows.  Test hooks:
        `path` (1 = scan, 2 = exhaustive), `cand_cap`, and `max_run_rows` (default: the measured one; a smaller one voids exactness);
        `grouped_stats` reads the counters."""
        if getattr(self, "group_of", None) is None:
            raise ValueError("search_grouped needs set_groups(group_of) first")
        q, P, m = queries_f16, int(n_groups), int(chunks_per_group)

        def call(*rest):
            return self.lib.arx_topk_search_grouped_tuned(self.corpus.data_ptr(), self.n_rows, self.group_of.data_ptr(),
                                                          int(self.max_run_rows if max_run_rows is None else max_run_rows),
                                                          None if allow is None else allow.data_ptr(), -1 if n_allowed is None else int(n_allowed),
                                                          q.data_ptr(), *rest)
        outs = (((P, m), torch.float32, float("-inf")), ((P, m), torch.int64, -1), ((P,), torch.int32, -1))
        return self._scan_search("grouped", "arx_topk_search_grouped", q, {"n_groups": P, "chunks_per_group": m}, outs,
                                 self.lib.arx_topk_grouped_workspace_bytes, call, lambda nq: allow is None or self._check_allow(allow),
                                 path, cand_cap, ws, refuse_empty=True)

    def grouped_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search_grouped` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("grouped", self.lib.arx_topk_grouped_stats, ws)

    # ---- boosted search: cosine plus a weighted row prior ---------------------------------------------------------------------
    def prior_info(self, prior: torch.Tensor) -> Tuple[float, int]:
        """(the largest |finite value|, the number of non-finite values) of a device f32 tensor, in one pass (`arx_prior_info`).
        Synchronises on the current stream."""
        assert prior.is_cuda and prior.dtype == torch.float32 and prior.dim() == 1 and prior.is_contiguous()
        info = torch.zeros(2, dtype=torch.int64, device=prior.device)
        if prior.numel():
            _lib.check(self.lib.arx_prior_info(prior.data_ptr(), prior.numel(), info.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "arx_prior_info")
        bits, bad = (int(v) for v in info.tolist())
        return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0], bad

    def search_boosted(self, queries_f16: torch.Tensor, k: int, prior: torch.Tensor, weight, allow: Optional[torch.Tensor] = None,
                       n_allowed: Optional[int] = None, ws: Optional[torch.Tensor] = None, max_abs_prior: Optional[float] = None,
                       **debug) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D] (device), `prior` f32 [n_rows] (device), `weight` a number or one per query ->
        (scores f32 [Q, k], base f32 [Q, k], ids int64 [Q, k]) on the device (`arx_topk_search_boosted`): the k <= 32
        best visible rows by (boosted desc, row asc), boosted = float32(base + float32(weight[q] * prior[r])), `base` the bits `search`
        gives the pair; (-inf, -inf, -1) pads.  A row with a NaN or +-inf prior is hidden from every query.  `allow` / `n_allowed` as
        for `search(allow=...)`, None = every row.  Runs on the fp16 rows.
        `weight` on the host (a number, a sequence, a numpy array, a host tensor): one that is not finite, or whose product with the
        largest |prior| is not, is a ValueError (`boost.check_args`), and the checked values are uploaded, which waits for the copy.
        `weight` as a contiguous device float32 tensor [Q] is taken as it is, with no copy and no wait: the device's rule holds (a
        non-finite weight gives its query no rows).
        `max_abs_prior`: the largest |finite prior|.  Given (`HipCollection.set_boost` measures it once), the call is stream-ordered
        with a device weight.  None: `prior_info` measures it, which synchronises, once per prior tensor and version of it (the result
        is kept beside the tensor's address; a prior written behind torch's back needs the argument).
        Test hooks: `path` (1 = scan, 2 = exhaustive) and `cand_cap`; `boosted_stats` reads the counters."""
        from . import boost as _boost
        unknown = set(debug) - {"path", "cand_cap"}
        if unknown:
            raise TypeError(f"ShardIndex.search_boosted() got unexpected keyword argument(s): {', '.join(sorted(unknown))}")
        q = queries_f16
        if not (torch.is_tensor(prior) and prior.is_cuda and prior.dtype == torch.float32 and prior.shape == (self.n_rows,) and prior.is_contiguous()):
            raise ValueError(f"prior must be a contiguous device float32 tensor of shape ({self.n_rows},)")
        if max_abs_prior is None:
            key = (prior.data_ptr(), prior.numel(), prior._version)
            if getattr(self, "_prior_info_key", None) != key:
                self._prior_info_key, self._prior_info_max = key, self.prior_info(prior)[0]
            max_abs_prior = self._prior_info_max
        nq = int(q.shape[0])
        if torch.is_tensor(weight) and weight.is_cuda:
            if not (weight.dtype == torch.float32 and weight.shape == (nq,) and weight.is_contiguous()):
                raise ValueError(f"a device boost weight must be a contiguous float32 tensor of shape ({nq},)")
            _boost.check_args(k, 0.0, nq, max_abs_prior, self.dim)
            wd = weight
        else:
            wd = torch.from_numpy(_boost.check_args(k, weight, nq, max_abs_prior, self.dim)).to(q.device)

        def call(*rest):
            return self.lib.arx_topk_search_boosted(self.corpus.data_ptr(), self.n_rows, prior.data_ptr(), float(max_abs_prior), wd.data_ptr(),
                                                    None if allow is None else allow.data_ptr(), -1 if n_allowed is None else int(n_allowed),
                                                    q.data_ptr(), *rest)
        ninf = float("-inf")
        outs = (((k,), torch.float32, ninf), ((k,), torch.float32, ninf), ((k,), torch.int64, -1))
        return self._scan_search("boosted", "arx_topk_search_boosted", q, {"k": k}, outs, self.lib.arx_topk_search_boosted_workspace_bytes, call,
                                 lambda nq: allow is None or self._check_allow(allow), ws=ws, **debug)

    def boosted_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search_boosted` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("boosted", self.lib.arx_topk_boosted_stats, ws)

    # ---- score threshold: every row at or above a cosine, up to 1 024 per query ---------------------------------------------
    def search_range(self, queries_f16: torch.Tensor, min_score, max_results: int, allow: Optional[torch.Tensor] = None, n_allowed: int = -1,
                     ws: Optional[torch.Tensor] = None, path: int = 0, cand_cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """queries fp16 [Q, D] (device) -> (scores f32 [Q, M], ids int64 [Q, M], counts int32 [Q]) on the device, M = `max_results` in
        1..1024 (`arx_range_search`).  `min_score`: a float, or one per query (a tensor on the host or the device, or anything numpy
        converts).  A visible row qualifies when its score is >= the query's threshold, compared in f32 (-inf: every visible row; +inf or
        NaN: none); the best min(count, M) qualifying rows come by (score desc, row asc), ids = local row + idx_base, (-inf, -1) pads.
        `counts[q]` is the number of qualifying rows when that is <= M and exactly M + 1 when more qualify: the list then holds the best
        M (an exact total above M is not offered: it would cost a full exact scan).  A (query, row) score has the bits `search` gives
        it.  `allow` / `n_allowed` as for `search(allow=...)`, None = every row.  Runs on the fp16 rows: the int8 index plays no part.
        Test hooks: `path` (1 = scan, 2 = exhaustive) and `cand_cap`; `range_stats` reads the counters."""
        q, M = queries_f16, int(max_results)
        ms = device_thresholds(min_score, q.shape[0], q.device)

        def call(*rest):
            return self.lib.arx_range_search_tuned(self.corpus.data_ptr(), self.n_rows, None if allow is None else allow.data_ptr(),
                                                   -1 if n_allowed is None else int(n_allowed), q.data_ptr(), ms.data_ptr(), *rest)
        outs = (((M,), torch.float32, float("-inf")), ((M,), torch.int64, -1), ((), torch.int32, 0))
        return self._scan_search("range", "arx_range_search", q, {"max_results": M}, outs, self.lib.arx_range_workspace_bytes, call,
                                 lambda nq: allow is None or self._check_allow(allow), path, cand_cap, ws, refuse_empty=True)

    def range_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose candidate list overflowed and were answered by the exhaustive path, candidate groups rescored) of the LAST
        `search_range` on this index (or on `ws`).  Synchronises on the current stream."""
        return self._masked_stats("range", self.lib.arx_range_stats, ws)

    def _i8_nq_limit(self) -> int:
        """The largest query batch the int8 pass takes under this index's policy (`i8_max_queries`; None = the library default, 1 024)."""
        if self.i8_max_queries is None:
            return 1024
        return max(0, min(int(self.i8_max_queries), 1024))

    def certificate_stats(self, ws: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """(queries whose first selection could not be certified, extra 64-row groups rescored for them) of the LAST `search`
        on this index (or on `ws`): the answer is exact either way (csrc/search_tail.h, rescore_kernel step 5); the counters say how often
        the slow path ran.  Where the int8 pre-filter ran the pair is (queries whose OWN candidate lists overflowed and went to the
        exhaustive kernel, (query, group) candidates the pre-filter's bounds let through) instead.
        Synchronises on the current stream."""
        ws = self._last_ws if ws is None else ws
        if ws is None:
            return (0, 0)
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.arx_topk_stats(ws.data_ptr(), C.byref(a), C.byref(b), torch.cuda.current_stream().cuda_stream),
                   "arx_topk_stats")
        return (int(a.value), int(b.value))

    # ---- a stream of batches --------------------------------------------------------------------------------------------
    def _pipeline(self, tail_cus: int, lanes: int):
        """`lanes` (scan, tail) stream pairs for `tail_cus` (process-wide per device, see `_cu_streams`) + one workspace per lane."""
        if self._pipe is None or (self._pipe["tail_cus"], len(self._pipe["lanes"])) != (tail_cus, lanes):
            self._pipe = {"tail_cus": tail_cus, "lanes": [_cu_streams(self.corpus.device, tail_cus, ln) for ln in range(lanes)],
                          "ws": [None] * lanes, "xchg": torch.cuda.Stream(self.corpus.device)}
        return self._pipe

    def search_many(self, batches, k: int = 10, distributed: bool = False, group=None, tail_cus: int = 0, lanes: int = 2):
        """A STREAM of query batches (each <= 1 024 queries), pipelined over `lanes` pairs of HIP streams: a lane's `scan` stream (pass A:
        HBM-bound) and its `tail` stream (select / exact rescoring / certificate), batch b on lane b % lanes, one workspace per lane.
        While one lane is in its tail — or in the few microseconds of dependent-launch latency between its kernels — the other lane's
        scan has the memory system to itself (SURVEY.md §8e "Overlap": on a 625 k-row shard the tail and the exchange are as long as the
        pass itself).  Under a process group batch b's all-gather of the [Q, k] partials and the merge run on a third, ordinary stream.
        `tail_cus` > 0 gives the two streams of a lane DISJOINT compute-unit masks (scan on all but `tail_cus` CUs, tail on the rest:
        `arx_stream_create_cu_mask`), so that the tail's blocks never wait for scan blocks to drain.  Measured on the 625 k x 768 shard
        (profiles/r04/search_many_lanes_cu_split.md): it LOSES — 0.191 ms per 64-query batch with plain streams, 0.22-0.28 with 16-64
        tail CUs: once the tail reads one row per selected group (round 4) it is short enough that taking CUs from the scan costs more
        than the waiting did — hence the default 0.
        The caller's stream waits for every stream before this returns.  Same results, bit for bit, as `search` /
        `search_distributed` batch by batch."""
        import torch.distributed as dist
        batches = list(batches)
        if not batches:
            return []
        dev = self.corpus.device
        cur = torch.cuda.current_stream(dev)
        if self.n_rows == 0 or any(q.shape[0] > 1024 or q.shape[0] == 0 for q in batches):
            return [self.search_distributed(q, k, group) if distributed else self.search(q, k) for q in batches]
        self._refresh()                                      # on the caller's stream, BEFORE any lane may read the int8 copy / norm bound
        lanes = max(1, min(int(lanes), len(batches)))
        pipe = self._pipeline(tail_cus, lanes)
        need = max(self.workspace_bytes(nq_b, k) for nq_b in {q.shape[0] for q in batches})      # (not monotonic in the batch size: small batches carry aux words)
        for j in range(lanes):
            if pipe["ws"][j] is None or pipe["ws"][j].numel() < need:
                pipe["ws"][j] = torch.empty(need, dtype=torch.uint8, device=dev)
        scan_cus = pipe["lanes"][0][2]
        o_scan = self._options(cu_limit=scan_cus, flags=_lib.TOPK_SCAN_ONLY)
        o_tail = self._options(cu_limit=tail_cus, flags=_lib.TOPK_TAIL_ONLY)
        xchg = pipe["xchg"]
        nb = len(batches)
        # every buffer the side streams touch is allocated HERE, on the caller's stream (nothing is allocated under, or recorded on, the
        # CU-masked streams: they are not torch's, and the caching allocator must never be asked to order a free against them)
        all_s = [torch.empty((q.shape[0], k), dtype=torch.float32, device=dev) for q in batches]
        all_i = [torch.empty((q.shape[0], k), dtype=torch.int64, device=dev) for q in batches]
        ready = torch.cuda.Event(); ready.record(cur)
        for scan, tail, _ in pipe["lanes"]:
            scan.wait_event(ready); tail.wait_event(ready)
        scanned = [torch.cuda.Event() for _ in range(nb)]
        tailed = [torch.cuda.Event() for _ in range(nb)]
        out = []
        do_dist = distributed and dist.is_initialized()
        if do_dist:
            xchg.wait_event(ready)
        for b, q in enumerate(batches):
            scan, tail, _ = pipe["lanes"][b % lanes]
            ws = pipe["ws"][b % lanes]
            if b >= lanes:
                scan.wait_event(tailed[b - lanes])           # the lane's workspace has been read out
            self.search(q, k, ws=ws, out=(all_s[b], all_i[b]), _opt=o_scan, _stream=scan.cuda_stream)
            scanned[b].record(scan)
            tail.wait_event(scanned[b])
            s, i = self.search(q, k, ws=ws, out=(all_s[b], all_i[b]), _opt=o_tail, _stream=tail.cuda_stream)
            tailed[b].record(tail)
            if do_dist:                                      # the exchange on an ordinary torch stream (RCCL's own kernels take any CU)
                xchg.wait_event(tailed[b])
                with torch.cuda.stream(xchg):
                    s, i = merge_partials(*gather_partials(s, i, group), k)
                    s.record_stream(cur); i.record_stream(cur)
            out.append((s, i))
        for scan, tail, _ in pipe["lanes"]:
            cur.wait_stream(scan); cur.wait_stream(tail)
        if do_dist:
            cur.wait_stream(xchg)
        self._last_ws = pipe["ws"][(nb - 1) % lanes]
        return out

    def search_distributed(self, queries_f16: torch.Tensor, k: int = 10, group=None, allow: Optional[torch.Tensor] = None,
                           n_allowed=None, allows: Optional[torch.Tensor] = None, filter_of: Optional[torch.Tensor] = None):
        """Every rank passes the SAME queries; returns the global top-k on every rank.  `allow` / `n_allowed` (see `search`): each rank
        filters its OWN shard with its own bitmap; the gather and the merge are the same.  `allows` + `filter_of` (see
        `search_filtered_many`; `n_allowed` is then its sequence of counts): a filter per query, again each rank's own bitmaps."""
        import torch.distributed as dist
        if (allows is None) != (filter_of is None):
            raise ValueError("allows and filter_of go together")
        if allows is not None:
            if allow is not None:
                raise ValueError("pass allow (one filter for the call) or allows + filter_of (one per query), not both")
            s, i = self.search_filtered_many(queries_f16, allows, filter_of, k, n_allowed=n_allowed)
        else:
            s, i = self.search(queries_f16, k, allow=allow, n_allowed=n_allowed)
        if not dist.is_initialized():
            return s, i
        # world size 1 takes the same gather + merge path (a 1-part merge is the identity): one code path to test
        all_s, all_i = gather_partials(s, i, group)
        return merge_partials(all_s, all_i, k)


def search_filtered_grouped(index: ShardIndex, queries_f16: torch.Tensor, k: int, bitmaps, filter_of, counts=None, group=None):
    """`ShardIndex.search_filtered_many` (through `search_distributed`) for ANY number of distinct filters: `bitmaps` is a list of device
    int64 [ceil(n_rows / 64)] tensors (or one contiguous [F, ceil(n_rows / 64)] tensor, whose rows a call then reads in place),
    `filter_of` a host sequence with the index of every query's bitmap, `counts` the bitmaps' allowed rows (or None).  The batch is cut into calls of at most 64 distinct filters (`filter_sets.filter_groups`) and the rows are put back
    in query order -> (scores [Q, k], ids [Q, k]) as one call would return them."""
    from .filter_sets import filter_groups
    q = queries_f16
    dev = q.device
    groups = filter_groups(filter_of)
    scores = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev)
    ids = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev)
    for positions, filters, local_of in groups:
        if torch.is_tensor(bitmaps) and filters == list(range(filters[0], filters[-1] + 1)):
            allows = bitmaps[filters[0]:filters[-1] + 1]
        else:
            allows = torch.stack([bitmaps[f] for f in filters]).contiguous()
        fo = torch.tensor(local_of, dtype=torch.int32, device=dev)
        n_allowed = None if counts is None else [counts[f] for f in filters]
        if len(groups) == 1:                                   # the whole batch, already in order
            return index.search_distributed(q, k, group, n_allowed=n_allowed, allows=allows, filter_of=fo)
        pos = torch.tensor(positions, dtype=torch.int64, device=dev)
        s, i = index.search_distributed(q[pos].contiguous(), k, group, n_allowed=n_allowed, allows=allows, filter_of=fo)
        scores[pos], ids[pos] = s, i
    return scores, ids


_CU_STREAMS = {}


def _cu_streams(device, tail_cus: int, lane: int = 0):
    """(scan stream, tail stream, CUs of the scan stream) for one device: two HIP streams with DISJOINT compute-unit masks
    (`arx_stream_create_cu_mask`) — `scan` on all but `tail_cus` CUs, `tail` on the rest; tail_cus a multiple of 8 (the driver deals mask
    bits round-robin to the 8 XCDs — measured: bits [224, 256) are 4 CUs on each XCD — so both streams keep CUs on every XCD).
    tail_cus = 0: two ordinary torch streams, the whole chip each.  Created once per (device, split) and kept for the life of the
    process: a HIP stream that torch has seen must not be destroyed while tensors or events may still refer to it."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(tail_cus), int(lane))
    if key in _CU_STREAMS:
        return _CU_STREAMS[key]
    lib = _lib.load()
    if tail_cus <= 0:
        val = (torch.cuda.Stream(device), torch.cuda.Stream(device), 0)
    else:
        with torch.cuda.device(device):
            n_cu = lib.arx_device_cu_count()
            assert tail_cus % 8 == 0 and tail_cus < n_cu, f"tail_cus={tail_cus} must be a multiple of 8 below {n_cu}"
            words = (n_cu + 31) // 32

            def stream_of(lo, hi):
                m = (C.c_uint32 * words)()
                for b in range(lo, hi):
                    m[b // 32] |= 1 << (b % 32)
                h = C.c_void_p(None)
                _lib.check(lib.arx_stream_create_cu_mask(m, words, C.byref(h)), "arx_stream_create_cu_mask")
                return torch.cuda.ExternalStream(h.value, device=device)
            val = (stream_of(0, n_cu - tail_cus), stream_of(n_cu - tail_cus, n_cu), n_cu - tail_cus)
    _CU_STREAMS[key] = val
    return val


def gather_partials(s: torch.Tensor, i: torch.Tensor, group=None):
    """The path's only exchange step: every rank contributes its [Q, k] partial (scores, global ids);
    returns the stacked [P, Q, k] tensors on every rank (RCCL on GPU tensors, gloo on CPU tensors)."""
    import torch.distributed as dist
    P = dist.get_world_size(group)
    all_s = torch.empty((P,) + tuple(s.shape), dtype=s.dtype, device=s.device)
    all_i = torch.empty((P,) + tuple(i.shape), dtype=i.dtype, device=i.device)
    if s.is_cuda:
        dist.all_gather_into_tensor(all_s, s.contiguous(), group=group)
        dist.all_gather_into_tensor(all_i, i.contiguous(), group=group)
    else:                                   # gloo: list form
        ls = [torch.empty_like(s) for _ in range(P)]; li = [torch.empty_like(i) for _ in range(P)]
        dist.all_gather(ls, s.contiguous(), group=group); dist.all_gather(li, i.contiguous(), group=group)
        all_s = torch.stack(ls); all_i = torch.stack(li)
    return all_s, all_i


def merge_partials(all_scores: torch.Tensor, all_ids: torch.Tensor, k: int):
    """[P, Q, k] partial lists (device) -> merged [Q, k] via the HIP merge kernel."""
    lib = _lib.load()
    P, nq, kk = all_scores.shape
    assert kk == k and all_scores.is_contiguous() and all_ids.is_contiguous()
    out_s = torch.empty((nq, k), dtype=torch.float32, device=all_scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=all_scores.device)
    rc = lib.arx_topk_merge(all_scores.data_ptr(), all_ids.data_ptr(), P, nq, k, out_s.data_ptr(), out_i.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "arx_topk_merge")
    return out_s, out_i


def shard_bounds(n_total: int, world: int, rank: int) -> Tuple[int, int]:
    """rows [r*ceil(N/P), min(N, (r+1)*ceil(N/P)))  (SURVEY.md §8e)."""
    per = (n_total + world - 1) // world
    lo = min(n_total, rank * per)
    return lo, min(n_total, lo + per)


def fill_unit_rows(n_rows: int, dim: int, seed: int, device="cuda:0", row_base: int = 0) -> torch.Tensor:
    """Synthetic corpus/queries generated directly in HBM (bench cfg 3).  `row_base`: this tensor is rows [row_base, row_base + n_rows)
    of the corpus the seed defines — every rank of a sharded run fills its own slice of ONE corpus (bench cfg 4)."""
    lib = _lib.load()
    t = torch.empty((n_rows, dim), dtype=torch.float16, device=device)
    if n_rows > 0:
        _lib.check(lib.arx_fill_unit_rows_f16_at(t.data_ptr(), n_rows, dim, seed, row_base, torch.cuda.current_stream(t.device).cuda_stream),
                   "arx_fill_unit_rows_f16_at")
    return t


def fill_clustered_rows(n_rows: int, dim: int, seed: int, n_clusters: int, device="cuda:0", row_base: int = 0, spread: float = 0.35,
                        hot_dims: int = 3, hot_gain: float = 6.0) -> torch.Tensor:
    """Embedding-LIKE synthetic rows generated in HBM (`arx_fill_clustered_rows_f16_at`): tight clusters around `n_clusters` centres and a
    few hot dimensions — what the iid Gaussian rows of `fill_unit_rows` are not: a query's neighbours score within the int8 bound's
    slack of each other, and max|x| (the int8 scale) is set by the hot dimensions.  Queries: same seed, a `row_base` beyond the corpus
    (scattered clusters) or inside it (topic order).  `n_clusters < 0`: TOPIC ORDER, consecutive runs of `-n_clusters` rows share a centre."""
    lib = _lib.load()
    t = torch.empty((n_rows, dim), dtype=torch.float16, device=device)
    if n_rows > 0:
        _lib.check(lib.arx_fill_clustered_rows_f16_at(t.data_ptr(), n_rows, dim, seed, row_base, n_clusters, spread, hot_dims, hot_gain,
                                                      torch.cuda.current_stream(t.device).cuda_stream), "arx_fill_clustered_rows_f16_at")
    return t
