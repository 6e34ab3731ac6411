"""What the two candidate-scan indexes share (`binary.BinaryIndex`, `pq.PqIndex`): a code array with one entry per row of a
`ShardIndex`, a scan over it that names every query's `n_candidates` best rows, and the exact rescore of those lists.

`CodeIndex` keeps the codes beside the rows (`append`, `compact`; `rows_added` and `rows_compacted` to a collection), owns the two
cached workspaces and is the one `search`: check, `candidates`, `rescore_candidates`.  A subclass says how rows become codes (`encode_rows`), how queries become the scan's input
and which entry point scans (`candidates`), and how large that scan's workspace is (`_scan_bytes`).  `rescore_candidates` hands the
lists to `arx_ivf_search` as inverted lists (`ivf._launch`), so every score has the bits of `ShardIndex.search`; `rescore_host` restates
it with numpy (for the tests).  `launch` is the one launch path of both modules' own entry points.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

MAX_CANDIDATES, MAX_K = 256, 32
RESCORE_QUERIES = 1024          # queries per `arx_ivf_search` call of a rescore (one list per query, n_lists <= 4096)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_candidate_args(k, n_candidates) -> None:
    """The refusals about `n_candidates` and k (None: a scan without a rescore), each a ValueError before anything is launched."""
    if not _is_int(n_candidates) or not (1 <= n_candidates <= MAX_CANDIDATES):
        raise ValueError(f"n_candidates={n_candidates!r} must be an integer in [1, {MAX_CANDIDATES}]")
    if k is not None:
        if not _is_int(k) or not (1 <= k <= MAX_K):
            raise ValueError(f"k={k!r} must be an integer in [1, {MAX_K}] (the search's k limit)")
        if n_candidates < k:
            raise ValueError(f"n_candidates={n_candidates} is below k={k}: the rescore picks its k rows among the candidates")


def check_centre(centre, dim: int):
    """`centre` as a `build` takes it -> "mean", None or a float32 array [dim]; anything else is a ValueError."""
    if centre is None or (isinstance(centre, str) and centre == "mean"):
        return centre
    if isinstance(centre, str):
        raise ValueError(f"centre={centre!r} must be \"mean\", None or a float32 array [dim]")
    c = np.asarray(centre.detach().cpu().numpy() if hasattr(centre, "detach") else centre)
    if c.shape != (dim,) or c.dtype.kind != "f":
        raise ValueError(f"centre must be \"mean\", None or a float array of shape ({dim},), not {c.dtype} {tuple(c.shape)}")
    return np.ascontiguousarray(c, dtype=np.float32)


def launch(name: str, device, *args):
    """The one launch path: entry point `name` with `args` and the current stream of `device` behind them; a refusal is an
    `ArxError` naming the field."""
    import torch
    from . import _lib
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream(device).cuda_stream), name)


def rescore_host(X, Q, cand, count, k: int):
    """(scores f32 [nq, k], ids int64 [nq, k], count): the best k of the first `count[q]` rows of every list `cand[q]` by
    (`topics.exact_scores_host` desc, row asc), `lexsort`ed; what `rescore_candidates` returns with idx_base = 0, bit for bit."""
    from .topics import exact_scores_host
    X, Q = np.asarray(X), np.asarray(Q)
    nq = Q.shape[0]
    scores, ids = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        rows = cand[q, :count[q]].astype(np.int64)
        if rows.shape[0] == 0:
            continue
        sc = exact_scores_host(X[rows], Q[q:q + 1])[:, 0].astype(np.float32, copy=False)
        best = np.lexsort((rows, -sc))[:k]
        scores[q, :best.shape[0]], ids[q, :best.shape[0]] = sc[best], rows[best]
    return scores, ids, count


def rescore_candidates(index, q16, cand, count, k: int, cache):
    """(scores f32 [nq, k], ids int64 [nq, k], count) on the device: the best k of every query's candidate list (`cand` int32 device
    [nq, R], local rows, -1 padded) by (exact score desc, row asc), padded with (-inf, -1); ids = local row + `index.idx_base`.
    `cache`: the object whose `_ws_ivf` holds the workspace, grown only when too small.  Stream-ordered, no host synchronisation."""
    import torch
    from .ivf import _launch as ivf_launch
    nq, R, dev = int(q16.shape[0]), int(cand.shape[1]), q16.device
    scores = torch.full((nq, int(k)), float("-inf"), dtype=torch.float32, device=dev)
    ids = torch.full((nq, int(k)), -1, dtype=torch.int64, device=dev)
    if nq == 0 or int(index.n_rows) == 0:
        return scores, ids, count
    q16 = q16.contiguous()
    for a in range(0, nq, RESCORE_QUERIES):                      # a query's candidates are one list: order = cand, start[q] = q R, probes[q] = {q}
        b = min(nq, a + RESCORE_QUERIES)
        m = b - a
        start = torch.arange(m + 1, dtype=torch.int64, device=dev) * R
        probes = torch.arange(m, dtype=torch.int32, device=dev)[:, None].contiguous()
        need = index.lib.arx_ivf_workspace_bytes(m * R, m, m, 1, int(index.dim), int(k))
        if cache._ws_ivf is None or cache._ws_ivf.numel() < need:
            cache._ws_ivf = torch.empty(need, dtype=torch.uint8, device=dev)
        s, i, _ = ivf_launch(index.corpus, cand[a:b].reshape(-1), start, R, q16[a:b], probes, int(k), None, None, index.idx_base,
                             None, cache._ws_ivf, index.n_rows)
        scores[a:b], ids[a:b] = s, i
    return scores, ids, count


class CodeIndex:
    """`codes` (device [n_rows, ...], one entry per row of `index`) and `centre` (f32 device [dim] or None), kept as given: nothing
    recomputes the centre, so answers do not depend on how a mean was reduced."""

    def __init__(self, index, codes, centre):
        self.index, self.codes, self.centre = index, codes, centre
        self._ws = self._ws_ivf = None

    @staticmethod
    def check_build(index, centre):
        """The refusals every `build` shares, each a ValueError before any launch: n_rows >= 2^31, a centre of another kind or shape
        -> `check_centre`'s result."""
        n = int(index.n_rows)
        if n >= 1 << 31:
            raise ValueError(f"n_rows={n} must be below 2^31 (the candidate lists hold int32 rows)")
        return check_centre(centre, int(index.dim))

    @staticmethod
    def device_centre(index, centre):
        """`check_centre`'s result -> f32 device [dim] or None: "mean" is the f32 column mean of the rows, computed once here."""
        import torch
        dim, n, dev = int(index.dim), int(index.n_rows), index.corpus.device
        if isinstance(centre, str):
            c = index.corpus[:n].mean(dim=0, dtype=torch.float32) if n else torch.zeros(dim, dtype=torch.float32, device=dev)
        else:
            c = None if centre is None else torch.from_numpy(centre).to(dev)
        return None if c is None else c.contiguous()

    def append(self, rows, index=None) -> None:
        """The shard grew by `rows` (fp16 device [m, dim]): their codes, under what the index keeps, are appended; `index`: the
        `ShardIndex` over the grown shard, where the caller made a new one."""
        import torch
        self.codes = torch.cat([self.codes, self.encode_rows(rows)])
        if index is not None:
            self.index = index

    def compact(self, keep_words, word_rank, count: int, index=None) -> None:
        """Move the kept rows' codes to the front (`arx_compact_rows`, a code's bytes a row), as the shard's rows moved."""
        import torch
        from .mutation import compact_rows_device
        moved = torch.zeros_like(self.codes)
        compact_rows_device(self.codes, moved, int(self.codes.shape[0]), keep_words, word_rank)
        self.codes = moved[:count].contiguous()
        if index is not None:
            self.index = index

    def rows_added(self, lo: int, hi: int, rows, index=None) -> None:
        """`append`, as `HipCollection.add` tells every derived index (the rows are [lo, hi) of the shard)."""
        self.append(rows, index=index)

    rows_compacted = compact                                     # as `HipCollection.compact` tells every derived index

    def _workspace(self, nq: int, R: int):
        import torch
        need = self._scan_bytes(nq, R)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.codes.device)
        return self._ws

    def _require_rows(self) -> None:
        if int(self.codes.shape[0]) != int(self.index.n_rows):
            raise ValueError(f"the index holds {int(self.index.n_rows)} rows, the codes {int(self.codes.shape[0])}: append or compact them first")

    def search(self, q16, k: int, n_candidates: int, allow=None, rows_per_block: Optional[int] = None):
        """(scores f32 [nq, k], ids int64 [nq, k], count int64 [nq]) on the device: the best k of every query's candidate list by
        (exact score desc, row asc), padded with (-inf, -1); ids = local row + the index's idx_base; `count` the candidates scored.
        Stream-ordered, no host synchronisation."""
        self.check(k, n_candidates)
        cand, _, count = self.candidates(q16, n_candidates, allow=allow, rows_per_block=rows_per_block)
        return rescore_candidates(self.index, q16, cand, count, k, self)
