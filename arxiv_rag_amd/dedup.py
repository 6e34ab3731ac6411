"""Near-duplicate chunks: which rows of the corpus are near-copies of an EARLIER row, in embedding space.

Stage 3 cuts 2 000-character chunks with a 400-character overlap, and the reference can only find duplicates by hashing text
(`1-downloader/deduplicate.py`; its embedding analysis counts `chunks_duplicate_text`).  Comparing every chunk with every earlier one is
one N x N x D fp16 matrix product with a triangular mask: `ShardIndex.nearest_earlier` (csrc/prefix.hip) gives, for every row, its
nearest earlier row exactly.

Semantics.  Row r is a DUPLICATE when ANY earlier row (index < r) scores >= threshold against it, whether that earlier row was itself
flagged or not; `dup_of[r]` is then its NEAREST earlier row (highest score, ties to the lower row), else -1.  So the first member of a
run of near-copies is always kept, and chains collapse onto earlier rows: with a ~ b ~ c but a !~ c, both b (onto a) and c (onto b) are
flagged and only a is kept.  The score is the search's dot product of the fp16 rows (`exact_row_score`: fp32 FMA chains), which is the
cosine on the unit rows the encoder writes; fp16 rows are unit only to about 2^-9, so a score is the cosine to within about 2^-8 relative
and an exact copy of a row scores its squared norm, 1 +- 2^-8.  Choose thresholds with that in mind."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np


def nearest_earlier_f64(rows) -> Tuple[np.ndarray, np.ndarray]:
    """The definition in float64: rows [n, D] -> (scores f64 [n], ids int64 [n]); for row r the largest dot product with a row j < r
    and the lowest such j; row 0 has none: (-inf, -1)."""
    x = np.asarray(rows, dtype=np.float64)
    n = x.shape[0]
    scores = np.full(n, -np.inf, np.float64)
    ids = np.full(n, -1, np.int64)
    step = 1024
    for a in range(0, n, step):
        b = min(n, a + step)
        s = x[a:b] @ x[:b].T                                   # [b - a, b]
        s[np.arange(b)[None, :] >= np.arange(a, b)[:, None]] = -np.inf
        j = s.argmax(axis=1)                                   # first maximum = lowest row
        best = s[np.arange(b - a), j]
        ok = best > -np.inf
        scores[a:b] = best
        ids[a:b] = np.where(ok, j, -1)
    return scores, ids


def duplicates_from_nearest(scores, ids, threshold: float) -> np.ndarray:
    """(nearest-earlier scores [n] or [n, k], ids likewise; column 0 is used) -> dup_of int64 [n]: the id of the nearest earlier row where
    its score is >= threshold, else -1."""
    s, i = np.asarray(scores), np.asarray(ids, dtype=np.int64)
    if s.ndim == 2:
        s, i = s[:, 0], i[:, 0]
    return np.where((i >= 0) & (s >= threshold), i, -1).astype(np.int64)


def keep_bitmap(dup_of) -> np.ndarray:
    """dup_of [n] -> uint64 [ceil(n / 64)], the `allow` words of `ShardIndex.search`: bit r set = row r is not a duplicate."""
    from .where import pack_bitmap
    return pack_bitmap(np.asarray(dup_of) < 0)


def check_threshold(threshold) -> float:
    t = float(threshold)
    if not (0.0 < t <= 1.0):                                   # (also rejects nan)
        raise ValueError(f"dedup_threshold={threshold} must be in (0, 1]")
    return t


def find_duplicates(index, threshold: float) -> Tuple[np.ndarray, np.ndarray]:
    """`index` (a `ShardIndex`) -> (dup_of int64 [n] of LOCAL rows, scores f32 [n] of each row's nearest earlier row) on the host.  One
    self-join on the device (`nearest_earlier`, k = 1)."""
    t = check_threshold(threshold)
    s, i = index.nearest_earlier(0, index.n_rows, 1)
    s, i = s.cpu().numpy()[:, 0], i.cpu().numpy()[:, 0]
    local = np.where(i >= 0, i - index.idx_base, -1)
    return duplicates_from_nearest(s, local, t), s


def duplicate_entries(dup_of, scores, chunk_ids: Sequence[str], base: int = 0) -> List[Dict]:
    """The list `HipCollection.duplicates` and `duplicates.json` hold: one entry per flagged row, in row order."""
    out = []
    for r in np.nonzero(np.asarray(dup_of) >= 0)[0].tolist():
        o = int(dup_of[r])
        out.append({"index": base + r, "chunk_id": chunk_ids[r], "duplicate_of_index": base + o, "duplicate_of": chunk_ids[o],
                    "score": float(scores[r])})
    return out
