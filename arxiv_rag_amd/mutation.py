"""Host bookkeeping of a mutable `HipCollection` (`capacity=...`; INTEGRATION.md "Adding and deleting rows"): the id -> row map, the
old -> new row map of a compaction and the compaction of the flat word pieces, plus the device calls of csrc/compact.hip
(`arx_compact_plan`, `arx_compact_rows`).  Everything but `plan_device` and `compact_rows_device` is numpy only."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np


def chunk_id_of(meta: Dict, row: int) -> str:
    """The id `HipCollection.query` returns for a row: its `chunk_id`, else `chunk_<row>`."""
    return meta.get("chunk_id", f"chunk_{row}")


def build_id_map(metadata: Sequence[Dict], base: int = 0, into: Dict = None) -> Dict:
    """-> {id: row} over `metadata` (row = `base` + position), added to a copy of `into`.  An id that occurs twice, in `metadata` or
    against `into`, is a ValueError naming it and the two rows; `into` itself is never changed."""
    ids = dict(into) if into else {}
    for j, m in enumerate(metadata):
        cid = chunk_id_of(m, base + j)
        if cid in ids:
            raise ValueError(f"duplicate id {cid!r}: rows {ids[cid]} and {base + j}")
        ids[cid] = base + j
    return ids


def rows_of_ids(id_map: Dict, ids: Sequence) -> List[int]:
    """The rows of `ids`, in their order; an unknown id is a ValueError naming it."""
    rows = []
    for cid in ids:
        if cid not in id_map:
            raise ValueError(f"unknown id {cid!r}")
        rows.append(id_map[cid])
    return rows


def old_to_new(keep_mask) -> np.ndarray:
    """keep_mask bool [n] -> int64 [n]: the row each old row has after a stable compaction, -1 for a removed one."""
    keep = np.asarray(keep_mask, dtype=bool)
    return np.where(keep, np.cumsum(keep, dtype=np.int64) - 1, -1).astype(np.int64)


def word_rank_host(keep_words: np.ndarray, n_rows: int) -> np.ndarray:
    """What `arx_compact_plan` computes, in numpy: uint64 words [ceil(n / 64)] -> int64 [ceil(n / 64) + 1]."""
    n_words = (n_rows + 63) // 64
    bits = np.unpackbits(np.ascontiguousarray(keep_words[:n_words], dtype="<u8").view(np.uint8), bitorder="little")[:n_rows]
    per_word = np.add.reduceat(bits.astype(np.int64), np.arange(0, n_rows, 64)) if n_rows else np.zeros(0, np.int64)
    out = np.zeros(n_words + 1, np.int64)
    np.cumsum(per_word, out=out[1:])
    return out


def compact_pieces(flat: np.ndarray, doc_ptr: np.ndarray, keep_mask) -> Tuple[np.ndarray, np.ndarray]:
    """The flat word pieces (`keyword.flatten_pieces`' layout) of the kept documents, in order."""
    keep = np.asarray(keep_mask, dtype=bool)
    lens = np.diff(doc_ptr)
    new_ptr = np.zeros(int(keep.sum()) + 1, np.int64)
    np.cumsum(lens[keep], out=new_ptr[1:])
    return np.ascontiguousarray(flat[np.repeat(keep, lens)]), new_ptr


def append_pieces(flat: np.ndarray, doc_ptr: np.ndarray, more_flat: np.ndarray, more_ptr: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    return (np.concatenate([flat, np.asarray(more_flat, flat.dtype)]),
            np.concatenate([doc_ptr, doc_ptr[-1] + np.asarray(more_ptr[1:], np.int64)]))


def piece_lists(flat: np.ndarray, doc_ptr: np.ndarray) -> List[List[int]]:
    """The per-document lists `keyword.build_postings` takes, from the flat layout."""
    return [flat[a:b].tolist() for a, b in zip(doc_ptr[:-1].tolist(), doc_ptr[1:].tolist())]


def unpack_rows(words: np.ndarray, n_rows: int) -> np.ndarray:
    """Row bitmap words (int64 or uint64 [ceil(n / 64)]) -> bool [n]."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n_rows].astype(bool)


# ---- the device calls --------------------------------------------------------------------------------------------------------------
def plan_device(keep_words, n_rows: int):
    """`arx_compact_plan` -> (word_rank int64 [ceil(n / 64) + 1] on the device, count).  Waits for the count."""
    import torch
    from . import _lib
    dev = keep_words.device
    word_rank = torch.empty((n_rows + 63) // 64 + 1, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().arx_compact_plan(keep_words.data_ptr(), int(n_rows), word_rank.data_ptr(), count.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "arx_compact_plan")
    return word_rank, int(count.item())


def compact_rows_device(src, dst, n_rows: int, keep_words, word_rank) -> None:
    """`arx_compact_rows`: the kept rows of `src[:n_rows]` to the front of `dst` (dense tensors of one row size, not overlapping)."""
    import torch
    from . import _lib
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype and src.shape[1:] == dst.shape[1:]
    row_bytes = src.element_size() * (int(np.prod(src.shape[1:])) if src.dim() > 1 else 1)
    _lib.check(_lib.load().arx_compact_rows(src.data_ptr(), dst.data_ptr(), row_bytes, int(n_rows), keep_words.data_ptr(), word_rank.data_ptr(),
                                            torch.cuda.current_stream(src.device).cuda_stream), "arx_compact_rows")
