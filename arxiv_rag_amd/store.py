"""Hand-off from the stage-4 output files to the HBM-resident index.

* `load_embeddings_from_disk` reads what stage 4 leaves on disk — either the layout GEN writes
  (`embeddings.npy` + `metadata.json` + `index.json`, generate_embeddings_parallel.py:271-321) or the batched
  layout of `4-embed/utils/save_embeddings_to_disk.py:15-80` (`embeddings_batch_%04d.npy`,
  `metadata_batch_%04d.json`, `index.json` with `num_batches`), with the same return value as that file's
  `load_embeddings_from_disk` (:82-117): `(embeddings [N, D], metadata list)`.
* `save_embeddings_disk` writes that batched layout (byte-identical to the reference's writer).
* `HipCollection` keeps this rank's rows in HBM as fp16 and answers `query(...)` in the shape of a Chroma
  collection (`ids`, `documents`, `metadatas`, `distances` per query), so code written against the collection the
  reference fills at GEN:404-424 ports over.  Distances are squared L2 (Chroma's default space), which on unit
  rows is `2 - 2*cosine`: the same ranking as the cosine top-k the kernels compute.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def load_embeddings_from_disk(input_dir: str | Path, batch_index: Optional[int] = None,
                              mmap: bool = True) -> Tuple[np.ndarray, List[Dict]]:
    p = Path(input_dir)
    if batch_index is not None:
        emb = np.load(p / f"embeddings_batch_{batch_index:04d}.npy", mmap_mode="r" if mmap else None)
        meta = json.loads((p / f"metadata_batch_{batch_index:04d}.json").read_text(encoding="utf-8"))
        return emb, meta
    index = json.loads((p / "index.json").read_text(encoding="utf-8"))
    if "num_batches" in index:                               # batched layout
        embs, meta = [], []
        for i in range(index["num_batches"]):
            embs.append(np.load(p / f"embeddings_batch_{i:04d}.npy", mmap_mode="r" if mmap else None))
            meta.extend(json.loads((p / f"metadata_batch_{i:04d}.json").read_text(encoding="utf-8")))
        return np.vstack(embs), meta
    emb = np.load(p / "embeddings.npy", mmap_mode="r" if mmap else None)      # GEN layout
    meta = json.loads((p / "metadata.json").read_text(encoding="utf-8"))
    if emb.shape[0] != index.get("total_embeddings", emb.shape[0]):
        raise ValueError(f"{p}: index.json says {index['total_embeddings']} rows, embeddings.npy has {emb.shape[0]}")
    return emb, meta


def save_embeddings_disk(chunks: Sequence[Dict], embeddings, output_dir: str | Path = "./embeddings_saved", batch_size: int = 10000) -> None:
    """Writer of the BATCHED on-disk layout (`4-embed/utils/save_embeddings_to_disk.py:15-80`, the reference's alternative to the three
    files GEN writes): `embeddings_batch_%04d.npy` (float64 — the reference's `.tolist()` round trip — [<= batch_size, D]),
    `metadata_batch_%04d.json` (the GEN fields + `batch_index`, `batch_position`; indent 2, ensure_ascii=False) and `index.json`
    (`total_embeddings`, `embedding_dimension`, `num_batches`, `batch_size`, `chunks` = every chunk's id or null).  Byte-identical to
    what the reference's function writes (tests/golden/harness/expected_batched, produced by that function).  `embeddings`: anything
    indexable by row ([N, D] array, memmap, list of rows); one batch is in memory at a time."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    n = len(embeddings)
    num_batches = (n + batch_size - 1) // batch_size
    dim = int(np.asarray(embeddings[0]).shape[0]) if n else 0
    for i in range(num_batches):
        a, b = i * batch_size, min((i + 1) * batch_size, n)
        np.save(out / f"embeddings_batch_{i:04d}.npy", np.asarray(embeddings[a:b], dtype=np.float64))
        meta = []
        for j, ch in enumerate(chunks[a:b]):
            m = ch.get("metadata", {})
            meta.append({"chunk_id": ch.get("chunk_id", f"chunk_{a + j}"), "paper_id": m.get("paper_id"), "section": m.get("section"),
                         "quality_score": m.get("quality_score"), "text": ch["text"], "text_length": len(ch["text"]),
                         "batch_index": i, "batch_position": j})
        with open(out / f"metadata_batch_{i:04d}.json", "w", encoding="utf-8") as fh:
            json.dump(meta, fh, indent=2, ensure_ascii=False)
    index = {"total_embeddings": n, "embedding_dimension": dim, "num_batches": num_batches, "batch_size": batch_size,
             "chunks": [ch.get("chunk_id") for ch in chunks]}
    with open(out / "index.json", "w", encoding="utf-8") as fh:
        json.dump(index, fh, indent=2)


class HipCollection:
    """This rank's shard of the corpus, resident in HBM, with a Chroma-shaped `query`."""

    def __init__(self, embeddings: np.ndarray, metadata: Sequence[Dict], device="cuda:0", encoder=None,
                 rank: int = 0, world: int = 1, chunk_rows: int = 1 << 18, keyword: bool = False, tokenizer=None,
                 documents: bool = False, dedup_threshold: Optional[float] = None, group_key: Optional[str] = None,
                 where_on_device: bool = False, hybrid_filters: bool = False, hybrid_on_device: bool = False,
                 keyword_build_on_device: bool = False, document_regex: bool = False, capacity: Optional[int] = None):
        """`keyword=True`: also build a BM25 `keyword.KeywordIndex` over this shard's `metadata[i]["text"]` (word pieces of `tokenizer`,
        default the encoder's; corpus statistics summed over all ranks when `world > 1`), which `query(hybrid_alpha=...)` needs.
        `documents=True`: also keep this shard's texts as a UTF-8 blob in HBM (`where_document.DocumentStore`), which
        `query(where_document=...)` scans.
        `dedup_threshold` (a float in (0, 1]; None = off, nothing changes): near-duplicate detection (`dedup.find_duplicates`,
        INTEGRATION.md "Near-duplicate chunks") runs once, here: a row is a duplicate when any EARLIER row scores >= the threshold against
        it (the search's dot product = the cosine on unit rows).  `self.duplicates` lists them
        (`{index, chunk_id, duplicate_of_index, duplicate_of, score}`, the nearest earlier row each) and every `query` skips them: the
        keep-bitmap is and-ed into the filter of `where` / `where_document`, or is the filter when neither is given.  With `world > 1` it
        raises ValueError: a rank sees only its own rows, and a cross-rank join is out of scope.
        `group_key` (a metadata key, e.g. "paper_id"; None = off, nothing changes): consecutive rows of this rank with equal
        `metadata[i][group_key]` are one group (`grouping.runs_from_keys`; a key that reappears after its run ended is a ValueError naming
        the key and the two rows), uploaded once (`ShardIndex.set_groups`); `query(group_by=True)` needs it.
        `where_on_device` (False = nothing changes): `query(where=...)` evaluates the filter on the device from metadata columns kept in
        HBM (`where_device.MetadataColumns`: 9 bytes per row and referenced key, a column built on first use), not with numpy on the
        host; the dedup keep-bitmap and the `where_document` bitmap are and-ed in by the same kernel, so no mask is built or uploaded,
        and a per-query `where` list is evaluated in one launch per 64 distinct filters.  The results are the default path's, bit for
        bit (INTEGRATION.md "where on the device").
        `hybrid_filters` (False = nothing changes; needs `keyword=True`): `query(hybrid_alpha=...)` composes with `where`,
        `where_document`, per-query lists of either, the dedup keep-bitmap and `where_on_device` instead of raising: the bitmaps the
        cosine search is given go to the keyword search unchanged (`KeywordIndex.search(allow=...)`, `arx_bm25_search_filtered`), so
        both candidate lists hold allowed rows only.  The BM25 statistics stay those of the whole corpus (INTEGRATION.md "Hybrid search
        with filters").
        `hybrid_on_device` (False = nothing changes; needs `keyword=True`): `query(hybrid_alpha=...)` fuses the two candidate lists on
        the device (`keyword.fuse_device`, `arx_hybrid_fuse`) and accepts `n_candidates` up to 1024, with or without `reranker`: the
        dense list then comes from `ShardIndex.search_range(-inf)` and the keyword list from `KeywordIndex.search_wide`.  With
        `n_candidates <= 32` the result is the default path's, bit for bit (INTEGRATION.md "Hybrid search on the device").
        `keyword_build_on_device` (False = nothing changes; needs `keyword=True`): the BM25 index is built on the device
        (`KeywordIndex(build_on_device=True)`: `arx_bm25_build_postings`, `arx_bm25_build_impacts`) from the flat word pieces of
        `tokenizer.full_pieces_flat`.  The index is the default build's, bit for bit, so every query answers the same (INTEGRATION.md
        "Building the keyword index on the device").
        `document_regex` (False = nothing changes; needs `documents=True`): `query(where_document=...)` also takes `{"$regex": p}` and
        `{"$not_regex": p}` leaves.  A pattern is compiled on the host to a byte-level DFA (`regex_dfa.compile_regex`: the dialect, its
        ASCII \\d \\w \\s and ASCII-only `(?i)`, at most 256 states and 8 distinct regexes per filter; a refused pattern is a ValueError
        before anything is launched) and `arx_text_regex` scans the texts in HBM; the bitmap goes where the `$contains` one goes, so
        everything that composes with `where_document` composes unchanged (INTEGRATION.md "Document filters").
        `capacity` (None = nothing changes: the collection is immutable and `add`, `delete`, `compact` raise ValueError): the shard is
        allocated with room for that many rows (>= len(embeddings); `world` must be 1) and the collection can grow and shrink
        (INTEGRATION.md "Adding and deleting rows"): `add` appends rows, `delete` tombstones rows in the keep-bitmap every query and-s
        in, `compact` removes the tombstoned rows from HBM on the device (`arx_compact_plan`, `arx_compact_rows`, `arx_compact_text`),
        `get` reads rows by id.  `metadata` is then copied into a list the collection owns, and the ids
        (`metadata[i].get("chunk_id", f"chunk_{i}")`) must be distinct: a duplicate is a ValueError naming it."""
        import torch
        from .index import shard_bounds
        if capacity is not None:
            capacity = int(capacity)
            if world > 1:
                raise ValueError("capacity needs world == 1: the shard bounds of a multi-rank collection are static")
            if capacity < len(embeddings):
                raise ValueError(f"capacity={capacity} is below the {len(embeddings)} rows given")
            from .mutation import build_id_map
            metadata = list(metadata)
            self._ids = build_id_map(metadata)
        self.capacity, self._deleted, self._n_deleted = capacity, None, 0
        if hybrid_filters and not keyword:
            raise ValueError("hybrid_filters=True needs keyword=True: it passes the row filters to the BM25 keyword search")
        if hybrid_on_device and not keyword:
            raise ValueError("hybrid_on_device=True needs keyword=True: it chooses where the BM25 keyword list and the cosine list are fused")
        if keyword_build_on_device and not keyword:
            raise ValueError("keyword_build_on_device=True needs keyword=True: it chooses where the BM25 keyword index is built")
        if document_regex and not documents:
            raise ValueError("document_regex=True needs documents=True: it scans the chunk texts the collection keeps in HBM")
        self.hybrid_filters = bool(hybrid_filters)
        self.document_regex = bool(document_regex)
        self.hybrid_on_device = bool(hybrid_on_device)
        if dedup_threshold is not None:
            from .dedup import check_threshold
            dedup_threshold = check_threshold(dedup_threshold)
            if world > 1:
                raise ValueError("dedup_threshold needs world == 1: a rank sees only its own rows, and a cross-rank join is out of scope")
        n, d = embeddings.shape
        lo, hi = shard_bounds(n, world, rank)
        self.n_total, self.dim, self.lo, self.hi = n, d, lo, hi
        self.world = world
        self.group_key, self.group_keys = group_key, None       # the key of every run of this rank's rows, by `group_of` value
        if group_key is not None:
            from .grouping import runs_from_keys
            group_of, self.group_keys = runs_from_keys([metadata[r].get(group_key) for r in range(lo, hi)], base=lo)
        self.metadata = metadata
        self._where_columns: Dict = {}                          # `query(where=...)`: one numpy column per referenced metadata key
        self.where_on_device, self._device_columns = bool(where_on_device), None
        self.encoder = encoder
        self._buf = torch.empty((hi - lo if capacity is None else capacity, d), dtype=torch.float16, device=device)
        self._buf_spare = self._group_buf = None                # (mutable collections: `compact`'s second buffer, `group_of` at capacity)
        shard = self._buf[:hi - lo]
        for s0 in range(lo, hi, chunk_rows):                   # stream: never a second full copy in host RAM
            s1 = min(hi, s0 + chunk_rows)
            shard[s0 - lo:s1 - lo] = torch.from_numpy(np.ascontiguousarray(embeddings[s0:s1], dtype=np.float16)).to(device)
        self._group_host = None
        if group_key is not None and capacity is not None:
            self._group_host = group_of
            self._group_buf = torch.zeros(capacity, dtype=torch.int32, device=device)
            self._group_buf[:hi - lo] = torch.from_numpy(group_of).to(device)
        self._make_index()
        if group_key is not None and capacity is None:
            self.index.set_groups(group_of)
        self.keyword = None
        self._kw_stale, self._kw_pieces, self._kw_on_device = False, None, bool(keyword_build_on_device)
        if keyword:
            from .keyword import KeywordIndex
            tokenizer = tokenizer if tokenizer is not None else getattr(encoder, "tokenizer", None)
            if tokenizer is None:
                raise ValueError("keyword=True needs a tokenizer (or an encoder that has one)")
            if capacity is None:
                self.keyword = KeywordIndex(texts=[metadata[r].get("text") or "" for r in range(lo, hi)], tokenizer=tokenizer,
                                            stats="global" if world > 1 else None, idx_base=lo, device=device,
                                            **({"build_on_device": True} if keyword_build_on_device else {}))
            else:                                               # the collection keeps its rows' flat word pieces: the index is rebuilt from them
                self._kw_tokenizer = tokenizer
                self._kw_pieces = self._pieces_of([m.get("text") or "" for m in metadata])
                self._rebuild_keyword()
        self.documents = None
        if documents:
            from .where_document import DocumentStore
            self.documents = DocumentStore([metadata[r].get("text") or "" for r in range(lo, hi)], device=device)
        self.dedup_threshold, self.duplicates = dedup_threshold, []
        self._keep_mask = self._keep = None                     # rows that are not duplicates: host bool [n], device bitmap words
        self._boost_spec = self._boost_buf = None               # `set_boost`: the spec (None for an array) and the prior, f32 in HBM
        self._boost_max = 0.0                                   # ... and its largest |finite value| (`arx_prior_info`, once per change)
        if dedup_threshold is not None and hi > lo:
            from .dedup import duplicate_entries, find_duplicates, keep_bitmap
            dup_of, scores = find_duplicates(self.index, dedup_threshold)
            self.duplicates = duplicate_entries(dup_of, scores, [metadata[r].get("chunk_id", f"chunk_{r}") for r in range(lo, hi)], base=lo)
            self._keep_mask = dup_of < 0
            self._keep = torch.from_numpy(keep_bitmap(dup_of).view(np.int64)).to(device)

    @classmethod
    def from_disk(cls, input_dir, **kw) -> "HipCollection":
        emb, meta = load_embeddings_from_disk(input_dir)
        return cls(emb, meta, **kw)

    def count(self) -> int:
        return self.n_total - getattr(self, "_n_deleted", 0)

    # ---- adding and deleting rows (`capacity=...`; INTEGRATION.md "Adding and deleting rows") -----------------------------------
    def _make_index(self):
        """The `ShardIndex` over the rows there are now: the prefix [0, hi - lo) of the capacity buffer.  A new index, so the int8
        copy, the norm bound, the cached workspaces and the groups all describe these rows and no others."""
        from .index import ShardIndex
        shard = self._buf[:self.hi - self.lo]
        dim = int(shard.shape[1])
        self.index = ShardIndex(shard, idx_base=self.lo, prefilter="int8" if (dim % 128 == 0 and 0 < dim <= 1024 and shard.shape[0] > 0) else None,
                                adaptive=True)
        if self._group_buf is not None:                         # (zero rows too: a grouped query of an empty collection returns empty lists)
            self.index.set_groups(self._group_buf[:self.hi - self.lo])

    def _pieces_of(self, texts):
        """(pieces int32 [T], doc_ptr int64 [n + 1]) of `texts`, through the tokenizer call the collection's build path uses."""
        from .keyword import flatten_pieces
        if self._kw_on_device:
            return self._kw_tokenizer.full_pieces_flat(list(texts))
        return flatten_pieces(self._kw_tokenizer._full_pieces(list(texts)))

    def _rebuild_keyword(self):
        """The keyword index of the rows there are now, by the build path the collection was created with: the one a fresh collection
        over these rows builds."""
        from .keyword import KeywordIndex
        from .mutation import piece_lists
        flat, doc_ptr = self._kw_pieces
        dev = self._buf.device
        if self._kw_on_device:
            self.keyword = KeywordIndex(pieces=(flat, doc_ptr), tokenizer=self._kw_tokenizer, idx_base=0, device=dev, build_on_device=True)
        else:
            self.keyword = KeywordIndex(pieces=piece_lists(flat, doc_ptr), tokenizer=self._kw_tokenizer, idx_base=0, device=dev)
        self._kw_stale = False

    def _require_mutable(self, what: str):
        if getattr(self, "capacity", None) is None:
            raise ValueError(f"{what} needs a collection built with capacity=...: without it the collection is immutable")

    def _drop_columns(self):
        """The metadata columns (`where`'s host cache and the device columns) are dropped whenever the rows change, and rebuilt on
        first use."""
        self._where_columns, self._device_columns = {}, None

    def _set_keep(self, mask):
        import torch
        from .where import pack_bitmap
        self._keep_mask = mask
        self._keep = None if mask is None else torch.from_numpy(pack_bitmap(mask).view(np.int64)).to(self._buf.device)

    def add(self, embeddings, metadatas: Sequence[Dict], boost=None) -> None:
        """Append rows (`embeddings` [m, dim], converted to fp16 as the constructor converts them; one metadata dict each).  Everything
        derived is extended: texts, word pieces (the keyword index is rebuilt on its next use), the runs of `group_key`
        (`grouping.continue_runs`: the first new row may continue the last run; a key whose run ended is a ValueError) and, with
        `dedup_threshold`, `duplicates` and the keep-bitmap, from a self-join over the new rows only
        (`ShardIndex.nearest_earlier(row_lo=old_n)`).  ValueError, with nothing added: more rows than `capacity` has room for, a
        duplicate id, another dim, a different number of dicts.  With `set_boost` the prior is extended: from the new metadatas for a
        spec; for an array prior `boost` (floats [m]) is needed, and is refused in every other case."""
        import torch
        from .mutation import append_pieces, build_id_map, chunk_id_of
        self._require_mutable("add")
        emb = np.asarray(embeddings) if not isinstance(embeddings, np.ndarray) else embeddings
        metadatas = list(metadatas)
        if emb.ndim != 2 or emb.shape[1] != self.dim or emb.shape[0] != len(metadatas):
            raise ValueError(f"add: embeddings of shape {tuple(emb.shape)} and {len(metadatas)} metadata dicts; rows of dim {self.dim} and "
                             f"one dict each are needed")
        n, m = self.n_total, len(metadatas)
        if n + m > self.capacity:
            raise ValueError(f"add: {n} rows + {m} new rows exceed capacity={self.capacity}")
        if m == 0:
            return
        prior_new = None
        if getattr(self, "_boost_buf", None) is not None and self._boost_spec is not None:
            if boost is not None:
                raise ValueError("add: boost= cannot be given when set_boost took a spec: the prior of the new rows comes from their metadata")
            from .boost import prior_from_metadata
            prior_new = prior_from_metadata(metadatas, self._boost_spec)
        elif getattr(self, "_boost_buf", None) is not None:
            if boost is None:
                raise ValueError("add: set_boost took an array, so the prior of the new rows is needed: pass boost=[m floats]")
            a = boost.detach().cpu().numpy() if torch.is_tensor(boost) else np.asarray(boost)
            if a.dtype.kind != "f" or a.shape != (m,):
                raise ValueError(f"add: boost must hold floats and have shape ({m},), not {a.dtype} {tuple(a.shape)}")
            with np.errstate(over="ignore"):
                prior_new = np.ascontiguousarray(a, dtype=np.float32)
        elif boost is not None:
            raise ValueError("add: boost= needs set_boost(array) first")
        ids = build_id_map(metadatas, base=n, into=self._ids)
        if self.group_key is not None:
            from .grouping import continue_runs
            group_new, group_keys = continue_runs(self._group_host, self.group_keys, [md.get(self.group_key) for md in metadatas])
        texts = [md.get("text") or "" for md in metadatas]
        pieces = self._pieces_of(texts) if self._kw_pieces is not None else None
        # nothing above changed the collection; from here on nothing can be refused
        dev = self._buf.device
        self._buf[n:n + m] = torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float16)).to(dev)
        self.metadata.extend(metadatas)
        self._ids = ids
        self.n_total = self.hi = n + m
        if self.group_key is not None:
            self._group_host, self.group_keys = np.concatenate([self._group_host, group_new]), group_keys
            self._group_buf[n:n + m] = torch.from_numpy(group_new).to(dev)
        if pieces is not None:
            self._kw_pieces, self._kw_stale = append_pieces(*self._kw_pieces, *pieces), True
        if self.documents is not None:
            self.documents.append(texts)
        self._drop_columns()
        self._make_index()
        if prior_new is not None:
            self._boost_buf[n:n + m] = torch.from_numpy(prior_new).to(dev)
            self._measure_prior((n, n + m))
        for derived in self._derived():                          # labelled, packed, encoded, linked in (or the graph goes stale)
            derived.rows_added(n, n + m, self._buf[n:n + m], index=self.index)
        if self._deleted is not None:
            self._deleted = np.concatenate([self._deleted, np.zeros(m, bool)])
        if self.dedup_threshold is not None:
            from .dedup import duplicate_entries, duplicates_from_nearest
            s, i = self.index.nearest_earlier(n, n + m, 1)
            s, i = s.cpu().numpy()[:, 0], i.cpu().numpy()[:, 0]
            dup_new = duplicates_from_nearest(s, i, self.dedup_threshold)
            dup_of = np.concatenate([np.full(n, -1, np.int64), dup_new])
            scores = np.concatenate([np.zeros(n, s.dtype), s])
            self.duplicates = self.duplicates + [e for e in duplicate_entries(dup_of, scores, [chunk_id_of(md, r) for r, md in enumerate(self.metadata)])]
            old = self._keep_mask if self._keep_mask is not None else np.ones(n, bool)
            self._set_keep(np.concatenate([old, dup_new < 0]))
        elif self._keep_mask is not None:
            self._set_keep(np.concatenate([self._keep_mask, np.ones(m, bool)]))

    def delete(self, ids: Optional[Sequence] = None, where=None, where_document=None) -> int:
        """Tombstone rows: those of the `chunk_id`s in `ids` (an unknown one is a ValueError naming it) and / or those a `where` /
        `where_document` filter selects, evaluated by the path a query's filters take; with several arguments a row must satisfy all of
        them, as in Chroma.  At least one is needed.  The rows' bits are cleared in the keep-bitmap every query and-s in, so no query
        returns them from this moment (with `hybrid_alpha` that needs `hybrid_filters=True`, as for every keep-bitmap); they stay in HBM,
        and in the BM25 statistics, until `compact()`.  Their ids are forgotten at once.  -> the number of rows deleted.  With
        `dedup_threshold` it raises ValueError: a deleted original may un-hide its duplicates, and re-joining them is out of scope."""
        from .mutation import chunk_id_of, rows_of_ids, unpack_rows
        self._require_mutable("delete")
        if self.dedup_threshold is not None:
            raise ValueError("delete cannot be used on a collection built with dedup_threshold: a deleted original may un-hide its duplicates")
        if ids is None and where is None and where_document is None:
            raise ValueError("delete needs ids, where or where_document")
        n = self.n_total
        hit = np.ones(n, bool)
        if ids is not None:
            by_id = np.zeros(n, bool)
            by_id[rows_of_ids(self._ids, list(ids))] = True
            hit &= by_id
        if where is not None or where_document is not None:
            words, _ = self._row_filters().allow_of(where, where_document)
            hit &= unpack_rows(words.cpu().numpy(), n)
        if self._deleted is not None:
            hit &= ~self._deleted
        rows = np.nonzero(hit)[0].tolist()
        if not rows:
            return 0
        for r in rows:
            del self._ids[chunk_id_of(self.metadata[r], r)]
        self._deleted = hit if self._deleted is None else (self._deleted | hit)
        self._n_deleted = int(self._deleted.sum())
        self._set_keep(~self._deleted)
        return len(rows)

    def compact(self) -> np.ndarray:
        """Remove the tombstoned rows for good, on the device: one `arx_compact_plan`, `arx_compact_rows` for the shard (into a second
        capacity-sized buffer the collection keeps from then on; the two swap) and for `group_of`, `arx_compact_text` for the texts.
        The host lists are compacted, the id map is rebuilt (a row without a `chunk_id` is `chunk_<its new row>`), the keyword index is
        rebuilt on its next use, so its statistics become the survivors', and the tombstones are cleared.  -> int64 [rows before]: every
        old row's new row, -1 for a removed one.  Afterwards the collection answers as one built from the survivors in order."""
        import torch
        from . import _lib
        from .mutation import build_id_map, compact_pieces, compact_rows_device, old_to_new, plan_device
        self._require_mutable("compact")
        n = self.n_total
        if self._deleted is None or not self._deleted.any():
            return np.arange(n, dtype=np.int64)
        keep = ~self._deleted
        word_rank, count = plan_device(self._keep, n)
        if count != int(keep.sum()):
            raise _lib.ArxError(f"arx_compact_plan counted {count} rows, the host's tombstones leave {int(keep.sum())}")
        if self._buf_spare is None:
            self._buf_spare = torch.empty_like(self._buf)
        compact_rows_device(self._buf, self._buf_spare, n, self._keep, word_rank)
        self._buf, self._buf_spare = self._buf_spare, self._buf
        if self._group_buf is not None:
            moved = torch.zeros_like(self._group_buf)
            compact_rows_device(self._group_buf, moved, n, self._keep, word_rank)
            self._group_buf, self._group_host = moved, self._group_host[keep]
        if self.documents is not None:
            self.documents.compact(self._keep, word_rank, count)
        if getattr(self, "_boost_buf", None) is not None:      # the prior moves as `group_of` moves: 4-byte rows
            moved = torch.zeros_like(self._boost_buf)
            compact_rows_device(self._boost_buf, moved, n, self._keep, word_rank)
            self._boost_buf = moved
        keep_words = self._keep
        self.metadata = [md for md, k in zip(self.metadata, keep.tolist()) if k]
        self._ids = build_id_map(self.metadata)
        if self._kw_pieces is not None:
            self._kw_pieces, self._kw_stale = compact_pieces(*self._kw_pieces, keep), True
        self.n_total = self.hi = count
        self._deleted, self._n_deleted = None, 0
        self._set_keep(None)
        self._drop_columns()
        self._make_index()
        if getattr(self, "_boost_buf", None) is not None:      # (the survivors' maximum: what a collection built from them measures)
            self._measure_prior()
        for derived in self._derived():                          # what each keeps per row moves as the rows moved, by the old keep-bitmap
            derived.rows_compacted(keep_words, word_rank, count, index=self.index)
        return old_to_new(keep)

    def _derived(self):
        """The indexes built over the rows that follow them through `add` and `compact` (`rows_added`, `rows_compacted`), in the order
        they are told."""
        return [ix for ix in (getattr(self, name, None) for name in ("ivf", "binary", "pq", "graph")) if ix is not None]

    def _prior(self):
        """The prior of the rows there are now (a view of the capacity-sized buffer), or None."""
        return None if getattr(self, "_boost_buf", None) is None else self._boost_buf[:self.hi - self.lo]

    def _measure_prior(self, rows=None) -> None:
        """`arx_prior_info` over the prior (or its rows [rows[0], rows[1]): the new ones, whose maximum joins the kept one)."""
        p = self._prior()
        if rows is None:
            self._boost_max = self.index.prior_info(p)[0] if p.numel() else 0.0
        elif rows[1] > rows[0]:
            self._boost_max = max(self._boost_max, self.index.prior_info(p[rows[0]:rows[1]])[0])

    def set_boost(self, spec_or_array) -> Optional[Dict]:
        """The per-row prior `query(boost_weight=...)` adds to the cosine (INTEGRATION.md "Boosted search").  A dict is a spec of
        `boost.prior_from_metadata` ({"key": K, "missing": 0.0}, or with "decay": "exp", "origin", "half_life"), evaluated over this
        rank's metadata and again over the new rows of every `add`; a float array or tensor [rows] is taken as it is (`add` then needs
        `boost=`).  The prior is kept in HBM as f32 (at `capacity` on a mutable collection), `arx_prior_info` runs once, and rows with
        a NaN or +-inf prior are hidden from every boosted query.  `set_boost(None)` clears it.  -> {"rows", "max_abs_prior",
        "non_finite"} (None after clearing).  ValueError: a bad spec, a non-numeric metadata value, another length."""
        import torch
        from .boost import prior_from_metadata
        if spec_or_array is None:
            self._boost_spec = self._boost_buf = None
            self._boost_max = 0.0
            return None
        rows = self.hi - self.lo
        if isinstance(spec_or_array, dict):
            spec = dict(spec_or_array)
            prior = prior_from_metadata([self.metadata[r] for r in range(self.lo, self.hi)], spec)
        else:
            spec = None
            a = spec_or_array.detach().cpu().numpy() if torch.is_tensor(spec_or_array) else np.asarray(spec_or_array)
            if a.dtype.kind != "f" or a.shape != (rows,):
                raise ValueError(f"set_boost: a prior array must hold floats and have shape ({rows},), not {a.dtype} {tuple(a.shape)}")
            with np.errstate(over="ignore"):
                prior = np.ascontiguousarray(a, dtype=np.float32)
        cap = getattr(self, "capacity", None)
        buf = torch.zeros(rows if cap is None else cap, dtype=torch.float32, device=self._buf.device)
        buf[:rows] = torch.from_numpy(prior).to(buf.device)
        self._boost_spec, self._boost_buf = spec, buf
        self._measure_prior()
        return {"rows": rows, "max_abs_prior": self._boost_max, "non_finite": int((~np.isfinite(prior)).sum())}

    def build_ivf(self, n_lists: int, iters: int = 10, seed: int = 0, train_rows: Optional[int] = None) -> Dict:
        """Build the inverted lists `query(nprobe=...)` needs (INTEGRATION.md "IVF probe search"; `ivf.IvfIndex.build`): k-means with
        `n_lists` centroids on a sample of this collection's rows (tombstoned ones included: the keep-bitmap hides them at query
        time), every row labelled, the rows sorted by list.  Again replaces the index; nothing re-fits the centroids otherwise: `add`
        labels the new rows against them, `compact` moves the labels.  -> {n_lists, list_rows_min / median / max, iterations,
        train_rows, seconds}.  ValueError before any launch: `world > 1`, an empty collection, the refusals of `IvfIndex.build`."""
        from .ivf import IvfIndex, check_build_args
        if getattr(self, "world", 1) > 1:
            raise ValueError("build_ivf needs world == 1: more than one rank is out of scope")
        check_build_args(self.hi - self.lo, self.dim, n_lists, iters, train_rows)
        self.ivf = IvfIndex.build(self.index, n_lists, iters=iters, seed=seed, train_rows=train_rows)
        return self.ivf.summary()

    def build_binary(self, centre="mean") -> Dict:
        """Pack the sign-bit codes `query(binary_candidates=...)` needs (INTEGRATION.md "Binary-code search";
        `binary.BinaryIndex.build`): one bit per dimension, `x[j] > centre[j]`, of every row (tombstoned ones included: the keep-bitmap
        hides them at query time).  `centre`: "mean" (the f32 column mean of the rows there are now, computed once and kept), None (0)
        or a float array [dim].  Again replaces the codes and the centre; nothing recomputes the centre otherwise: `add` packs the new
        rows with it, `compact` moves the codes.  -> {rows, words_per_row, code_bytes, centre}.  ValueError before any launch:
        `world > 1`, a dim that is not a multiple of 64 in [64, 8192], a centre of another shape."""
        from .binary import BinaryIndex, check_centre, check_dim
        if getattr(self, "world", 1) > 1:
            raise ValueError("build_binary needs world == 1: more than one rank is out of scope")
        check_dim(int(self.dim))
        kind = check_centre(centre, int(self.dim))
        self.binary = BinaryIndex.build(self.index, centre=kind)
        n, w = (int(v) for v in self.binary.codes.shape)
        return {"rows": n, "words_per_row": w, "code_bytes": n * w * 8, "centre": "mean" if isinstance(kind, str) else ("none" if kind is None else "given")}

    def build_pq(self, dsub: int = 8, centre="mean", train_rows: int = 65536, iters: int = 10, seed: int = 0, codebooks=None) -> Dict:
        """Train the codebooks and encode the 8-bit PQ codes `query(pq_candidates=...)` needs (INTEGRATION.md "Product-quantised
        search"; `pq.PqIndex.build`): one byte per `dsub` dimensions of every row (tombstoned ones included: the keep-bitmap hides
        them at query time), the nearest of 256 sub-centroids to the centred row.  `centre` as `build_binary` takes it; `codebooks`: a
        float array [dim / dsub, 256, dsub] kept unchanged, or None: Lloyd's algorithm over at most `train_rows` rows, `iters` rounds.
        Again replaces the codes, the codebooks and the centre; nothing recomputes them otherwise: `add` encodes the new rows with
        them, `compact` moves the codes.  -> {rows, dsub, bytes_per_row, code_bytes, centre, trained}.  ValueError before any launch:
        `world > 1`, a dim, dsub or dim / dsub outside the limits, a centre or codebooks of another shape or not finite, an empty
        collection without `codebooks`."""
        from .binary import check_centre
        from .pq import PqIndex, check_codebooks, check_dsub
        if getattr(self, "world", 1) > 1:
            raise ValueError("build_pq needs world == 1: more than one rank is out of scope")
        check_dsub(int(self.dim), dsub)
        kind = check_centre(centre, int(self.dim))
        if codebooks is not None:
            codebooks = check_codebooks(codebooks, int(self.dim), dsub)
        self.pq = PqIndex.build(self.index, dsub=dsub, centre=kind, codebooks=codebooks, train_rows=train_rows, iters=iters, seed=seed)
        n, m = (int(v) for v in self.pq.codes.shape)
        return {"rows": n, "dsub": int(dsub), "bytes_per_row": m, "code_bytes": n * m,
                "centre": "mean" if isinstance(kind, str) else ("none" if kind is None else "given"), "trained": codebooks is None}

    def build_graph(self, degree: int = 32, n_entry_lists: Optional[int] = None, iters: int = 10, seed: int = 0, nprobe: Optional[int] = None,
                    maintain: bool = False, insert_ef: int = 64) -> Dict:
        """Build the k-NN graph `query(graph_ef=...)` walks (INTEGRATION.md "Graph search"; `graph.GraphIndex.build`) over this
        collection's rows (tombstoned ones included: the keep-bitmap hides them at query time and they stay bridges of the walk).
        `nprobe` (needs `build_ivf` first): the k-NN lists come from the IVF search with that many probes, an approximate build.
        Again replaces the graph.  `delete` needs nothing; `add` and `compact` make the graph stale, and `query(graph_ef=...)` then
        raises until `build_graph` has run again.  With `maintain=True` (a collection with `capacity=`) the graph follows the rows
        instead (INTEGRATION.md "Keeping the graph"): `add` links the new rows in (`GraphIndex.insert`, a walk of width `insert_ef`
        in [31, 512] a row), `compact` moves and renumbers the lists (`GraphIndex.remap`), and the graph never goes stale.
        -> {rows, degree, edges, entry_lists, inserted, orphans, approximate, seconds}.  ValueError before any launch: `world > 1`,
        an empty collection, `nprobe` without `build_ivf`, `maintain` without `capacity`, an `insert_ef` outside its range, the
        refusals of `graph.check_build_args`."""
        from .graph import KNN, MAX_EF, GraphIndex, _is_int, check_build_args
        if getattr(self, "world", 1) > 1:
            raise ValueError("build_graph needs world == 1: more than one rank is out of scope")
        if maintain and getattr(self, "capacity", None) is None:
            raise ValueError("build_graph(maintain=True) needs a collection built with capacity=...: without it the collection is immutable")
        if maintain and (not _is_int(insert_ef) or not (KNN - 1 <= insert_ef <= MAX_EF)):
            raise ValueError(f"insert_ef={insert_ef!r} must be an integer in [{KNN - 1}, {MAX_EF}]")
        ivf = getattr(self, "ivf", None) if nprobe is not None else None
        if nprobe is not None and ivf is None:
            raise ValueError("build_graph(nprobe=...) needs an IVF index: call build_ivf(n_lists) first")
        check_build_args(self.hi - self.lo, self.dim, degree, ivf.n_lists if ivf is not None and n_entry_lists is None else n_entry_lists, iters,
                         nprobe=nprobe, has_ivf=ivf is not None)
        self.graph = GraphIndex.build(self.index, degree=degree, n_entry_lists=n_entry_lists, iters=iters, seed=seed, ivf=ivf, nprobe=nprobe)
        self.graph.maintain, self.graph.insert_ef = bool(maintain), int(insert_ef)
        if maintain:
            self.graph.reserve(self.capacity)
        return self.graph.summary()

    def get(self, ids: Sequence) -> Dict:
        """-> {ids, metadatas, documents} of the rows with these `chunk_id`s, in the order asked, from the host lists (the shape of one
        query's lists in `query`'s result).  An unknown or deleted id is a ValueError naming it."""
        from .mutation import build_id_map, rows_of_ids
        id_map = getattr(self, "_ids", None)
        if id_map is None:                                       # (an immutable collection: the map is built when first asked for)
            id_map = self._ids = build_id_map([self.metadata[r] for r in range(self.lo, self.hi)], base=self.lo)
        ms = [self.metadata[r] for r in rows_of_ids(id_map, list(ids))]
        return {"ids": list(ids), "documents": [m.get("text") for m in ms],
                "metadatas": [{k: m.get(k) for k in ("paper_id", "section", "quality_score")} for m in ms]}

    def _columns(self):
        if self._device_columns is None:
            from .where_device import MetadataColumns
            self._device_columns = MetadataColumns(self.metadata, self.lo, self.hi, self.index.corpus.device)
        return self._device_columns

    def _documents(self):
        if self.documents is None:
            raise ValueError("where_document needs a collection built with documents=True")
        return self.documents

    def _row_filters(self):
        """This shard's `retrieval.RowFilters`: the bitmaps of `where`, `where_document` and the dedup keep-bitmap."""
        from .retrieval import RowFilters
        return RowFilters(self.metadata, self.index.corpus.device, self.lo, self.hi, keep_mask=self._keep_mask, keep_words=self._keep,
                          documents=self._documents, columns=self._columns, where_on_device=getattr(self, "where_on_device", False),
                          cache=self._where_columns, document_regex=getattr(self, "document_regex", False))

    def facets(self, keys, where=None, where_document=None, top: Optional[int] = 10):
        """Facet counts (INTEGRATION.md "Facet counts"): for every key of `keys`, how many of the rows a query with these filters could
        return hold each of its values.  `keys`: a list of specs (one spec alone is a list of one): a metadata key name (faceted over
        its strings if any row has a string there, else its numbers, else its bools), `{"key": k, "kind": "string" | "number" | "bool"}`
        or `{"key": k, "edges": [e0, e1, ...]}` (numbers counted per interval [e_i, e_i+1), the last one closed).  -> one dict per key,
        `{key, values, counts, distinct, missing, unbinned, total}`: the `top` values with the most rows (count descending, then value
        ascending; `top=None`: every value with a row; for `edges` every `(lo, hi)` interval in order, empty ones included), `distinct`
        the values with at least one row, `missing` the allowed rows without a value of the kind, `unbinned` those with a NaN or a number
        outside the edges, `total` the allowed rows.  Numbers come back as floats.
        `where` / `where_document` are what `query` takes, evaluated by the same `retrieval.RowFilters` (on the host, or on the device
        with `where_on_device`; the dedup and tombstone keep-bitmap and-ed in); a list of either gives a list of results, one per entry,
        the distinct (where, where_document) pairs evaluated once.  The counting runs on the device (`facets.count`,
        `arx_facet_count`) from the metadata columns `where_on_device` uses, built on first use whether or not the collection has that
        flag.  ValueError, before anything is launched: a malformed spec or `top`; `world > 1` (ranks number their strings separately
        and a per-rank top list cannot be merged exactly); more than 2^20 distinct values under one key."""
        from . import facets as F
        from .filter_sets import is_per_query
        if getattr(self, "world", 1) > 1:
            raise ValueError("facets needs world == 1: ranks number their strings separately, and a per-rank top list cannot be merged exactly")
        specs = [keys] if isinstance(keys, (str, dict)) else list(keys)
        for s in specs:
            F.parse_spec(s)
        F._check_top(top)
        rf = self._row_filters()
        if is_per_query(where) or is_per_query(where_document):
            nq = len(where) if is_per_query(where) else len(where_document)
            bitmaps, filter_of, _ = rf.per_query(nq, where, where_document)
            per_filter = F.count(self._columns(), specs, bitmaps, top) if nq else []
            return [per_filter[f] for f in filter_of]
        if where_document is not None:
            self._documents()
        allow, _ = rf.allow_of(where, where_document)
        return F.count(self._columns(), specs, allow, top)[0]

    def topics(self, n_topics: int, where=None, where_document=None, iters: int = 20, seed: int = 0, representatives: int = 3,
               store_as: Optional[str] = None) -> Dict:
        """Topic clustering (INTEGRATION.md "Topics"): spherical k-means (`topics.kmeans`) of the rows a query with these filters could
        return, by their embeddings, on the device.  `where` / `where_document` are what `query` takes (single dicts), evaluated by the
        same `retrieval.RowFilters`, the dedup and tombstone keep-bitmap and-ed in; with any of them the allowed rows are gathered once
        (`arx_gather_rows`) into a buffer of their own and clustered as a collection built from them alone would be, bit for bit.
        -> {labels, sizes, centroids, objective, iterations, representatives}: `labels` numpy int32 [rows of this collection], -1 for a
        row that was not clustered; `sizes` [n_topics]; `centroids` f32 [n_topics, dim]; `objective` the mean cosine of a row to its
        centroid; `iterations` the assigns run (at most `iters`; fewer once an assign changes no label); `representatives` per topic
        the `representatives` (0..32) allowed rows nearest its centroid, from one exact `index.search(centroids_f16, k, allow=...)`
        with its ordering rule, as `{ids, indices, scores, documents, labels}`: a representative is usually a member of its topic but
        need not be, so its own label is given.  The default initial centroids are `n_topics` of the clustered rows chosen by
        `numpy.random.default_rng(seed)`; of two identical rows among them the higher-numbered topic is empty in the first assign and
        keeps its value (empty topics are not relocated).
        `store_as` (a metadata key, e.g. "topic"): writes `metadata[r][store_as] = int(label)` for every clustered row, leaves the
        others untouched and drops the metadata columns, so `facets(store_as)` and `query(where={store_as: 3})` see the topics.
        Nothing else is kept.  ValueError before anything is launched: `world > 1` (a rank sees only its own rows); `representatives`
        outside [0, 32]; `n_topics` outside [1, min(clustered rows, 4096)]; `iters < 1`; a dim that is not a multiple of 64."""
        from . import topics as T
        if getattr(self, "world", 1) > 1:
            raise ValueError("topics needs world == 1: a rank sees only its own rows, and a multi-rank fit is out of scope")
        T.check_representatives(representatives)
        if store_as is not None and not isinstance(store_as, str):
            raise ValueError(f"store_as={store_as!r} must be a metadata key name or None")
        T.check_args(max(self.hi - self.lo, 1), self.dim, 1, iters)  # (dim and iters, before a filter is evaluated)
        if where_document is not None:
            self._documents()
        allow, _ = self._row_filters().allow_of(where, where_document)
        res = T.fit_shard(self.index, allow, n_topics, iters=iters, seed=seed, representatives=representatives)
        labels, reps = res["labels"], []
        for s, i in zip(res["rep_scores"], res["rep_rows"]):
            found = [int(r) for r in i if r >= 0]
            ms = [self.metadata[r] for r in found]
            reps.append({"ids": [m.get("chunk_id", f"chunk_{r}") for m, r in zip(ms, found)], "indices": found, "scores": s[i >= 0].tolist(),
                         "documents": [m.get("text") for m in ms], "labels": [int(labels[r - self.lo]) for r in found]})
        if store_as is not None:
            for r in np.nonzero(labels >= 0)[0].tolist():
                self.metadata[self.lo + r][store_as] = int(labels[r])
            self._drop_columns()
        return {"labels": labels, "sizes": res["sizes"], "centroids": res["centroids"], "objective": res["objective"],
                "iterations": res["iterations"], "representatives": reps}

    def assign_topics(self, centroids, where=None, where_document=None, store_as: Optional[str] = None) -> Dict:
        """Label rows against given topic centroids (INTEGRATION.md "Topics"; `topics.predict`, `arx_cluster_assign`) without a new
        fit: after `res = topics(...)` and `add(...)`, `assign_topics(res["centroids"], store_as="topic")` brings the stored labels up
        to date.  `centroids`: f32 or fp16 [C, dim] (numpy or torch), f32 rounded to fp16 as the fit rounds its own, so on the rows of
        the fit `assign_topics(res["centroids"])` reproduces `res["labels"]`.  The rows labelled are those a query with these filters
        could return: `where` / `where_document` go through the same `retrieval.RowFilters` as in `topics`, the dedup and tombstone
        keep-bitmap and-ed in, and the allowed rows are gathered as there.
        -> {labels, scores, sizes}: `labels` numpy int32 [rows of this collection], -1 for an excluded row, else the lowest centroid
        that maximises the exact score of the row; `scores` f32, that score, nan for an excluded row; `sizes` int64 [C].
        `store_as` writes `metadata[r][store_as] = int(label)` for every labelled row and drops the metadata columns, as in `topics`.
        ValueError before anything is launched: `world > 1`; a `store_as` that is not a string; centroids of the wrong shape or
        dtype, with a value that is not finite, or more than 4096 of them; a dim that is not a multiple of 64."""
        from . import topics as T
        if getattr(self, "world", 1) > 1:
            raise ValueError("assign_topics needs world == 1: a rank sees only its own rows")
        if store_as is not None and not isinstance(store_as, str):
            raise ValueError(f"store_as={store_as!r} must be a metadata key name or None")
        T.check_centroids(centroids, self.dim)
        if where_document is not None:
            self._documents()
        allow, _ = self._row_filters().allow_of(where, where_document)
        res = T.label_shard(self.index, allow, centroids)
        if store_as is not None:
            labels = res["labels"]
            for r in np.nonzero(labels >= 0)[0].tolist():
                self.metadata[self.lo + r][store_as] = int(labels[r])
            self._drop_columns()
        return res

    def query(self, query_embeddings=None, query_texts: Optional[Sequence[str]] = None, n_results: int = 10, reranker=None,
              n_candidates: int = 32, hybrid_alpha: Optional[float] = None, where=None, where_document=None,
              mmr_lambda: Optional[float] = None, group_by=None, chunks_per_group: int = 1, min_score=None,
              nprobe: Optional[int] = None, binary_candidates: Optional[int] = None, boost_weight=None,
              pq_candidates: Optional[int] = None, graph_ef: Optional[int] = None, graph_entries: int = 8) -> Dict:
        """Between the encoded queries and the rerank step this is the pipeline `search_queries` runs too: `retrieval.RowFilters` builds
        the row bitmaps, `retrieval.retrieve` searches, picks by MMR and fuses.
        `reranker` (a `rerank.HipCrossEncoder`; needs `query_texts`): the search fetches `n_candidates` (<= 32) rows per query,
        the cross-encoder scores (query, document) for each, and the best `n_results` come back in reranked order with an added
        `rerank_scores` list per query (`scores` / `distances` stay the cosine ones).
        `hybrid_alpha` (a float in [0, 1]; needs `query_texts` and a collection built with `keyword=True`; None = cosine only): the
        cosine search and the BM25 keyword search each fetch `n_candidates` (<= 32) rows per query, `keyword.fuse` ranks their union by
        `alpha * normalised cosine + (1 - alpha) * normalised BM25` and the best `n_results` come back with added `hybrid_scores` and
        `keyword_scores` lists.  `scores` / `distances` stay the cosine ones where the row came from the dense list and are nan where
        it came from the keyword list only (`keyword_scores` is nan where the row was not in the keyword list).  With `reranker` as
        well, the cross-encoder receives the fused top `n_candidates` instead of the dense ones.
        `where` (a Chroma filter: implicit `$eq`, `$eq $ne $gt $gte $lt $lte $in $nin`, `$and` / `$or`; `where.compile_where`): only rows
        whose metadata satisfies it can be returned.  It is evaluated on this rank's rows, packed into a bitmap and applied INSIDE the
        search (`ShardIndex.search(allow=...)`), so the result is the exact top-`n_results` of the satisfying rows — shorter lists when
        fewer satisfy it.  Composes with `reranker` (the cross-encoder sees the filtered candidates).  With `hybrid_alpha` it raises
        ValueError: the BM25 kernel has no row filter, and fusing a filtered dense list with an unfiltered keyword list would return
        disallowed rows.
        `where_document` (`{"$contains": s}`, `{"$not_contains": s}`, `$and` / `$or`; `where_document.compile_where_document`; needs a
        collection built with `documents=True`): only rows whose text satisfies it (case-sensitive substring) can be returned.  The texts
        of this rank's rows are scanned on the device (`arx_text_contains`), the tree is folded over the pattern bitmaps there, and the
        resulting bitmap goes to the same filtered search as `where`; with `where` as well the two bitmaps are and-ed on the device.
        Composes with `reranker`; with `hybrid_alpha` it raises ValueError for the same reason as `where`.
        `mmr_lambda` (a float in [0, 1]; None = off, nothing changes): maximal marginal relevance (INTEGRATION.md "MMR").  The search
        fetches `n_candidates` (in [n_results, 32]) rows per query, with `where` / `where_document` applied as without it, and
        `mmr.mmr_select` picks `n_results` of them on the device: first the most relevant, then each time the row that maximises
        `lambda * cos(q, row) - (1 - lambda) * max cos(row, picked row)`.  The lists come back in pick order; `scores` / `distances` stay
        the search's cosine values of the picked rows and an added `mmr_scores` list per query holds the objective at each pick.
        Together with `reranker` or `hybrid_alpha` it raises ValueError: diversifying a reranked or a fused list is out of scope.
        A collection built with `dedup_threshold` never returns a row it flagged as a duplicate, whatever the other parameters; with
        `hybrid_alpha` it raises ValueError for the same reason as `where`.
        `where` and `where_document` may each also be a list or tuple with ONE ENTRY PER QUERY, a filter dict or None (no filter for that
        query); a list of another length is a ValueError.  Each query is then restricted to its own filter (and-ed with the other
        argument's entry, or its single dict, and with the dedup keep-bitmap): the bitmap of every distinct (where, where_document) pair
        is built once and the whole batch is answered by `ShardIndex.search_filtered_many`, which reads the shard once, not once per
        filter; a batch with more than 64 distinct pairs is cut into calls of at most 64.  Query by query the result is what the same
        call with that query alone and its own dict returns; `reranker` and `mmr_lambda` compose as before, `hybrid_alpha` raises the
        same ValueError.  A single dict (or None) means what it meant.
        `group_by=True` (needs a collection built with `group_key`; absent / None / False = nothing changes): grouped results
        (INTEGRATION.md "Grouped results").  `n_results` (<= 32) then counts PAPERS: the exact best papers by their best visible chunk,
        each with its `chunks_per_group` (<= 8) best visible chunks (`ShardIndex.search_grouped`).  The usual lists are flattened paper
        by paper, best paper first and within a paper the best chunk first; added `group_keys` holds the papers' keys per query and
        `group_sizes` the chunks returned for each.  Composes with a single `where`, `where_document` and the dedup keep-bitmap (one
        bitmap per call).  ValueError with `reranker`, `hybrid_alpha`, `mmr_lambda`, per-query filter lists, `world > 1` (a paper may
        straddle ranks) or a collection built without `group_key`.
        `min_score` (a float or one float per query; None = nothing changes): a score threshold (INTEGRATION.md "Score threshold").  Every
        row whose cosine to the query is >= its threshold, compared in f32, qualifies (-inf: every row; +inf or NaN: none), and the best
        `n_results` qualifying rows come back, `n_results` then in 1..1024 (`ShardIndex.search_range`).  The usual lists have their
        natural, variable lengths, and an added `truncated` list holds one bool per query: True when more rows qualified than the
        search was asked for (how many more is not known: counting them would cost a full exact scan).  Composes with a single `where`,
        `where_document` and the dedup keep-bitmap (one bitmap per call), and with `reranker`: `n_candidates` may then be up to 1024, the
        cross-encoder receives the range list (`truncated` refers to it) and scores its pairs in batches of at most 32, so
        `min_score=float("-inf"), n_candidates=50` is "re-rank the top 50".  ValueError with `hybrid_alpha`, `mmr_lambda`, `group_by`,
        per-query filter lists and `world > 1` (a cross-rank merge of long lists is out of scope).
        On a collection built with `hybrid_filters=True` every "raises ValueError with `hybrid_alpha`" above that is about a row filter
        (`where`, `where_document`, per-query lists, `dedup_threshold`) is lifted: the keyword search is restricted by the very bitmaps
        of the cosine search, query by query, `fuse` and `reranker` work as without a filter, and idf / avgdl stay corpus-wide.
        `mmr_lambda`, `group_by` and `min_score` stay refused with `hybrid_alpha`.
        On a collection built with `hybrid_on_device=True`, `hybrid_alpha` takes `n_candidates` up to 1024 (each side's list and the
        fused list a `reranker` receives, whose pairs are then scored 32 at a time) and the fusion runs on the device; beyond 32
        candidates it raises ValueError with per-query filter lists and with `world > 1`.  Everything else stays as above.
        `nprobe` (an integer in [1, min(128, n_lists)]; None = nothing changes; needs `build_ivf` first): the IVF probe search
        (INTEGRATION.md "IVF probe search").  Every query is scored against the rows of its `nprobe` nearest lists only
        (`ivf.IvfIndex.search`, `arx_ivf_search`): the exact top rows among those, with the score bits and the order of the exact
        search, and an added `ivf_scanned` list holds the rows scored per query.  `nprobe = n_lists` is the exact search.  Composes
        with a single `where`, `where_document` and the dedup and tombstone keep-bitmap (one bitmap per call), and with `reranker` and
        `mmr_lambda`, which consume the candidate list (`n_candidates <= 32`).
        `binary_candidates` (an integer R in [width, 256], the width being what the search returns: `n_candidates` with `reranker`
        or `mmr_lambda`, else `n_results`; None = nothing changes; needs `build_binary` first): the binary-code search
        (INTEGRATION.md "Binary-code search").  Every row is ranked by the Hamming distance between its sign bits and the query's
        (`arx_binary_candidates`), and the first R visible rows by (distance, row) are rescored exactly: the exact top rows among
        those, with the score bits and the order of the exact search, and an added `binary_count` list holds the candidates rescored
        per query.  Composes with a single `where`, `where_document` and the dedup and tombstone keep-bitmap (one bitmap per call),
        and with `reranker` and `mmr_lambda`, which consume the list (`n_candidates <= 32`).
        `boost_weight` (a float, or one per query; None = nothing changes; needs `set_boost` first): the boosted search (INTEGRATION.md
        "Boosted search"): the exact top rows by float32(cosine + float32(weight * prior)) under the one bitmap of `where`,
        `where_document` and the keep-bitmap.  `scores` holds the boosted values, `distances` follow them as they follow the cosine
        otherwise, and an added `base_scores` list holds the cosines of the same rows.  `reranker` and `mmr_lambda` consume the list
        as any other.  A weight that is not finite is a ValueError.
        `pq_candidates` (an integer R in [width, 256], the width as for `binary_candidates`; None = nothing changes; needs `build_pq`
        first): the product-quantised search (INTEGRATION.md "Product-quantised search").  Every row is ranked by the sum of the
        query's byte look-up tables over its PQ code (`arx_pq_candidates`), and the first R visible rows by (sum desc, row) are
        rescored exactly: the exact top rows among those, with the score bits and the order of the exact search, and an added
        `pq_count` list holds the candidates rescored per query.  Composes with a single `where`, `where_document` and the dedup and
        tombstone keep-bitmap (one bitmap per call), and with `reranker` and `mmr_lambda` (`n_candidates <= 32`).
        `graph_ef` (an integer L in [width, 512], the width as for `binary_candidates`; None = nothing changes; needs `build_graph`
        first) with `graph_entries` (E in [1, 32], at most the graph's entry lists): the graph search (INTEGRATION.md "Graph
        search").  Every query walks the k-NN graph from the medoids of its E nearest entry centroids with a beam of L rows
        (`arx_graph_search`), scoring a few thousand rows whatever the collection's size: which rows get visited is the only
        approximation, the scores and the order are the exact search's, and an added `graph_scored` list holds the rows scored per
        query.  Composes with a single `where`, `where_document` and the dedup and tombstone keep-bitmap (one bitmap per call; it
        restricts what comes back, hidden rows stay bridges of the walk), and with `reranker` and `mmr_lambda`
        (`n_candidates <= 32`).  A graph that is stale after `add` or `compact` is a ValueError.
        What each of these five modes cannot be combined with (each other, `hybrid_alpha`, `group_by`, `min_score`, per-query filter
        lists, `world > 1`, a collection without its index) is `modes.MODES`; `modes.check_modes` refuses, with a ValueError naming the
        part, before the queries are encoded or anything is launched."""
        import torch
        from .filter_sets import is_per_query
        from .grouping import check_grouped_query
        from .modes import MODES, check_modes
        from .ranging import RERANK_BATCH, check_range_query
        from .retrieval import check_hybrid_on_device, check_shared_query, retrieve
        per_query = is_per_query(where) or is_per_query(where_document)
        graph, ivf = getattr(self, "graph", None), getattr(self, "ivf", None)
        nq_given = 1
        if boost_weight is not None and query_embeddings is not None:
            nq_given = 1 if np.ndim(query_embeddings) == 1 else len(query_embeddings)
        elif boost_weight is not None and query_texts is not None:
            nq_given = len(query_texts)
        check_modes(                                             # (nprobe: its width is `retrieve`'s to check, which asks all of this again)
            {"graph_ef": graph_ef, "pq_candidates": pq_candidates, "boost_weight": boost_weight, "binary_candidates": binary_candidates,
             "nprobe": nprobe},
            {"graph_ef": dict(has_index=graph is not None, stale=getattr(graph, "stale", False), n_entries=graph_entries,
                              n_entry_lists=getattr(graph, "n_entry_lists", 0), degree=getattr(graph, "degree", 32)),
             "pq_candidates": dict(has_index=getattr(self, "pq", None) is not None),
             "boost_weight": dict(has_index=self._prior() is not None, n_queries=nq_given, max_abs_prior=getattr(self, "_boost_max", 0.0)),
             "binary_candidates": dict(has_index=getattr(self, "binary", None) is not None),
             "nprobe": dict(has_index=ivf is not None, n_lists=getattr(ivf, "n_lists", 0), n_width=1)},
            per_query=per_query, hybrid_alpha=hybrid_alpha, group_by=group_by, min_score=min_score, world=getattr(self, "world", 1),
            n_width=n_candidates if (reranker is not None or mmr_lambda is not None) else n_results)
        on_device = hybrid_alpha is not None and getattr(self, "hybrid_on_device", False)
        check_range_query(n_results, ranged=min_score is not None, reranker=reranker, n_candidates=n_candidates, hybrid_alpha=hybrid_alpha,
                          mmr_lambda=mmr_lambda, group_by=group_by, per_query_filters=per_query, world=getattr(self, "world", 1))
        check_grouped_query(n_results, chunks_per_group, grouped=bool(group_by), has_group_key=getattr(self, "group_key", None) is not None,
                            reranker=reranker, hybrid_alpha=hybrid_alpha, mmr_lambda=mmr_lambda, per_query_filters=per_query,
                            world=getattr(self, "world", 1))
        check_shared_query(
            n_results, hybrid_alpha=hybrid_alpha, hybrid_filters=getattr(self, "hybrid_filters", False), reranker=reranker,
            mmr_lambda=mmr_lambda, n_fetch=n_candidates,
            fetch_refusal=f"n_candidates={n_candidates} must be in [n_results, 32] (the search's k limit) and n_results at least 1",
            filters_first=(("where cannot be combined", per_query),           # (a per-query list of either argument is refused as `where`)
                           ("a collection built with dedup_threshold cannot be queried" if getattr(self, "_deleted", None) is None
                            else "a collection with deleted rows cannot be queried", self._keep is not None)),
            filters=(("where_document cannot be combined", where_document is not None and not per_query),
                     ("where cannot be combined", where is not None and not per_query)))
        if where_document is not None and not per_query:         # (refused here, before the queries are encoded)
            from .where_document import compile_where_document
            self._documents()
            compile_where_document(where_document, regex=getattr(self, "document_regex", False))
        if hybrid_alpha is not None:
            if not (0.0 <= float(hybrid_alpha) <= 1.0):
                raise ValueError(f"hybrid_alpha={hybrid_alpha} must be in [0, 1]")
            if query_texts is None or self.keyword is None:
                raise ValueError("hybrid search needs query_texts and a collection built with keyword=True")
            if getattr(self, "_kw_stale", False):                # rows were added or compacted away since the index was built
                self._rebuild_keyword()
            if on_device:
                check_hybrid_on_device(n_candidates, per_query_filters=per_query, world=getattr(self, "world", 1))
            if not (n_results <= n_candidates <= (1024 if on_device else 32)):
                raise ValueError(f"n_candidates={n_candidates} must be in [n_results, {1024 if on_device else 32}] (the candidate lists' length limit)")
        if reranker is not None:
            if query_texts is None:
                raise ValueError("reranking needs query_texts")
            if min_score is None and not on_device and not (n_results <= n_candidates <= 32):
                raise ValueError(f"n_candidates={n_candidates} must be in [n_results, 32] (the search's k limit)")
        if query_embeddings is None:
            if query_texts is None or self.encoder is None:
                raise ValueError("pass query_embeddings, or query_texts with an encoder")
            query_embeddings = self.encoder.encode(list(query_texts), normalize_embeddings=True, convert_to_numpy=True, low_latency=True)
        q = torch.from_numpy(np.ascontiguousarray(query_embeddings, dtype=np.float16)).to(self.index.corpus.device)
        if q.dim() == 1:
            q = q[None]
        hit = retrieve(self.index, q, self._row_filters(), n_results, n_candidates=n_candidates, reranked=reranker is not None, where=where,
                       where_document=where_document, min_score=min_score, grouped=bool(group_by), chunks_per_group=chunks_per_group,
                       mmr_lambda=mmr_lambda, hybrid_alpha=hybrid_alpha, keyword=self.keyword, query_texts=query_texts,
                       hybrid_on_device=on_device, world=getattr(self, "world", 1),
                       **({} if nprobe is None else {"nprobe": nprobe, "ivf": self.ivf}),
                       **({} if binary_candidates is None else {"binary_candidates": binary_candidates, "binary": self.binary}),
                       **({} if pq_candidates is None else {"pq_candidates": pq_candidates, "pq": self.pq}),
                       **({} if graph_ef is None else {"graph_ef": graph_ef, "graph": self.graph, "graph_entries": graph_entries}),
                       **({} if boost_weight is None else {"boost_weight": boost_weight, "prior": self._prior(), "max_abs_prior": self._boost_max}))
        s, i, hyb, kws, base = hit.scores, hit.ids, hit.hybrid, hit.keyword, hit.base
        if reranker is not None:
            from .rerank import rerank_candidates, reorder_by_rerank
            texts = {int(j): self.metadata[int(j)].get("text") or "" for j in np.unique(i) if j >= 0}
            sc = rerank_candidates(lambda pairs: reranker.predict(pairs, batch_size=n_candidates if min_score is None and not on_device else min(n_candidates, RERANK_BATCH),
                                                                convert_to_numpy=True),
                                   list(query_texts), i, texts)
            picked = reorder_by_rerank(i, sc, n_results)
            width = max([len(p) for p in picked] + [1])
            s2 = np.full((len(picked), width), -np.inf, np.float32); i2 = np.full((len(picked), width), -1, np.int64)
            if base is not None:
                base = np.array([[base[qi, p[r][0]] if r < len(p) else -np.inf for r in range(width)] for qi, p in enumerate(picked)], np.float32)
            rr = [[h[2] for h in p] for p in picked]
            for qi, p in enumerate(picked):
                for r, (pos, j, _) in enumerate(p):
                    s2[qi, r], i2[qi, r] = s[qi, pos], j
            if hyb is not None:
                hyb = np.array([[hyb[qi, p[r][0]] if r < len(p) else -np.inf for r in range(width)] for qi, p in enumerate(picked)])
                kws = np.array([[kws[qi, p[r][0]] if r < len(p) else np.nan for r in range(width)] for qi, p in enumerate(picked)])
            s, i = s2, i2
        out = {"ids": [], "distances": [], "scores": [], "documents": [], "metadatas": [], "indices": []}
        for qi in range(q.shape[0]):
            keep = i[qi] >= 0
            rows = i[qi][keep].tolist()
            ms = [self.metadata[r] for r in rows]
            out["indices"].append(rows)
            out["ids"].append([m.get("chunk_id", f"chunk_{r}") for m, r in zip(ms, rows)])
            out["scores"].append(s[qi][keep].tolist())
            out["distances"].append((2.0 - 2.0 * s[qi][keep]).tolist())
            out["documents"].append([m.get("text") for m in ms])
            out["metadatas"].append([{k: m.get(k) for k in ("paper_id", "section", "quality_score")} for m in ms])
        if hit.groups is not None:
            out["group_keys"] = [[self.group_keys[int(v)] for v in hit.groups[qi] if v >= 0] for qi in range(q.shape[0])]
            out["group_sizes"] = [[int(n) for n, v in zip(hit.group_sizes[qi], hit.groups[qi]) if v >= 0] for qi in range(q.shape[0])]
        if hit.truncated is not None:
            out["truncated"] = hit.truncated
        for counter in (m.counter for m in MODES.values() if m.counter is not None):      # the rows the mode that ran scored, per query
            if getattr(hit, counter) is not None:
                out[counter] = [int(v) for v in getattr(hit, counter)]
        if base is not None:
            out["base_scores"] = [base[qi][i[qi] >= 0].tolist() for qi in range(q.shape[0])]
        if hit.mmr is not None:
            out["mmr_scores"] = [hit.mmr[qi][i[qi] >= 0].tolist() for qi in range(q.shape[0])]
        if reranker is not None:
            out["rerank_scores"] = rr
        if hyb is not None:
            out["hybrid_scores"] = [hyb[qi][i[qi] >= 0].tolist() for qi in range(q.shape[0])]
            out["keyword_scores"] = [kws[qi][i[qi] >= 0].tolist() for qi in range(q.shape[0])]
        return out
