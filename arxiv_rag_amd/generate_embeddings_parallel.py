#!/usr/bin/env python3
"""Drop-in for stage 4 of arxiv-rag: `4-embed/generation/generate_embeddings_parallel.py` ("GEN").

Same positional argument, flags and defaults (GEN:471-491), same exit codes (GEN:497-499, 527-529, 603-609),
same `./embeddings_saved/{embeddings.npy, metadata.json, index.json}` layout (GEN:271-321), same
never-raise-per-chunk policy (GEN:155-177).  What changes is underneath: one process per MI355X
(`torchrun --nproc-per-node N`), each rank encodes a contiguous shard of the chunk list through the HIP
encoder and keeps its rows in HBM as its fp16 corpus shard; an optional `--queries` step then serves
brute-force cosine top-k over the shards (RCCL all-gather of partial top-k).

Additive flags only: --model also takes a local directory; --model-dir, --out-dtype, --queries, --top-k,
--skip-chroma.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import sys
import threading
import time
import traceback
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

MODEL_CHOICES = ["all-mpnet-base-v2", "all-MiniLM-L6-v2"]          # GEN:474

_model = None
_model_name = None


# --------------------------------------------------------------------------------------------- model
def init_worker_model(model_name: str, factory: Optional[Callable] = None):
    """Per-process singleton (GEN:40-65): here one process owns one GPU."""
    global _model, _model_name
    if _model is None or _model_name != model_name:
        if factory is None:
            from .hub import load_sentence_encoder
            dev = f"cuda:{os.environ.get('LOCAL_RANK', '0')}"
            factory = lambda name: load_sentence_encoder(name, device=dev)     # noqa: E731
        print(f"[rank {os.environ.get('RANK', '0')}] Loading model: {model_name}")
        _model = factory(model_name)
        _model_name = model_name
        print(f"[rank {os.environ.get('RANK', '0')}] Model loaded successfully")
    return _model


def get_worker_model(model_name: str):
    """GEN:67-74."""
    return init_worker_model(model_name)


# --------------------------------------------------------------------------------------------- load
def load_chunks_from_file(file_path: Path, min_quality: float = 0.8) -> List[Dict]:
    """One chunk-JSON file -> its chunks with metadata.quality_score >= min_quality (missing = 0);
    unreadable files contribute nothing (GEN:76-92)."""
    kept: List[Dict] = []
    try:
        with open(file_path, "r", encoding="utf-8") as fh:
            doc = json.load(fh)
        for ch in doc.get("chunks", []):
            if ch.get("metadata", {}).get("quality_score", 0) >= min_quality:
                kept.append(ch)
    except Exception:
        pass
    return kept


def _load_many(args: Tuple[List[str], float]) -> List[Dict]:
    paths, min_quality = args
    out: List[Dict] = []
    for p in paths:
        out.extend(load_chunks_from_file(Path(p), min_quality))
    return out


PROCESS_POOL_MIN_FILES = 4096      # below this a spawn pool's start-up (~0.2 s per worker) costs more than it saves


def effective_cpus() -> int:
    """CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota.  `mp.cpu_count()` reports every
    logical CPU of the machine (256 on a GPU box whose one-GPU job is granted 16): pools sized from it oversubscribe the quota 16x."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per) + 0.5)))
    except Exception:
        try:
            q = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read_text())
            per = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read_text())
            if q > 0:
                n = min(n, max(1, int(q / per + 0.5)))
        except Exception:
            pass
    return max(1, n)


def default_load_workers() -> int:
    """GEN:103 (`int(cpu_count * 0.8)`) on the CPUs this process may use, shared among the ranks of this node."""
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    return max(1, int(effective_cpus() * 0.8) // local_world)


def list_chunk_files(output_dir: Path) -> List[Path]:
    """All `*.json` under the tree except `._*` (GEN:97-98), SORTED: the order every rank agrees on."""
    return sorted(f for f in Path(output_dir).rglob("*.json") if not f.name.startswith("._"))


def load_chunk_files(files: Sequence[Path], min_quality: float = 0.8, num_workers: Optional[int] = None) -> List[List[Dict]]:
    """The kept chunks of each file, one list per file, in the order given.  `json.load` holds the GIL, so a corpus-sized list
    (GEN:103 sizes its pool for 70 k files) is parsed by a process pool — `spawn` context, as GEN:611-616 sets, which is also the
    only start method that is safe once the process has touched the GPU — fed contiguous slices through ordered `imap`; small
    lists are read by a thread pool in-process."""
    if num_workers is None:
        num_workers = default_load_workers()
    per_file: List[List[Dict]] = []
    if len(files) >= PROCESS_POOL_MIN_FILES and num_workers > 1:
        nproc = min(num_workers, 64, max(2, len(files) // 1024))
        step = 128
        jobs = [([str(f) for f in files[i:i + step]], min_quality) for i in range(0, len(files), step)]
        with mp.get_context("spawn").Pool(nproc) as pool:
            for part in pool.imap(_load_many_per_file, jobs, chunksize=1):
                per_file.extend(part)
    else:
        with ThreadPoolExecutor(max_workers=max(1, min(num_workers, 64))) as ex:
            per_file.extend(ex.map(lambda f: load_chunks_from_file(f, min_quality), files))
    return per_file


def _load_many_per_file(args: Tuple[List[str], float]) -> List[List[Dict]]:
    paths, min_quality = args
    return [load_chunks_from_file(Path(p), min_quality) for p in paths]


def load_chunks_parallel(output_dir: Path, min_quality: float = 0.8, num_workers: Optional[int] = None) -> List[Dict]:
    """All `*.json` under the tree except `._*` (GEN:94-129).  Files are visited in SORTED order and results concatenated in that
    order: the reference's imap_unordered order is not a contract, and a deterministic order is what lets N ranks agree on the
    shard boundaries."""
    files = list_chunk_files(output_dir)
    if num_workers is None:
        num_workers = default_load_workers()
    print(f"Loading chunks from {len(files):,} files using {num_workers} workers...")
    out: List[Dict] = []
    for part in load_chunk_files(files, min_quality, num_workers):
        if part:
            out.extend(part)
    print(f"Loaded {len(out):,} high-quality chunks (quality >= {min_quality})")
    return out


class RankChunks:
    """What ONE rank of an N-rank run holds of the corpus: the chunks of global rows [lo, hi) (its contiguous range of work quanta),
    `total` = the corpus' chunk count.  Built by `load_chunks_for_rank`: the tree is parsed ONCE across the ranks, not once per rank."""

    def __init__(self, chunks: List[Dict], lo: int, hi: int, total: int, files_total: int, files_parsed: int):
        self.chunks, self.lo, self.hi, self.total = chunks, lo, hi, total
        self.files_total, self.files_parsed = files_total, files_parsed


def load_chunks_for_rank(output_dir: Path, min_quality: float, num_workers: Optional[int], chunks_per_worker: int,
                         world: int, rank: int, gather_counts: Optional[Callable] = None) -> RankChunks:
    """Per-rank loading (the reference loads the tree once, with one pool: GEN:94-129; N ranks each loading ALL of it would be N
    parses and N copies of every chunk's text).  Rank r parses only its contiguous slice of the SORTED file list; an
    `all_gather_object` of the per-file kept-chunk counts gives every rank the global row offset of every file (the order contract —
    sorted files, chunks in file order — is unchanged); the rank's row range stays the range of work quanta the sharded dispatcher
    assigns (`shard_range` over `ceil(total / chunks_per_worker)` quanta, so every quantum is the same set of chunks as in a
    one-rank run), and the few files of a neighbouring slice that reach into that range are parsed here as well."""
    files = list_chunk_files(output_dir)
    f_lo, f_hi = shard_range(len(files), world, rank)
    if num_workers is None:
        num_workers = default_load_workers()
    print(f"[rank {rank}] Loading chunks from files [{f_lo:,}, {f_hi:,}) of {len(files):,} using {num_workers} workers...")
    mine = load_chunk_files(files[f_lo:f_hi], min_quality, num_workers)
    counts_local = [len(c) for c in mine]
    if gather_counts is None:
        import torch.distributed as dist
        def gather_counts(x):                                          # noqa: E306
            out: List = [None] * world
            dist.all_gather_object(out, x, group=host_group())
            return out
    counts: List[int] = [n for part in gather_counts(counts_local) for n in part]
    assert len(counts) == len(files), "ranks disagree on the file list"
    offsets = np.zeros(len(files) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    n_quanta = (total + chunks_per_worker - 1) // chunks_per_worker
    q_lo, q_hi = shard_range(n_quanta, world, rank)
    lo, hi = min(total, q_lo * chunks_per_worker), min(total, q_hi * chunks_per_worker)
    chunks: List[Dict] = []
    extra = 0
    if hi > lo:
        fa = int(np.searchsorted(offsets, lo, side="right")) - 1       # first file holding row lo
        fb = int(np.searchsorted(offsets, hi, side="left"))            # one past the last file holding row hi - 1
        need = [i for i in range(fa, fb) if counts[i] > 0]
        outside = [i for i in need if not (f_lo <= i < f_hi)]
        extra = len(outside)
        fetched = dict(zip(outside, load_chunk_files([files[i] for i in outside], min_quality, num_workers))) if outside else {}
        for i in need:
            part = mine[i - f_lo] if f_lo <= i < f_hi else fetched[i]
            a, b = max(lo, int(offsets[i])) - int(offsets[i]), min(hi, int(offsets[i + 1])) - int(offsets[i])
            chunks.extend(part[a:b])
    assert len(chunks) == hi - lo, (len(chunks), lo, hi)
    print(f"[rank {rank}] parsed {f_hi - f_lo + extra} of {len(files)} files (own slice [{f_lo}, {f_hi}) + {extra} boundary files); "
          f"holds chunks [{lo:,}, {hi:,}) of {total:,} (quality >= {min_quality})")
    return RankChunks(chunks, lo, hi, total, len(files), f_hi - f_lo + extra)


# --------------------------------------------------------------------------------------------- embed
def generate_embeddings_worker(args: Tuple[List[str], str, int, int]) -> Tuple[int, List[np.ndarray], Optional[str]]:
    """One work quantum (<= chunks_per_worker texts): sub-batches of batch_size through model.encode;
    a failed sub-batch is retried per text, a failed text becomes a zero row; never raises (GEN:131-177)."""
    texts, model_name, batch_size, batch_idx = args
    try:
        model = get_worker_model(model_name)
        if model is None:
            return (batch_idx, [], "model not loaded")
        rows: List[np.ndarray] = []
        for s0 in range(0, len(texts), batch_size):
            sub = texts[s0:s0 + batch_size]
            try:
                rows.extend(model.encode(sub, batch_size=min(batch_size, len(sub)), normalize_embeddings=True,
                                         show_progress_bar=False, convert_to_numpy=True, convert_to_tensor=False))
            except Exception:
                print(f"[rank {os.environ.get('RANK', '0')}] sub-batch {s0 // batch_size} of quantum {batch_idx} failed, trying individual items")
                for t in sub:
                    try:
                        rows.extend(model.encode([t], normalize_embeddings=True, show_progress_bar=False, convert_to_numpy=True))
                    except Exception:
                        rows.append(np.zeros(model.get_sentence_embedding_dimension()))
        return (batch_idx, rows, None)
    except Exception as e:                                                   # noqa: BLE001
        msg = f"Error in rank {os.environ.get('RANK', '0')}: {e}"
        print(msg)
        traceback.print_exc()
        return (batch_idx, [], msg)


class ShardSink:
    """This rank's fp16 corpus shard, resident in HBM: rows [lo, hi) of the corpus, filled by the encoder kernels while the
    chunks are being embedded (`encode(..., device_f16_out=...)`) and searched where they lie — corpus rows never cross PCIe
    towards the device.  Only rows that came out of the reference's fallback policy (per-item retry / zero rows, GEN:155-169;
    host arrays by construction) are uploaded, a quantum at a time."""

    def __init__(self, model, lo: int, hi: int):
        import torch
        self.lo, self.hi = lo, hi
        self.rows = torch.zeros((hi - lo, model.get_sentence_embedding_dimension()), dtype=torch.float16,
                                device=model.encoder.device)

    def view(self, a: int, b: int):
        return self.rows[a - self.lo:b - self.lo]

    def put(self, a: int, rows: Sequence[np.ndarray]):
        import torch
        if len(rows):
            host = np.asarray(rows, dtype=np.float32).astype(np.float16)
            self.rows[a - self.lo:a - self.lo + len(rows)] = torch.from_numpy(host).to(self.rows.device)


def make_shard_sink(model, n_texts: int, chunks_per_worker: int, world: int, rank: int) -> Optional["ShardSink"]:
    """A sink for the row range this rank encodes (same split as the dispatchers below); None for a model with no device."""
    if getattr(model, "encoder", None) is None or not hasattr(model.encoder, "device"):
        return None
    n_quanta = (n_texts + chunks_per_worker - 1) // chunks_per_worker
    q_lo, q_hi = (0, n_quanta) if world == 1 else shard_range(n_quanta, world, rank)
    return ShardSink(model, min(n_texts, q_lo * chunks_per_worker), min(n_texts, q_hi * chunks_per_worker))


def _encode_quanta(texts: List[str], q_lo: int, q_hi: int, model_name: str, batch_size: int, chunks_per_worker: int,
                   super_quanta: int = 32, sink: Optional[ShardSink] = None, base: int = 0, total: Optional[int] = None):
    """Quanta [q_lo, q_hi) -> yields (qi, rows, err) exactly as `generate_embeddings_worker` would, but fast: a HIP sentence
    encoder gets `super_quanta` quanta per `encode()` call (rows do not depend on how texts are batched, so the result is the same;
    the tokenizer feeder and the 1024-sequence forwards then run at the device-bound rate instead of 200 texts at a time).  Any
    exception or row-count mismatch in a fast call falls back to the per-quantum worker, i.e. to the reference's policy
    (sub-batch retry, per-item retry, zero rows; GEN:131-177).  `texts` holds global rows [base, base + len(texts)) of a corpus of
    `total` chunks (per-rank loading); quanta are numbered globally."""
    total = len(texts) if total is None else total
    model = None
    try:
        model = get_worker_model(model_name)
    except Exception:
        model = None
    fast = model is not None and getattr(model, "coalesce_batches", False)
    qi = q_lo
    while qi < q_hi:
        qe = min(q_hi, qi + (super_quanta if fast else 1))
        a, b = qi * chunks_per_worker, min(total, qe * chunks_per_worker)
        rows = None
        if fast:
            try:
                extra = {"device_f16_out": sink.view(a, b)} if sink is not None else {}
                rows = model.encode(texts[a - base:b - base], batch_size=batch_size, normalize_embeddings=True, show_progress_bar=False,
                                    convert_to_numpy=True, convert_to_tensor=False, **extra)
                if len(rows) != b - a:
                    rows = None
            except Exception:
                rows = None
        for q in range(qi, qe):
            qa, qb = q * chunks_per_worker, min(total, (q + 1) * chunks_per_worker)
            if rows is not None:
                yield (q, list(rows[qa - a:qb - a]), None)
            else:
                res = generate_embeddings_worker((texts[qa - base:qb - base], model_name, batch_size, q))
                if sink is not None:                     # fallback rows are host arrays: this quantum's shard rows are replaced
                    try:
                        sink.view(qa, qb).zero_()
                        sink.put(qa, res[1][:qb - qa])
                    except Exception:                    # noqa: BLE001  (never raise per chunk; the rows stay zero)
                        pass
                yield res
        qi = qe


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


_host_pg = None


def init_distributed():
    """Bring up this rank's process group (one process per GPU; the reference's counterpart is the `mp.Pool` of GEN:197-217).
    The device is BOUND before the group exists: RCCL stages object collectives on `torch.cuda.current_device()`, which is cuda:0 in
    every rank until someone says otherwise — the first collective of the run (`load_chunks_for_rank`'s count exchange) runs before
    the model is loaded, and a communicator built with every rank on GPU 0 fails with "Duplicate GPU detected" or hangs
    (ADVICE r3).  `device_id` also makes the communicator eager, so a mis-launch fails here and not in the middle of the load."""
    import torch
    import torch.distributed as dist
    if dist.is_initialized():
        return
    if torch.cuda.is_available():
        local_rank = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
        n_dev = torch.cuda.device_count()
        if local_rank >= n_dev:
            raise RuntimeError(f"LOCAL_RANK={local_rank} but only {n_dev} GPU(s) visible: launch one rank per GPU")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group("gloo")


def host_group():
    """Process group for the HOST-side object exchanges of an N-rank run (per-file chunk counts, metadata bookkeeping, chunk ids of
    merged hits): gloo over TCP, so that pickled Python objects never pass through device memory and the loader does not depend on
    the GPU at all.  The default group itself when that already is gloo (CPU runs / tests)."""
    global _host_pg
    import torch.distributed as dist
    if dist.get_backend() == "gloo":
        return None
    if _host_pg is None:
        _host_pg = dist.new_group(backend="gloo")
    return _host_pg


def shard_range(n_items: int, world: int, rank: int) -> Tuple[int, int]:
    per = (n_items + world - 1) // world
    lo = min(n_items, rank * per)
    return lo, min(n_items, lo + per)


def generate_embeddings_parallel(chunks: List[Dict], model_name: str = "all-mpnet-base-v2", batch_size: int = 200,
                                 num_workers: Optional[int] = None, chunks_per_worker: int = 500,
                                 sink: Optional[ShardSink] = None) -> List[np.ndarray]:
    """Embedding i <-> chunk i (GEN:179-269).  Quanta of chunks_per_worker texts; with torchrun each rank takes
    a contiguous range of quanta and the per-rank results are exchanged so every rank returns all N rows
    (missing quanta -> zero rows, count mismatch -> pad/truncate, as GEN:260-267)."""
    texts = [c["text"] for c in chunks]
    dist = _dist()
    world = dist.get_world_size() if dist else 1
    rank = dist.get_rank() if dist else 0
    quanta = [(texts[i:i + chunks_per_worker], model_name, batch_size, qi)
              for qi, i in enumerate(range(0, len(texts), chunks_per_worker))]
    print(f"Generating embeddings for {len(texts):,} chunks on {world} GPU(s)...")
    print(f"Model: {model_name}, Batch size: {batch_size}, Chunks per worker: {chunks_per_worker}")
    q_lo, q_hi = shard_range(len(quanta), world, rank)
    done: Dict[int, List[np.ndarray]] = {}
    errors: List[str] = []
    for idx, rows, err in _encode_quanta(texts, q_lo, q_hi, model_name, batch_size, chunks_per_worker, sink=sink):
        if err:
            errors.append(f"Batch {idx}: {err}")
        if rows:
            done[idx] = rows
        else:
            print(f"Warning: Batch {idx} produced no embeddings")
    if dist and world > 1:
        gathered: List = [None] * world
        dist.all_gather_object(gathered, (done, errors), group=host_group())
        done, errors = {}, []
        for d, e in gathered:
            done.update(d); errors.extend(e)
    if errors:
        print(f"\n⚠️  {len(errors)} batches had errors:")
        for e in errors[:10]:
            print(f"  - {e}")
    embeddings: List[np.ndarray] = []
    missing = 0
    for qi in range(len(quanta)):
        rows = done.get(qi)
        if rows is not None:
            embeddings.extend(rows)
        else:
            missing += 1
    if missing:
        print(f"⚠️  {missing} batches missing, used zero vectors as fallback")
    print(f"Generated {len(embeddings):,} embeddings")
    if len(embeddings) != len(texts):
        print(f"⚠️  Warning: Embedding count ({len(embeddings)}) doesn't match text count ({len(texts)})")
        if len(embeddings) < len(texts):
            dim = len(embeddings[0]) if embeddings else 768
            embeddings.extend([np.zeros(dim)] * (len(texts) - len(embeddings)))
        else:
            embeddings = embeddings[:len(texts)]
    return embeddings


def generate_embeddings_sharded(chunks: List[Dict], model_name: str, batch_size: int = 200,
                                chunks_per_worker: int = 500, sink: Optional[ShardSink] = None,
                                span: Optional[Tuple[int, int, int]] = None) -> Tuple[np.ndarray, int, int]:
    """Multi-rank form of the dispatcher: this rank encodes a contiguous range of quanta and KEEPS its rows
    (no exchange of embeddings: at ~5 M chunks x 768 that would be 15 GB per rank for nothing).
    Returns (rows float32 [hi-lo, D], lo, hi) with row j <-> chunk lo + j; failed quanta are zero rows.
    `span = (lo, hi, total)`: `chunks` are only this rank's chunks, global rows [lo, hi) of `total` (`load_chunks_for_rank`);
    without it `chunks` is the whole corpus."""
    texts = [c["text"] for c in chunks]
    dist = _dist()
    world = dist.get_world_size() if dist else 1
    rank = dist.get_rank() if dist else 0
    total = len(texts) if span is None else span[2]
    base = 0 if span is None else span[0]
    n_quanta = (total + chunks_per_worker - 1) // chunks_per_worker
    q_lo, q_hi = shard_range(n_quanta, world, rank)
    lo, hi = min(total, q_lo * chunks_per_worker), min(total, q_hi * chunks_per_worker)
    assert span is None or (span[0], span[1]) == (lo, hi), "the rank's chunks are not the rows its quanta cover"
    print(f"[rank {rank}] encoding chunks [{lo:,}, {hi:,}) of {total:,} ({q_hi - q_lo} quanta)")
    dim = get_worker_model(model_name).get_sentence_embedding_dimension()
    rows = np.zeros((hi - lo, dim), np.float32)
    errors = 0
    for idx, got, err in _encode_quanta(texts, q_lo, q_hi, model_name, batch_size, chunks_per_worker, sink=sink, base=base, total=total):
        a, b = idx * chunks_per_worker, min(total, (idx + 1) * chunks_per_worker)
        if err or len(got) != b - a:
            errors += 1
            print(f"Warning: Batch {idx} produced {len(got)} of {b - a} embeddings; missing rows stay zero")
        for j, e in enumerate(got[:b - a]):
            rows[a - lo + j] = e
    if errors:
        print(f"⚠️  [rank {rank}] {errors} batches had errors")
    return rows, lo, hi


def save_embeddings_sharded(chunks: List[Dict], rows: np.ndarray, lo: int, hi: int,
                            output_dir: str = "./embeddings_saved", out_dtype: str = "float64", prefetch=None,
                            total: Optional[int] = None):
    """Same three files as save_embeddings_to_disk_fallback, written cooperatively: rank 0 creates embeddings.npy
    (header + size), every rank stores its own row range through a memmap, rank 0 writes metadata/index.
    `total` given: `chunks` are only this rank's chunks (rows [lo, hi) of `total`); every rank then serialises ITS entries of
    metadata.json into a fragment file (beside the GPU work, when a `MetadataPrefetch` was started for it) and rank 0 joins the
    fragments in rank order — the same bytes `_dump_metadata` writes for the whole list."""
    dist = _dist()
    rank = dist.get_rank() if dist else 0
    world = dist.get_world_size() if dist else 1
    out = Path(output_dir)
    n, dim = (len(chunks) if total is None else total), rows.shape[1]
    if rank == 0:
        out.mkdir(parents=True, exist_ok=True)
        arr = np.lib.format.open_memmap(out / "embeddings.npy", mode="w+", dtype=np.dtype(out_dtype), shape=(n, dim))
        del arr
    if dist:
        dist.barrier()
    arr = np.load(out / "embeddings.npy", mmap_mode="r+")
    arr[lo:hi] = rows.astype(np.dtype(out_dtype))
    nbytes = arr.nbytes
    arr.flush()
    del arr
    if total is not None:                                   # this rank's entries of metadata.json
        frag = out / f"metadata.json.part{rank}"
        if prefetch is None or not prefetch.take(chunks, frag):
            _dump_metadata(chunks, frag, first_index=lo, fragment=True)
    if dist:
        dist.barrier()
    if rank == 0:
        if total is None:
            _write_metadata_and_index(chunks, out, n, dim, nbytes, prefetch)
        else:
            _join_metadata_fragments(out, world)
            print(f"✅ Saved metadata to {out / 'metadata.json'}")
            _write_index(out, n, dim, nbytes)
        print(f"✅ Saved {n:,} embeddings ({dim} dimensions) from {world} rank(s)")


def _join_metadata_fragments(out: Path, world: int):
    """metadata.json = "[\n" + the ranks' entry runs joined by ",\n" + "\n]" (what `_dump_metadata` writes for the whole list)."""
    with open(out / "metadata.json", "wb") as fh:
        first = True
        for r in range(world):
            frag = out / f"metadata.json.part{r}"
            if frag.stat().st_size:
                fh.write(b"[\n" if first else b",\n")
                first = False
                with open(frag, "rb") as src:
                    while True:
                        buf = src.read(1 << 24)
                        if not buf:
                            break
                        fh.write(buf)
            frag.unlink()
        fh.write(b"[]" if first else b"\n]")


# --------------------------------------------------------------------------------------------- write
def save_embeddings_to_disk_fallback(chunks: List[Dict], embeddings: Sequence, output_dir: str = "./embeddings_saved",
                                     out_dtype: str = "float64", prefetch=None):
    """embeddings.npy (float64 C-order [N, D] — the reference's `.tolist()` round trip yields float64),
    metadata.json (indent=2, ensure_ascii=False), index.json (GEN:271-321).  Streams through a memmap so a
    5 M x 768 corpus (30.7 GB) never needs a second in-RAM copy."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    print(f"\nSaving embeddings to disk: {output_dir}")
    n = len(embeddings)
    dim = len(embeddings[0]) if n else 0
    arr = np.lib.format.open_memmap(out / "embeddings.npy", mode="w+", dtype=np.dtype(out_dtype), shape=(n, dim))
    step = 65536
    for s0 in range(0, n, step):
        arr[s0:s0 + step] = np.asarray(embeddings[s0:s0 + step], dtype=np.dtype(out_dtype))
    nbytes = arr.nbytes
    arr.flush()
    del arr
    print(f"✅ Saved embeddings to {out / 'embeddings.npy'}")
    _write_metadata_and_index(chunks, out, n, dim, nbytes, prefetch)
    print(f"✅ Saved {n:,} embeddings ({dim} dimensions)")
    print(f"   Total size: ~{nbytes / 1024 / 1024 / 1024:.2f} GB")


def _dump_metadata(chunks: List[Dict], path: Path, first_index: int = 0, fragment: bool = False):
    """metadata.json, byte for byte what `json.dump(metadata, f, indent=2, ensure_ascii=False)` writes at GEN:292-306, but
    streamed one chunk at a time: the reference builds the whole list and its serialisation in RAM (the text of ~5 M chunks
    twice over); here the peak is one entry.  `fragment`: only the entries (joined by ",\n", no brackets) of chunks that are
    rows first_index.. of the corpus — one rank's part of the file (`_join_metadata_fragments`)."""
    with open(path, "w", encoding="utf-8") as fh:
        if not chunks:
            fh.write("" if fragment else "[]")
            return
        if not fragment:
            fh.write("[\n")
        for i, ch in enumerate(chunks):
            m = ch.get("metadata", {})
            item = {"chunk_id": ch.get("chunk_id", f"chunk_{first_index + i}"), "paper_id": m.get("paper_id"),
                    "section": m.get("section"), "quality_score": m.get("quality_score"),
                    "text": ch["text"], "text_length": len(ch["text"])}
            body = json.dumps(item, indent=2, ensure_ascii=False)
            fh.write("  " + body.replace("\n", "\n  "))
            if i + 1 < len(chunks):
                fh.write(",\n")
            elif not fragment:
                fh.write("\n")
        if not fragment:
            fh.write("]")


class MetadataPrefetch(threading.Thread):
    """metadata.json depends on the chunk list only, so its (pure-Python, ~17 us per chunk) serialisation runs beside the
    GPU while the embeddings are being generated, into `<out>/metadata.json.partial`; the writer renames it into place at
    the point where the reference writes the file (GEN:300-311), or discards it when the run does not get that far."""

    def __init__(self, chunks: List[Dict], output_dir: str = "./embeddings_saved", first_index: int = 0,
                 fragment_of_rank: Optional[int] = None):
        super().__init__(daemon=True)
        self.chunks, self.out, self.ok = chunks, Path(output_dir), False
        self.first_index, self.fragment = first_index, fragment_of_rank is not None
        self.partial = self.out / ("metadata.json.partial" if fragment_of_rank is None else f"metadata.json.partial{fragment_of_rank}")

    def run(self):
        try:
            self.out.mkdir(parents=True, exist_ok=True)
            _dump_metadata(self.chunks, self.partial, first_index=self.first_index, fragment=self.fragment)
            self.ok = True
        except Exception:                                              # noqa: BLE001  (the writer then serialises itself)
            self.ok = False

    def take(self, chunks: List[Dict], dest: Path) -> bool:
        self.join()
        if self.ok and chunks is self.chunks and self.partial.exists() and dest.parent.resolve() == self.out.resolve():
            os.replace(self.partial, dest)
            return True
        self.discard()
        return False

    def discard(self):
        self.join()
        try:
            self.partial.unlink()
        except OSError:
            pass


def _write_metadata_and_index(chunks: List[Dict], out: Path, n: int, dim: int, nbytes: int, prefetch: Optional["MetadataPrefetch"] = None):
    if prefetch is None or not prefetch.take(chunks, out / "metadata.json"):
        _dump_metadata(chunks, out / "metadata.json")
    print(f"✅ Saved metadata to {out / 'metadata.json'}")
    _write_index(out, n, dim, nbytes)


def _write_index(out: Path, n: int, dim: int, nbytes: int):
    index = {"total_embeddings": n, "embedding_dimension": dim, "total_size_gb": nbytes / 1024 / 1024 / 1024}
    with open(out / "index.json", "w", encoding="utf-8") as fh:
        json.dump(index, fh, indent=2)


def store_in_chroma_batched(chunks: List[Dict], embeddings: Sequence, db_path: str = "./chroma_db",
                            collection_name: str = "scientific_papers", batch_size: int = 2000):
    """Vector-store hand-off (GEN:323-468): ids / documents / metadatas exactly as GEN:404-412, batches of
    `batch_size`, 3 tries per batch then per-item adds.  Raises ImportError when chromadb is absent."""
    import chromadb                                                    # noqa: F401  (lazy: optional dependency)
    n = min(len(chunks), len(embeddings))
    client = chromadb.PersistentClient(path=db_path)
    try:
        coll = client.get_collection(name=collection_name)
    except Exception:
        coll = client.create_collection(name=collection_name, metadata={"description": "Scientific paper chunks for RAG"})
    stored = 0
    for s0 in range(0, n, batch_size):
        ids, embs, docs, metas = [], [], [], []
        for j in range(s0, min(n, s0 + batch_size)):
            ch, m = chunks[j], chunks[j].get("metadata", {})
            ids.append(ch.get("chunk_id", f"chunk_{j}"))
            embs.append(np.asarray(embeddings[j]).tolist())
            docs.append(ch["text"])
            metas.append({"paper_id": str(m.get("paper_id", "unknown")), "section": str(m.get("section", "unknown")),
                          "quality_score": float(m.get("quality_score", 0.0)), "chunk_index": str(m.get("chunk_index", j))})
        for attempt in range(3):
            try:
                coll.add(ids=ids, embeddings=embs, documents=docs, metadatas=metas)
                stored += len(ids)
                break
            except Exception as e:                                     # noqa: BLE001
                if attempt < 2:
                    time.sleep(0.5)
                    continue
                print(f"Error storing batch {s0 // batch_size}: {e}")
                for k in range(len(ids)):
                    try:
                        coll.add(ids=[ids[k]], embeddings=[embs[k]], documents=[docs[k]], metadatas=[metas[k]])
                        stored += 1
                    except Exception:
                        pass
    if stored == 0:
        print("\n❌ Failed to store any embeddings in ChromaDB")
    else:
        print(f"✅ Stored {stored:,} embeddings in ChromaDB")
    return stored


# --------------------------------------------------------------------------------------------- search (added step)
def check_chunk_count(n_rows: int, chunks, *, where=None, keep_mask=None, where_document=None, group_by_paper: bool = False) -> None:
    """`search_queries`: every mode that reads `chunks` (or `keep_mask`) row by row needs one entry per row of the shard; the first such
    mode that is on names the mismatch."""
    for mode, on, per_row in (("where", where is not None, chunks), ("keep_mask", keep_mask is not None, keep_mask),
                              ("where_document", where_document is not None, chunks), ("group_by_paper", group_by_paper, chunks)):
        if on and len(per_row) != n_rows:
            raise ValueError(f"{mode}: {len(per_row)} {'chunks' if per_row is chunks else 'entries'} for the shard's {n_rows} rows")


def n_cand_of(reranker, rerank_top_k: int, mmr_lambda, mmr_fetch_k: int) -> int:
    """Candidates per query where something picks among them afterwards: the reranker, MMR, or the fusion (each side's list)."""
    return rerank_top_k if reranker is not None else (mmr_fetch_k if mmr_lambda is not None else HYBRID_CANDIDATES)


def search_queries(model, chunks: List[Dict], shard: "ShardSink", queries: List[str], top_k: int = 10,
                   output_dir: str = "./embeddings_saved", chunk_base: int = 0, reranker=None, rerank_top_k: int = 32,
                   hybrid_alpha: Optional[float] = None, where=None,
                   where_document: Optional[Dict] = None, *, mmr_lambda: Optional[float] = None, mmr_fetch_k: int = 32,
                   keep_mask: Optional[np.ndarray] = None, group_by_paper: bool = False, chunks_per_paper: int = 1,
                   where_on_device: bool = False, min_score: Optional[float] = None, hybrid_filters: bool = False,
                   hybrid_on_device: bool = False, keyword_build_on_device: bool = False, document_regex: bool = False,
                   nprobe: Optional[int] = None, ivf_lists: Optional[int] = None, ivf_iters: int = 10, ivf_seed: int = 0,
                   binary_candidates: Optional[int] = None, binary_centre: Optional[str] = "mean", boost_spec: Optional[Dict] = None,
                   boost_weight: Optional[float] = None, pq_candidates: Optional[int] = None, pq_dsub: int = 8,
                   pq_centre: Optional[str] = "mean", graph_ef: Optional[int] = None, graph_degree: int = 32,
                   graph_entries: int = 8) -> List[Dict]:
    """Brute-force cosine top-k (config.yaml:63-64 `top_k: 10`) over the rank's fp16 rows in HBM; with
    torchrun each rank holds the contiguous row shard it encoded and the partial top-k lists are
    all-gathered over RCCL and merged.  `shard` is the `ShardSink` the encode step filled: rows [lo, hi) are already where they
    will be searched and nothing is uploaded here; the queries are encoded straight into an fp16 device matrix.  (A consumer that
    only has the `.npy` rows on disk builds a `store.HipCollection` instead.)  `chunks[j]` is row `chunk_base + j` of the corpus:
    with per-rank loading a rank only knows the chunk ids of its own rows, so the ids of the merged hits are exchanged (one
    `all_gather_object` of at most Q x k small entries).  Between the encoded queries and the rerank step this is the pipeline
    `HipCollection.query` runs too: `retrieval.RowFilters` builds the row bitmaps, `retrieval.retrieve` searches, picks by MMR and fuses.
    `reranker` (a `rerank.HipCrossEncoder`, or anything with its `predict`): the search fetches `rerank_top_k` candidates, each rank
    scores the (query, candidate) pairs whose texts it holds, the scores are exchanged over the host group, and the best `top_k` by
    rerank score are kept; every hit then carries `rerank_score` beside its cosine `score`.
    `hybrid_alpha` (a float in [0, 1]; None = cosine only): hybrid search (config.yaml:67-68).  Each rank also builds a BM25
    `keyword.KeywordIndex` over the word pieces of its own chunks (statistics summed over the ranks); the cosine and the keyword search
    each fetch HYBRID_CANDIDATES rows per query (`rerank_top_k` with a reranker), `keyword.fuse` ranks their union by
    `alpha * normalised cosine + (1 - alpha) * normalised BM25`, and the best `top_k` (with a reranker: the fused `rerank_top_k`, then
    reranked) are kept.  Every hit then carries `hybrid_score` and `keyword_score`; `score` stays the cosine one and is null, like
    `keyword_score`, where the row was not in that side's candidate list.
    `where` (a Chroma filter, see `where.compile_where`): only chunks whose `metadata` satisfies it are searched — each rank evaluates it
    on its own `chunks`, packs the row bitmap and searches with it (`ShardIndex.search(allow=...)`: the exact top-k of the allowed rows,
    on the fp16 rows).  Not together with `hybrid_alpha`: the keyword search has no row filter.  A LIST with one filter or None per
    query (`--where-file`) restricts every query to its own filter: one bitmap per distinct filter, and-ed with `keep_mask` and
    `where_document`, and one `ShardIndex.search_filtered_many` per 64 distinct filters instead of one search per filter.
    `where_document` (a Chroma document filter, see `where_document.compile_where_document`): only chunks whose `text` satisfies it
    (`$contains` / `$not_contains`, case-sensitive substrings) are searched — each rank uploads the texts of its own `chunks`, scans them
    on the device (`arx_text_contains`) and searches with the resulting bitmap, and-ed with the one of `where` if both are given; nothing
    new crosses ranks.  Not together with `hybrid_alpha` either.
    `mmr_lambda` (a float in [0, 1]; None = off): maximal marginal relevance (INTEGRATION.md "MMR").  The search fetches `mmr_fetch_k`
    (in [top_k, 32]) candidates per query, filters applied as without it; each rank gathers the candidates' rows it owns, the buffers are
    summed over the ranks (`mmr.exchange_candidate_rows`) and `arx_mmr_select` picks `top_k` of them.  The hits come in pick order and
    carry `mmr_score` beside the cosine `score`.  Not together with `reranker` or `hybrid_alpha` (out of scope).
    `keep_mask` (bool, one entry per row of the shard; None = every row): rows to search at all — `--dedup-threshold` passes the rows that
    are not near-duplicates (`find_shard_duplicates`).  It is and-ed into the bitmap of `where` / `where_document`, or is the bitmap
    when neither is given.  Not together with `hybrid_alpha`, for the reason `where` is not.
    `group_by_paper` (False = nothing changes): grouped results (INTEGRATION.md "Grouped results").  `top_k` (<= 32) then counts PAPERS:
    consecutive chunks with equal `metadata["paper_id"]` are one paper (`grouping.runs_from_keys`), and the search returns the exact
    best papers by their best chunk, each with its `chunks_per_paper` (<= 8) best chunks (`ShardIndex.search_grouped`), filters applied
    as without it.  The hits come paper by paper, best paper first, and carry `paper_rank` and `paper_id`.  Not together with
    `reranker`, `hybrid_alpha`, `mmr_lambda`, a per-query `where` list or more than one rank (a paper may straddle ranks).
    `where_on_device` (False = nothing changes; needs `where`): the `where` filters are evaluated on the device from metadata columns
    uploaded once (`where_device.MetadataColumns` over this rank's `chunks`), `keep_mask` and `where_document` and-ed in by the same
    kernel, a per-query list in one launch per 64 distinct filters.  Same hits as without it.
    `min_score` (a float; None = nothing changes): a score threshold (INTEGRATION.md "Score threshold").  Only chunks whose cosine to the
    query is >= it are returned, the best `top_k` of them, `top_k` then in 1..1024 (`ShardIndex.search_range`), `where` /
    `where_document` / `keep_mask` applied as without it; every entry of the results then carries `truncated`: more chunks qualified than
    `top_k`.  Not together with `reranker`, `hybrid_alpha`, `mmr_lambda`, `group_by_paper`, a per-query `where` list or more than one
    rank (reranking and a cross-rank merge of long lists are out of scope here).
    `hybrid_filters` (False = nothing changes, every refusal above stays): `hybrid_alpha` then composes with `where` (a dict or a per-query
    list), `where_document`, `keep_mask` and `where_on_device`: the bitmaps the cosine search uses go to the keyword search unchanged
    (`KeywordIndex.search(allow=...)`, `arx_bm25_search_filtered`), so both candidate lists hold allowed rows only and the fusion is what it
    was.  The BM25 statistics stay those of the whole corpus (INTEGRATION.md "Hybrid search with filters").
    `hybrid_on_device` (False = nothing changes; needs `hybrid_alpha`): the two candidate lists are fused on the device
    (`keyword.fuse_device`) and, with a reranker, `rerank_top_k` may be up to 1024: the cosine side then comes from
    `ShardIndex.search_range(-inf)`, the keyword side from `KeywordIndex.search_wide`, and the cross-encoder scores the fused
    `rerank_top_k` 32 pairs at a time.  Beyond 32 not with a per-query `where` list or more than one rank.  With `rerank_top_k <= 32`
    the same hits as without it (INTEGRATION.md "Hybrid search on the device").
    `keyword_build_on_device` (False = nothing changes; needs `hybrid_alpha`): the BM25 index is built on the device
    (`KeywordIndex(build_on_device=True)`); it is the default build's, bit for bit, so the hits are the same (INTEGRATION.md "Building the
    keyword index on the device").
    `document_regex` (False = nothing changes): `where_document` also takes `$regex` / `$not_regex` leaves (`--where-document-regex`),
    compiled on the host to byte-level DFAs (`regex_dfa.compile_regex`: the dialect and its limits) and scanned on the device
    (`arx_text_regex`); the bitmap goes where the `$contains` one goes (INTEGRATION.md "Document filters").
    `nprobe` with `ivf_lists` (None = nothing changes): the IVF probe search (INTEGRATION.md "IVF probe search").  An `ivf.IvfIndex` with
    `ivf_lists` lists is built over the shard (`ivf_iters`, `ivf_seed`) and every query is scored against the rows of its `nprobe` nearest
    lists only, filters applied as without it; every entry of the results then carries `ivf_scanned`, the rows scored.  Composes with
    `where` (one dict, or a list with one filter per query: one IVF call per batch whatever the number of distinct filters),
    `where_document`, `keep_mask`, `reranker`, `mmr_lambda` and `min_score` (`top_k` then at most 32).  With a `where` list or `min_score`
    the entries also carry `ivf_hits`, the exact number of visible chunks at or above the threshold (without one: the rows scored), and
    with `min_score` `truncated` (`ivf_hits > top_k`).  Not together with `hybrid_alpha`, `group_by_paper` or more than one rank.
    `binary_candidates` (None = nothing changes): the binary-code search (INTEGRATION.md "Binary-code search").  A `binary.BinaryIndex` is
    packed over the shard (`binary_centre`: "mean", the column mean of the rows, or None / "none", zero) and every query's first
    `binary_candidates` (at most 256, at least the width the search returns) visible rows by Hamming distance of the sign bits are
    rescored exactly, `where` (one dict), `where_document` and `keep_mask` applied as without it; every entry of the results then
    carries `binary_count`, the candidates rescored.  Composes with `reranker` and `mmr_lambda`.
    `boost_weight` with `boost_spec` (both or neither; None = nothing changes): the boosted search (INTEGRATION.md "Boosted search").
    `boost.prior_from_metadata(the chunks' metadata, boost_spec)` gives one prior per chunk, the ranking is by float32(cosine +
    float32(boost_weight * prior)) under the bitmap of `where`, `where_document` and `keep_mask`, every hit's "score" is the boosted
    value and an added "base_score" the cosine.
    `pq_candidates` (None = nothing changes): the product-quantised search (INTEGRATION.md "Product-quantised search").  A `pq.PqIndex`
    is trained and encoded over the shard (`pq_dsub` dimensions per code byte; `pq_centre`: "mean" or None / "none") and every query's
    first `pq_candidates` (at most 256, at least the width the search returns) visible rows by the sum of its byte tables over the
    codes are rescored exactly, `where` (one dict), `where_document` and `keep_mask` applied as without it; every entry of the
    results then carries `pq_count`, the candidates rescored.  Composes with `reranker` and `mmr_lambda`.
    `graph_ef` (None = nothing changes): the graph search (INTEGRATION.md "Graph search").  A `graph.GraphIndex` of degree
    `graph_degree` is built over the shard (exact k-NN lists, about sqrt(rows) entry lists) and every query walks it with a beam of
    `graph_ef` rows (at most 512, at least the width the search returns) from the medoids of its `graph_entries` nearest entry
    centroids, `where` (one dict), `where_document` and `keep_mask` restricting what comes back as without it; every entry of the
    results then carries `graph_scored`, the rows scored.  Composes with `reranker` and `mmr_lambda`.
    None of `binary_candidates`, `boost_weight`, `pq_candidates` and `graph_ef` goes together with another of them, `nprobe`,
    `hybrid_alpha`, `group_by_paper`, `min_score`, a per-query `where` list or more than one rank: a ValueError from `modes.check_mode`
    (the table is `modes.MODES`), before anything is launched."""
    from .retrieval import RowFilters, check_hybrid_on_device, check_shared_query, retrieve
    if keyword_build_on_device and hybrid_alpha is None:
        raise ValueError("keyword_build_on_device needs hybrid_alpha: it chooses where the BM25 keyword index is built")
    if hybrid_on_device:
        if hybrid_alpha is None:
            raise ValueError("hybrid_on_device needs hybrid_alpha: it chooses where the two candidate lists are fused")
        check_hybrid_on_device(rerank_top_k if reranker is not None else HYBRID_CANDIDATES, per_query_filters=isinstance(where, (list, tuple)),
                               world=int(os.environ.get("WORLD_SIZE", "1")))
    if min_score is not None:
        from .ranging import check_range_query
        if reranker is not None:
            raise ValueError("min_score cannot be combined with reranker here: reranking a long range list is out of scope for search_queries")
        check_range_query(top_k, ranged=True, hybrid_alpha=hybrid_alpha, mmr_lambda=mmr_lambda, group_by=group_by_paper,    # (IVF: a bitmap per query)
                          per_query_filters=isinstance(where, (list, tuple)) and nprobe is None, world=int(os.environ.get("WORLD_SIZE", "1")))
    from functools import partial
    from .modes import check_mode
    # every mode refuses through `modes.check_mode` with the one context; the boost is asked first here, and what a mode builds is checked with it
    refuse = partial(check_mode, per_query=isinstance(where, (list, tuple)), hybrid_alpha=hybrid_alpha, group_by=group_by_paper, min_score=min_score,
                     world=int(os.environ.get("WORLD_SIZE", "1")), has_index=True,
                     n_width=n_cand_of(reranker, rerank_top_k, mmr_lambda, mmr_fetch_k) if (reranker is not None or mmr_lambda is not None) else top_k,
                     others={"graph_ef": graph_ef, "pq_candidates": pq_candidates, "boost_weight": boost_weight, "binary_candidates": binary_candidates,
                             "nprobe": nprobe if nprobe is not None else ivf_lists})
    if (boost_weight is None) != (boost_spec is None):
        raise ValueError("boost_weight and boost_spec go together: the weight and the metadata key the prior comes from")
    if boost_weight is not None:
        from .boost import prior_from_metadata
        refuse("boost_weight", boost_weight, n_queries=len(queries))
        prior_host = prior_from_metadata([c.get("metadata") or {} for c in chunks], boost_spec)      # (a bad spec or value: refused here)
    if graph_ef is not None:
        from .graph import check_build_args as check_graph_build
        n_entry_lists = check_graph_build(int(shard.rows.shape[0]), int(shard.rows.shape[1]), graph_degree, None, 10)
        refuse("graph_ef", graph_ef, n_entries=graph_entries, n_entry_lists=n_entry_lists, degree=int(graph_degree))
    if pq_candidates is not None:
        from .pq import check_dsub
        if pq_centre not in (None, "none", "mean"):
            raise ValueError(f"pq_centre={pq_centre!r} must be \"mean\" or \"none\"")
        refuse("pq_candidates", pq_candidates)
        check_dsub(int(shard.rows.shape[1]), pq_dsub)
    if binary_candidates is not None:
        if binary_centre not in (None, "none", "mean"):
            raise ValueError(f"binary_centre={binary_centre!r} must be \"mean\" or \"none\"")
        refuse("binary_candidates", binary_candidates)
    if nprobe is not None or ivf_lists is not None:
        from .ivf import check_build_args
        if nprobe is None or ivf_lists is None:
            raise ValueError("nprobe and ivf_lists go together: the lists to build and how many of them a query probes")
        refuse("nprobe", nprobe, n_lists=int(ivf_lists), n_width=top_k if min_score is not None else 1, let_through=("per_query", "min_score"))
        check_build_args(int(shard.rows.shape[0]), int(shard.rows.shape[1]), ivf_lists, ivf_iters, None)
    if where_on_device and where is None:
        raise ValueError("where_on_device needs where: it chooses where the where filters are evaluated")
    if group_by_paper:
        from .grouping import check_grouped_query
        check_grouped_query(top_k, chunks_per_paper, grouped=True, reranker=reranker, hybrid_alpha=hybrid_alpha, mmr_lambda=mmr_lambda,
                            per_query_filters=isinstance(where, (list, tuple)), world=int(os.environ.get("WORLD_SIZE", "1")))
    check_shared_query(top_k, hybrid_alpha=hybrid_alpha, hybrid_filters=hybrid_filters, reranker=reranker, mmr_lambda=mmr_lambda,
                       n_fetch=mmr_fetch_k, fetch_refusal=f"mmr_fetch_k={mmr_fetch_k} must be in [top_k, {MMR_MAX_FETCH_K}] (top_k={top_k})",
                       filters_first=(("keep_mask cannot be combined", keep_mask is not None),),
                       filters=(("where cannot be combined", where is not None), ("where_document cannot be combined", where_document is not None)))
    import torch
    from .index import ShardIndex
    dist = _dist()
    rank = dist.get_rank() if dist else 0
    world = dist.get_world_size() if dist else 1
    dev = model.encoder.device
    qd = torch.empty((len(queries), model.get_sentence_embedding_dimension()), dtype=torch.float16, device=dev)
    model.encode(queries, batch_size=256, normalize_embeddings=True, convert_to_numpy=True, device_f16_out=qd, low_latency=True)
    n_rows, dim = shard.rows.shape
    check_chunk_count(n_rows, chunks, where=where, keep_mask=keep_mask, where_document=where_document, group_by_paper=group_by_paper)
    if where_document is not None:                           # (one dict for the call: a list is refused, as anything else that is no filter)
        from .where_document import compile_where_document
        compile_where_document(where_document, regex=document_regex)
    # int8 pre-filter (same exact answers; +50 % shard memory, one quantisation pass): 1.5-1.7x the queries per second on small batches;
    # a filtered, a grouped and a range search run on the fp16 rows
    masked = (where is not None or keep_mask is not None or where_document is not None or group_by_paper or min_score is not None or nprobe is not None or binary_candidates is not None
              or boost_weight is not None or pq_candidates is not None or graph_ef is not None
              or (hybrid_on_device and n_cand_of(reranker, rerank_top_k, mmr_lambda, mmr_fetch_k) > HYBRID_CANDIDATES))
    index = ShardIndex(shard.rows, idx_base=shard.lo, prefilter="int8" if (dim % 128 == 0 and dim <= 1024 and n_rows > 0 and not masked) else None,
                       adaptive=True)
    if min_score is not None and world > 1:
        raise ValueError("min_score needs a single GPU rank: a cross-rank merge of lists of up to 1024 rows is out of scope")
    if group_by_paper:
        from .grouping import runs_from_keys
        if world > 1:
            raise ValueError("group_by_paper needs a single GPU rank: a paper may straddle two ranks, and a cross-rank fold is out of scope")
        group_of, paper_ids = runs_from_keys([(c.get("metadata") or {}).get("paper_id") for c in chunks], base=chunk_base)
        index.set_groups(group_of)
    n_cand = n_cand_of(reranker, rerank_top_k, mmr_lambda, mmr_fetch_k)

    def keyword_index():                                     # (built per call, after the cosine search)
        from .keyword import KeywordIndex
        if top_k > n_cand:
            raise ValueError(f"hybrid search keeps at most {n_cand} results per query (top_k={top_k})")
        return KeywordIndex(texts=[c["text"] for c in chunks], tokenizer=model.tokenizer, stats="global" if world > 1 else None,
                            idx_base=chunk_base, device=dev, **({"build_on_device": True} if keyword_build_on_device else {}))
    # (a count the device would have to be waited for is left unknown for per-query lists: it merely steers the search's path)
    filters = RowFilters([c.get("metadata") or {} for c in chunks] if where is not None else (), dev, 0, n_rows, keep_mask=keep_mask,
                         texts=lambda: [c["text"] for c in chunks], where_on_device=where_on_device, count_both=False,
                         document_regex=document_regex)
    hit = retrieve(index, qd, filters, top_k, n_candidates=n_cand, reranked=reranker is not None, where=where, where_document=where_document,
                   min_score=None if min_score is None else float(min_score), grouped=group_by_paper, chunks_per_group=chunks_per_paper, mmr_lambda=mmr_lambda,
                   hybrid_alpha=hybrid_alpha, keyword=keyword_index, query_texts=queries, hybrid_on_device=hybrid_on_device, world=world,
                   **({} if nprobe is None else {"nprobe": int(nprobe), "ivf": build_ivf_index(index, ivf_lists, ivf_iters, ivf_seed)}),
                   **({} if binary_candidates is None else {"binary_candidates": int(binary_candidates), "binary": build_binary_index(index, binary_centre)}),
                   **({} if pq_candidates is None else {"pq_candidates": int(pq_candidates), "pq": build_pq_index(index, pq_dsub, pq_centre)}),
                   **({} if graph_ef is None else {"graph_ef": int(graph_ef), "graph": build_graph_index(index, graph_degree),
                                                   "graph_entries": int(graph_entries)}),
                   **({} if boost_weight is None else {"boost_weight": float(boost_weight), "prior": torch.from_numpy(prior_host).to(dev)}))
    base_of = (lambda qi, p: {}) if hit.base is None else (lambda qi, p: {"base_score": float(hit.base[qi, p])})
    s, i, grp, truncated, mmr_val, hyb, kws = hit.scores, hit.ids, hit.groups, hit.truncated, hit.mmr, hit.hybrid, hit.keyword
    if reranker is not None:
        from .ranging import RERANK_BATCH
        from .rerank import rerank_candidates, reorder_by_rerank
        texts = {int(j): chunks[int(j) - chunk_base]["text"] for j in np.unique(i) if chunk_base <= j < chunk_base + len(chunks)}
        scores = rerank_candidates(lambda pairs: reranker.predict(pairs, batch_size=min(rerank_top_k, RERANK_BATCH) if hybrid_on_device else rerank_top_k,
                                                                   convert_to_numpy=True),
                                   queries, i, texts, dist=dist if world > 1 else None, group=host_group() if world > 1 else None)
        picked = reorder_by_rerank(i, scores, top_k)
    names = {int(j): chunks[int(j) - chunk_base].get("chunk_id", f"chunk_{int(j)}")
             for j in np.unique(i) if chunk_base <= j < chunk_base + len(chunks)}
    if dist and world > 1:
        parts: List = [None] * world
        dist.all_gather_object(parts, names, group=host_group())
        names = {k: v for part in parts for k, v in part.items()}
    results = []
    counters = {c: getattr(hit, c) for c in ("ivf_scanned", "ivf_hits", "binary_count", "pq_count", "graph_scored") if getattr(hit, c) is not None}

    def scanned_of(qi):                                      # the rows the mode that ran scored (with nprobe also the hits, where counted)
        return {c: int(v[qi]) for c, v in counters.items()}

    def hybrid_fields(qi, p):                                # (null, not NaN, in the JSON file)
        if hyb is None:
            return {}
        return {"score": None if np.isnan(s[qi, p]) else float(s[qi, p]), "hybrid_score": float(hyb[qi, p]),
                "keyword_score": None if np.isnan(kws[qi, p]) else float(kws[qi, p])}

    for qi, text in enumerate(queries):
        hits = []
        if reranker is not None:
            for r, (p, j, rs_) in enumerate(picked[qi]):
                hits.append({"rank": r + 1, "score": float(s[qi, p]), "rerank_score": float(rs_), "index": j,
                             "chunk_id": names.get(j, f"chunk_{j}"), **hybrid_fields(qi, p), **base_of(qi, p)})
            results.append({"query": text, "results": hits, **scanned_of(qi)})
            continue
        if grp is not None:                                   # paper by paper; the padding of short papers is skipped
            for r in range(i.shape[1]):
                j, p = int(i[qi, r]), r // chunks_per_paper
                if j >= 0:
                    hits.append({"rank": len(hits) + 1, "paper_rank": p + 1, "paper_id": paper_ids[int(grp[qi, p])], "score": float(s[qi, r]),
                                 "index": j, "chunk_id": names.get(j, f"chunk_{j}")})
            results.append({"query": text, "results": hits})
            continue
        for r in range(top_k):
            j = int(i[qi, r])
            if j < 0:
                continue
            hits.append({"rank": r + 1, "score": float(s[qi, r]), "index": j, "chunk_id": names.get(j, f"chunk_{j}"),
                         **hybrid_fields(qi, r), **({} if mmr_val is None else {"mmr_score": float(mmr_val[qi, r])}), **base_of(qi, r)})
        results.append({"query": text, "results": hits, **({} if truncated is None else {"truncated": bool(truncated[qi])}), **scanned_of(qi)})
    if rank == 0:
        with open(Path(output_dir) / "search_results.json", "w", encoding="utf-8") as fh:
            json.dump(results, fh, indent=2, ensure_ascii=False)
        print(f"✅ Saved top-{top_k} {'papers' if group_by_paper else 'results'} for {len(queries)} queries to {Path(output_dir) / 'search_results.json'}")
    return results


def build_ivf_index(index, n_lists: int, iters: int = 10, seed: int = 0):
    """`--ivf-lists`: the `ivf.IvfIndex` of the search step's shard, with its summary printed."""
    from .ivf import IvfIndex
    ivf = IvfIndex.build(index, int(n_lists), iters=int(iters), seed=int(seed))
    info = ivf.summary()
    print(f"IVF index: {info['n_lists']} lists of {info['list_rows_min']} / {info['list_rows_median']:.0f} / {info['list_rows_max']} rows "
          f"(min / median / max), {info['iterations']} iterations on {info['train_rows']} rows, {info['seconds']:.2f} s")
    return ivf


def build_binary_index(index, centre: Optional[str] = "mean"):
    """`--binary-candidates`: the `binary.BinaryIndex` of the search step's shard, with its size printed."""
    from .binary import BinaryIndex
    bi = BinaryIndex.build(index, centre=None if centre in (None, "none") else "mean")
    n, w = (int(v) for v in bi.codes.shape)
    print(f"Binary index: {n} rows x {w * 64} sign bits ({n * w * 8} bytes), centre {'none' if bi.centre is None else 'mean'}")
    return bi


def build_pq_index(index, dsub: int = 8, centre: Optional[str] = "mean"):
    """`--pq-candidates`: the `pq.PqIndex` of the search step's shard (codebooks trained here), with its size printed."""
    from .pq import PqIndex
    pi = PqIndex.build(index, dsub=int(dsub), centre=None if centre in (None, "none") else "mean")
    n, m = (int(v) for v in pi.codes.shape)
    print(f"PQ index: {n} rows x {m} code bytes (dsub {int(dsub)}, {n * m} bytes), centre {'none' if pi.centre is None else 'mean'}")
    return pi


def build_graph_index(index, degree: int = 32):
    """`--graph-ef`: the `graph.GraphIndex` of the search step's shard (exact k-NN lists), with its summary printed."""
    from .graph import GraphIndex
    g = GraphIndex.build(index, degree=int(degree))
    info = g.summary()
    print(f"Graph index: {info['rows']} rows x degree {info['degree']}, {info['edges']} edges, {info['entry_lists']} entry lists, "
          f"{info['seconds']:.2f} s")
    return g


# --------------------------------------------------------------------------------------------- main
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Generate embeddings on MI355X (drop-in for generate_embeddings_parallel.py)")
    p.add_argument("input_dir", type=str, help="Input directory (output_improved)")
    p.add_argument("--model", type=str, default="all-mpnet-base-v2",
                   help=f"Embedding model: one of {MODEL_CHOICES} (resolved to a LOCAL directory) or a model directory")
    p.add_argument("--min-quality", type=float, default=0.9, help="Minimum quality score (default: 0.9)")
    p.add_argument("--batch-size", type=int, default=200, help="Batch size for embedding generation (default: 200)")
    p.add_argument("--chroma-db", type=str, default="./chroma_db", help="Path to ChromaDB (default: ./chroma_db)")
    p.add_argument("--collection-name", type=str, default="scientific_papers", help="ChromaDB collection name")
    p.add_argument("--load-workers", type=int, default=None, help="Number of workers for loading (default: 80%% of CPU cores)")
    p.add_argument("--embedding-workers", type=int, default=None,
                   help="Accepted for compatibility; embedding parallelism = one process per GPU (torchrun)")
    p.add_argument("--store-batch-size", type=int, default=2000, help="Batch size for storing in ChromaDB (default: 2000)")
    p.add_argument("--chunks-per-worker", type=int, default=500, help="Chunks per work quantum (default: 500)")
    # additive
    p.add_argument("--model-dir", type=str, default=None, help="Directory holding local model folders (sets ARX_MODEL_DIR)")
    p.add_argument("--out-dtype", type=str, default="float64", choices=["float64", "float32", "float16"],
                   help="dtype of embeddings.npy (default float64 = the reference's layout)")
    p.add_argument("--queries", type=str, default=None, help="Text file, one query per line: run the cosine top-k step")
    p.add_argument("--top-k", type=int, default=10, help="Results per query (default: 10)")
    p.add_argument("--skip-chroma", action="store_true", help="Do not attempt ChromaDB ingestion")
    p.add_argument("--rerank-model", type=str, default=None,
                   help="Cross-encoder (name resolved to a LOCAL directory, or a directory) that reranks the --queries candidates")
    p.add_argument("--rerank-top-k", type=int, default=32,
                   help=f"Candidates the search fetches for the reranker (default: 32; at most {RERANK_MAX_K}, the search's k limit)")
    p.add_argument("--hybrid-alpha", type=float, default=None,
                   help="Hybrid search for --queries: weight of the cosine side in [0, 1], the BM25 keyword side gets the rest "
                        "(config.yaml hybrid_alpha: 0.7; default: off, cosine only)")
    p.add_argument("--hybrid-filters", action="store_true",
                   help="Let --hybrid-alpha compose with --where, --where-file, --where-document and --dedup-threshold: the BM25 keyword "
                        "search reads the same row bitmaps as the cosine search (default: off, those combinations are refused)")
    p.add_argument("--hybrid-on-device", action="store_true",
                   help=f"Fuse the two candidate lists of --hybrid-alpha on the GPU; --rerank-top-k may then be up to {HYBRID_DEVICE_MAX_K} "
                        "(beyond 32: one GPU rank only, not with --where-file).  config.yaml's recipe: --hybrid-alpha 0.7 --rerank-model ... "
                        "--rerank-top-k 50 --top-k 10 --hybrid-on-device (default: off, the lists are fused on the host)")
    p.add_argument("--keyword-build-on-device", action="store_true",
                   help="Build the BM25 keyword index of --hybrid-alpha on the GPU (a radix sort of the word pieces) instead of with numpy "
                        "on the host; the index and the results are the same (default: off)")
    p.add_argument("--where", type=str, default=None,
                   help="Chroma metadata filter for --queries as JSON, e.g. '{\"section\": \"abstract\"}' or "
                        "'{\"quality_score\": {\"$gte\": 0.95}}': only matching chunks are searched (with --hybrid-alpha only next to --hybrid-filters)")
    p.add_argument("--where-file", type=str, default=None,
                   help="A different --where filter per query: a JSON-lines file with one filter object or null (no filter) per line, "
                        "one line per query of --queries; the batch is searched in one pass over the rows (not with --where; "
                        "with --hybrid-alpha only next to --hybrid-filters)")
    p.add_argument("--where-on-device", action="store_true",
                   help="Evaluate the --where / --where-file filters on the GPU from metadata columns kept in HBM, not with numpy on "
                        "the host (same results; needs --where or --where-file)")
    p.add_argument("--where-document", type=str, default=None,
                   help="Chroma document filter for --queries as JSON, e.g. '{\"$contains\": \"Lipschitz\"}' or "
                        "'{\"$and\": [{\"$contains\": \"graph\"}, {\"$not_contains\": \"lemma\"}]}': only chunks whose text "
                        "satisfies it are searched (case-sensitive substrings, scanned on the GPU; with --hybrid-alpha only next to --hybrid-filters)")
    p.add_argument("--where-document-regex", action="store_true",
                   help="Let the --where-document filter use '{\"$regex\": \"...\"}' and '{\"$not_regex\": \"...\"}' as well, e.g. "
                        "'{\"$regex\": \"(?i)transformer\"}': the pattern is compiled to a DFA and the texts are scanned on the GPU "
                        "(ASCII \\d \\w \\s, ASCII-only (?i); no backreferences, look-around or \\b; needs --where-document)")
    p.add_argument("--mmr-lambda", type=float, default=None,
                   help="Diversify the --queries results by maximal marginal relevance: weight of the relevance term in [0, 1], the "
                        "penalty on similarity to the rows already picked gets the rest (default: off; not with --rerank-model or "
                        "--hybrid-alpha)")
    p.add_argument("--mmr-fetch-k", type=int, default=32,
                   help="Candidates the search fetches for --mmr-lambda to pick --top-k from (default: 32, the search's k limit)")
    p.add_argument("--dedup-threshold", type=float, default=None,
                   help="Near-duplicate detection: a chunk whose embedding scores at least this cosine, in (0, 1], against ANY earlier "
                        "chunk is listed in duplicates.json with its nearest earlier chunk, and a --queries search skips it (default: "
                        "off; one GPU rank only; with --hybrid-alpha and --queries only next to --hybrid-filters)")
    p.add_argument("--group-by-paper", action="store_true",
                   help="Grouped results for --queries: --top-k counts PAPERS (consecutive chunks with equal paper_id), the exact best "
                        "by their best chunk, each with its --chunks-per-paper best chunks (one GPU rank only; not with --rerank-model, "
                        "--hybrid-alpha, --mmr-lambda or --where-file)")
    p.add_argument("--min-score", type=float, default=None,
                   help="Score threshold for --queries: only chunks whose cosine to the query is at least this are returned, the best "
                        "--top-k of them, --top-k then in 1..1024; every query's entry carries `truncated` (default: off; one GPU rank "
                        "only; not with --rerank-model, --hybrid-alpha, --mmr-lambda, --group-by-paper or --where-file)")
    p.add_argument("--chunks-per-paper", type=int, default=1,
                   help="Chunks returned for each paper of --group-by-paper (default: 1; at most 8)")
    p.add_argument("--facets", type=str, default=None,
                   help="Facet counts beside the --queries results: metadata keys separated by commas, e.g. section,paper_id; for each "
                        "key facets.json lists its values with the most chunks among those --where / --where-document (or each line of "
                        "--where-file) allow, counted on the GPU (default: off; needs --queries; one GPU rank only)")
    p.add_argument("--facets-top", type=int, default=10, help="Values listed per key of --facets (default: 10)")
    p.add_argument("--topics", type=int, default=None,
                   help="Topic clustering beside the --queries results: spherical k-means with this many topics over the embeddings of the "
                        "chunks --where / --where-document allow, on the GPU; topics.json lists the sizes, the objective and each topic's "
                        "nearest chunks (default: off; needs --queries; one GPU rank only; not with --where-file)")
    p.add_argument("--topics-iters", type=int, default=20, help="Iterations of --topics at most (default: 20)")
    p.add_argument("--topics-seed", type=int, default=0, help="Seed of the initial centroids of --topics (default: 0)")
    p.add_argument("--ivf-lists", type=int, default=None,
                   help="IVF probe search: cluster the chunks into this many lists (1..4096, spherical k-means on the GPU) before the "
                        "--queries search (default: off; needs --nprobe and --queries; one GPU rank only)")
    p.add_argument("--ivf-iters", type=int, default=10, help="Iterations of the --ivf-lists k-means at most (default: 10)")
    p.add_argument("--ivf-seed", type=int, default=0, help="Seed of the --ivf-lists sample and initial centroids (default: 0)")
    p.add_argument("--nprobe", type=int, default=None,
                   help="IVF probe search: score every query against the chunks of its this many nearest lists only (1..min(128, "
                        "--ivf-lists); exact among those; not with --hybrid-alpha, --group-by-paper, --min-score or --where-file)")
    p.add_argument("--binary-candidates", type=int, default=None,
                   help="Binary-code search: rank every chunk by the Hamming distance of its sign bits to the query's and rescore the "
                        "best this many exactly (1..256, at least the search's width; default: off; needs --queries; one GPU rank "
                        "only; not with --nprobe, --hybrid-alpha, --group-by-paper, --min-score or --where-file)")
    p.add_argument("--binary-centre", choices=("mean", "none"), default="mean",
                   help="What the sign bits of --binary-candidates are taken against: the column mean of the chunks' rows, or zero "
                        "(default: mean)")
    p.add_argument("--pq-candidates", type=int, default=None,
                   help="Product-quantised search: rank every chunk by the sum of the query's byte look-up tables over its 8-bit PQ "
                        "code and rescore the best this many exactly (1..256, at least the search's width; default: off; needs "
                        "--queries; one GPU rank only; not with --nprobe, --binary-candidates, --hybrid-alpha, --group-by-paper, "
                        "--min-score, --boost-key or --where-file)")
    p.add_argument("--pq-dsub", type=int, default=8,
                   help="Dimensions per code byte of --pq-candidates: a power of two in 4..64 (default: 8, dim / 8 bytes per chunk)")
    p.add_argument("--pq-centre", choices=("mean", "none"), default="mean",
                   help="What the rows are centred on before --pq-candidates encodes them: the column mean of the chunks' rows, or "
                        "zero (default: mean)")
    p.add_argument("--graph-ef", type=int, default=None,
                   help="Graph search: build a k-NN graph over the chunks and answer every query by a beam search of this width over "
                        "it, every score exact (at most 512, at least the search's width; default: off; needs --queries; one GPU "
                        "rank only; not with --nprobe, --binary-candidates, --pq-candidates, --hybrid-alpha, --group-by-paper, "
                        "--min-score, --boost-key or --where-file)")
    p.add_argument("--graph-degree", type=int, default=32,
                   help="Neighbours per chunk of --graph-ef's graph: a multiple of 8 in 8..32 (default: 32)")
    p.add_argument("--graph-entries", type=int, default=8,
                   help="Entry points per query of --graph-ef: the medoids of this many nearest entry centroids, 1..32 (default: 8)")
    p.add_argument("--boost-key", type=str, default=None,
                   help="Boosted search: rank by cosine + --boost-weight * prior, the prior being this metadata key's numeric value "
                        "(missing: 0), or its exponential decay with --boost-decay-origin / --boost-half-life (default: off; needs "
                        "--queries and --boost-weight; one GPU rank only; not with --hybrid-alpha, --group-by-paper, --min-score, "
                        "--nprobe, --binary-candidates or --where-file)")
    p.add_argument("--boost-weight", type=float, default=None, help="The weight of the --boost-key prior (finite; negative penalises)")
    p.add_argument("--boost-decay-origin", type=float, default=None,
                   help="With --boost-half-life: the prior is exp(-ln 2 * |value - origin| / half_life) of the --boost-key value")
    p.add_argument("--boost-half-life", type=float, default=None, help="The half-life of the --boost-decay-origin decay (> 0)")
    return p


RERANK_MAX_K = 32          # the exact top-k search returns k <= 32 per query (search.hip KMAX)
HYBRID_DEVICE_MAX_K = 1024  # ... and with --hybrid-on-device the fused list may be this long (retrieval.HYBRID_DEVICE_CANDIDATES)


def check_rerank_args(args) -> Optional[str]:
    """-> an error message for an unusable --rerank-top-k, else None."""
    if not args.rerank_model:
        return None
    on_device = getattr(args, "hybrid_on_device", False) and getattr(args, "hybrid_alpha", None) is not None
    if on_device and args.rerank_top_k > HYBRID_DEVICE_MAX_K:
        return f"--rerank-top-k {args.rerank_top_k}: --hybrid-on-device fuses at most {HYBRID_DEVICE_MAX_K} candidates per side"
    if not on_device and args.rerank_top_k > RERANK_MAX_K:
        return f"--rerank-top-k {args.rerank_top_k}: the search returns at most k <= {RERANK_MAX_K} candidates per query"
    if args.rerank_top_k < args.top_k:
        return f"--rerank-top-k {args.rerank_top_k} is below --top-k {args.top_k}: the reranker must see at least the results it keeps"
    return None


HYBRID_CANDIDATES = 32     # rows each side of a hybrid search contributes per query (the candidate lists' length limit)


def check_hybrid_args(args) -> Optional[str]:
    """-> an error message for an unusable --hybrid-alpha, else None."""
    if args.hybrid_alpha is None:
        return None
    if not (0.0 <= args.hybrid_alpha <= 1.0):                 # (also rejects nan)
        return f"--hybrid-alpha {args.hybrid_alpha}: the weight of the cosine side must be in [0, 1]"
    if args.top_k > HYBRID_CANDIDATES:
        return f"--top-k {args.top_k}: hybrid search fuses {HYBRID_CANDIDATES} candidates per side and returns at most that many"
    return None


def check_hybrid_device_args(args) -> Optional[str]:
    """-> an error message for an unusable --hybrid-on-device, else None.  (The other flags are read with getattr: absent = off.)"""
    if not getattr(args, "hybrid_on_device", False):
        return None
    if getattr(args, "hybrid_alpha", None) is None:
        return "--hybrid-on-device needs --hybrid-alpha: it chooses where the two candidate lists are fused"
    if getattr(args, "rerank_model", None) and getattr(args, "rerank_top_k", 32) > RERANK_MAX_K:
        if getattr(args, "where_file", None):
            return (f"--hybrid-on-device with --rerank-top-k above {RERANK_MAX_K} cannot be combined with --where-file: the range search "
                    "that fetches the long dense list takes one bitmap per call")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            return (f"--hybrid-on-device with --rerank-top-k above {RERANK_MAX_K} needs a single GPU rank: a cross-rank merge of long "
                    "candidate lists is out of scope")
    return None


def check_keyword_build_args(args) -> Optional[str]:
    """-> an error message for an unusable --keyword-build-on-device, else None."""
    if getattr(args, "keyword_build_on_device", False) and getattr(args, "hybrid_alpha", None) is None:
        return "--keyword-build-on-device needs --hybrid-alpha: it chooses where the BM25 keyword index is built"
    return None


MMR_MAX_FETCH_K = 32       # candidate slots of arx_mmr_select = the search's k limit


def check_hybrid_filters_args(args) -> Optional[str]:
    """-> an error message for an unusable --hybrid-filters, else None.  (The other flags are read with getattr: absent = off.)"""
    if not getattr(args, "hybrid_filters", False):
        return None
    if getattr(args, "hybrid_alpha", None) is None:
        return "--hybrid-filters needs --hybrid-alpha: it lets the hybrid search take the row filters"
    if all(getattr(args, name, None) is None for name in ("where", "where_file", "where_document", "dedup_threshold")):
        return ("--hybrid-filters needs --where, --where-file, --where-document or --dedup-threshold: it passes their row bitmaps to the "
                "BM25 keyword search")
    return None


def check_mmr_args(args) -> Optional[str]:
    """-> an error message for an unusable --mmr-lambda / --mmr-fetch-k, else None."""
    if args.mmr_lambda is None:
        return None
    if not (0.0 <= args.mmr_lambda <= 1.0):                   # (also rejects nan)
        return f"--mmr-lambda {args.mmr_lambda}: the weight of the relevance term must be in [0, 1]"
    if args.rerank_model:
        return "--mmr-lambda cannot be combined with --rerank-model: MMR re-orders the cosine search's candidates only"
    if args.hybrid_alpha is not None:
        return "--mmr-lambda cannot be combined with --hybrid-alpha: MMR re-orders the cosine search's candidates only"
    if args.mmr_fetch_k > MMR_MAX_FETCH_K:
        return f"--mmr-fetch-k {args.mmr_fetch_k}: the search returns at most k <= {MMR_MAX_FETCH_K} candidates per query"
    if args.top_k < 1 or args.mmr_fetch_k < args.top_k:
        return f"--mmr-fetch-k {args.mmr_fetch_k} is below --top-k {args.top_k}: MMR picks its results among the candidates"
    return None


def check_dedup_args(args) -> Optional[str]:
    """-> an error message for an unusable --dedup-threshold, else None."""
    if args.dedup_threshold is None:
        return None
    if not (0.0 < args.dedup_threshold <= 1.0):               # (also rejects nan)
        return f"--dedup-threshold {args.dedup_threshold}: the cosine at which a chunk counts as a duplicate must be in (0, 1]"
    if args.hybrid_alpha is not None and args.queries and not getattr(args, "hybrid_filters", False):
        return "--dedup-threshold cannot be combined with --hybrid-alpha and --queries: the BM25 keyword search has no row filter"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--dedup-threshold needs a single GPU rank: a rank sees only its own rows, and a cross-rank join is out of scope"
    return None


def find_shard_duplicates(shard: "ShardSink", chunks: List[Dict], threshold: float, output_dir: str = "./embeddings_saved") -> np.ndarray:
    """`--dedup-threshold`: the self-join over the fp16 rows the encode step left in HBM (`dedup.find_duplicates`), `duplicates.json`
    beside the other output files (`threshold`, `n_chunks`, `n_duplicates`, `duplicates`: one `{index, chunk_id, duplicate_of_index,
    duplicate_of, score}` per flagged chunk, pointing at its nearest earlier chunk) -> the rows to keep, bool [n]."""
    from .dedup import duplicate_entries, find_duplicates
    from .index import ShardIndex
    n = int(shard.rows.shape[0])
    dup_of, scores = find_duplicates(ShardIndex(shard.rows, idx_base=0), threshold) if n else (np.zeros(0, np.int64), np.zeros(0, np.float32))
    entries = duplicate_entries(dup_of, scores, [c.get("chunk_id", f"chunk_{shard.lo + j}") for j, c in enumerate(chunks)], base=shard.lo)
    with open(Path(output_dir) / "duplicates.json", "w", encoding="utf-8") as fh:
        json.dump({"threshold": float(threshold), "n_chunks": n, "n_duplicates": len(entries), "duplicates": entries}, fh, indent=2,
                  ensure_ascii=False)
    print(f"✅ Near-duplicates at cosine >= {threshold}: {len(entries):,} of {n:,} chunks listed in {Path(output_dir) / 'duplicates.json'}")
    return dup_of < 0


def check_facets_args(args) -> Optional[str]:
    """-> an error message for an unusable --facets / --facets-top, else None.  On success `args.facet_keys` holds the keys (None
    without --facets).  (The other flags are read with getattr: absent = off.)"""
    args.facet_keys = None
    if getattr(args, "facets", None) is None:
        if getattr(args, "facets_top", 10) != 10:
            return f"--facets-top {args.facets_top} needs --facets: it counts the values listed per key"
        return None
    keys = [k.strip() for k in args.facets.split(",")]
    if not all(keys):
        return f"--facets {args.facets!r}: metadata keys separated by commas, e.g. section,paper_id"
    if not getattr(args, "queries", None):
        return "--facets needs --queries: it counts under the filters of the search step"
    if getattr(args, "facets_top", 10) < 1:
        return f"--facets-top {args.facets_top}: at least one value per key"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--facets needs a single GPU rank: ranks number their strings separately, and a per-rank top list cannot be merged exactly"
    args.facet_keys = keys
    return None


def check_ivf_args(args) -> Optional[str]:
    """-> an error message for an unusable --ivf-lists / --ivf-iters / --nprobe, else None.  (The other flags are read with getattr:
    absent = off.)"""
    lists, nprobe = getattr(args, "ivf_lists", None), getattr(args, "nprobe", None)
    if lists is None and nprobe is None:
        return None
    if lists is None or nprobe is None:
        return "--ivf-lists and --nprobe go together: the lists to build and how many of them a query probes"
    if not (1 <= lists <= 4096):
        return f"--ivf-lists {lists} must be in [1, 4096]"
    if not (1 <= nprobe <= min(128, lists)):
        return f"--nprobe {nprobe} must be in [1, min(128, --ivf-lists)] = [1, {min(128, lists)}]"
    if getattr(args, "ivf_iters", 10) < 1:
        return f"--ivf-iters {args.ivf_iters}: at least one iteration"
    if not getattr(args, "queries", None):
        return "--nprobe needs --queries: it is a mode of the search step"
    if getattr(args, "hybrid_alpha", None) is not None:
        return "--nprobe cannot be combined with --hybrid-alpha: the BM25 keyword search has no inverted lists of topics"
    if getattr(args, "group_by_paper", False):
        return "--nprobe cannot be combined with --group-by-paper: the grouped search reads every row"
    if getattr(args, "min_score", None) is not None:
        return "--nprobe cannot be combined with --min-score: the range search reads every row"
    if getattr(args, "where_filters", None) is not None:
        return "--nprobe cannot be combined with --where-file: the IVF search takes one bitmap per call"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--nprobe needs a single GPU rank: more than one rank is out of scope"
    return None


def _check_candidate_scan_args(args, flag: str, r, codes: str, scan: str, also=(), limit: int = 256) -> Optional[str]:
    """The refusals the row-choosing modes of the search step share (--binary-candidates, --pq-candidates, --graph-ef): `r` the flag's
    value (at most `limit`), `codes` / `scan` the mode's words for what it keeps and its scan, `also` further (flag, on, why) refusals
    placed after --nprobe."""
    if not (1 <= r <= limit):
        return f"{flag} {r} must be in [1, {limit}]"
    if not getattr(args, "queries", None):
        return f"{flag} needs --queries: it is a mode of the search step"
    for other, on, why in (
            ("--nprobe / --ivf-lists", getattr(args, "nprobe", None) is not None or getattr(args, "ivf_lists", None) is not None,
             "both choose which rows get scored"),
            *also,
            ("--hybrid-alpha", getattr(args, "hybrid_alpha", None) is not None, f"the BM25 keyword search has no {codes}"),
            ("--group-by-paper", getattr(args, "group_by_paper", False), "the grouped search reads every row"),
            ("--min-score", getattr(args, "min_score", None) is not None, "the range search reads every row"),
            ("--where-file", getattr(args, "where_filters", None) is not None, f"{scan} takes one bitmap per call")):
        if on:
            return f"{flag} cannot be combined with {other}: {why}"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return f"{flag} needs a single GPU rank: more than one rank is out of scope"
    width = getattr(args, "top_k", 10)
    if getattr(args, "rerank_model", None):
        width = getattr(args, "rerank_top_k", 32)
    elif getattr(args, "mmr_lambda", None) is not None:
        width = getattr(args, "mmr_fetch_k", 32)
    if r < width:
        return f"{flag} {r} is below the {width} rows the search returns per query"
    return None


def check_binary_args(args) -> Optional[str]:
    """-> an error message for an unusable --binary-candidates, else None.  (The other flags are read with getattr: absent = off.)"""
    r = getattr(args, "binary_candidates", None)
    if r is None:
        return None
    return _check_candidate_scan_args(args, "--binary-candidates", r, "binary codes", "the Hamming scan")


def check_pq_args(args) -> Optional[str]:
    """-> an error message for an unusable --pq-candidates / --pq-dsub, else None.  (The other flags are read with getattr: absent = off.)"""
    r = getattr(args, "pq_candidates", None)
    if r is None:
        return None
    if 1 <= r <= 256 and getattr(args, "pq_dsub", 8) not in (4, 8, 16, 32, 64):
        return f"--pq-dsub {getattr(args, 'pq_dsub', 8)} must be a power of two in [4, 64]"
    return _check_candidate_scan_args(
        args, "--pq-candidates", r, "PQ codes", "the code scan",
        also=(("--binary-candidates", getattr(args, "binary_candidates", None) is not None, "both choose which rows get scored"),
              ("--boost-key", getattr(args, "boost_key", None) is not None, "the boosted search reads every row")))


def check_graph_args(args) -> Optional[str]:
    """-> an error message for an unusable --graph-ef / --graph-degree / --graph-entries, else None.  (The other flags are read with
    getattr: absent = off.)"""
    ef = getattr(args, "graph_ef", None)
    if ef is None:
        return None
    if not (1 <= ef <= 512):
        return f"--graph-ef {ef} must be in [1, 512]"
    degree, entries = getattr(args, "graph_degree", 32), getattr(args, "graph_entries", 8)
    if degree not in (8, 16, 24, 32):
        return f"--graph-degree {degree} must be a multiple of 8 in [8, 32]"
    if not (1 <= entries <= 32):
        return f"--graph-entries {entries} must be in [1, 32]"
    return _check_candidate_scan_args(
        args, "--graph-ef", ef, "graph", "the graph search", limit=512,
        also=(("--binary-candidates", getattr(args, "binary_candidates", None) is not None, "both choose which rows get scored"),
              ("--pq-candidates", getattr(args, "pq_candidates", None) is not None, "both choose which rows get scored"),
              ("--boost-key", getattr(args, "boost_key", None) is not None, "the boosted search reads every row")))


def boost_spec_of(args) -> Optional[Dict]:
    """The `boost.prior_from_metadata` spec the --boost-* flags name, None without --boost-key."""
    if getattr(args, "boost_key", None) is None:
        return None
    spec = {"key": args.boost_key, "missing": 0.0}
    if getattr(args, "boost_decay_origin", None) is not None:
        spec.update(decay="exp", origin=args.boost_decay_origin, half_life=args.boost_half_life)
    return spec


def check_boost_args(args) -> Optional[str]:
    """-> an error message for unusable --boost-* flags, else None.  (The other flags are read with getattr: absent = off.)"""
    key, w = getattr(args, "boost_key", None), getattr(args, "boost_weight", None)
    origin, half = getattr(args, "boost_decay_origin", None), getattr(args, "boost_half_life", None)
    if key is None and w is None and origin is None and half is None:
        return None
    if key is None or w is None:
        return "--boost-key and --boost-weight go together (and --boost-decay-origin / --boost-half-life need both)"
    if (origin is None) != (half is None):
        return "--boost-decay-origin and --boost-half-life go together"
    if not np.isfinite(np.float32(w)):
        return f"--boost-weight {w} must be finite"
    if half is not None and not (half > 0 and np.isfinite(half) and np.isfinite(origin)):
        return f"--boost-half-life {half} must be positive and finite, --boost-decay-origin finite"
    if not getattr(args, "queries", None):
        return "--boost-key needs --queries: it is a mode of the search step"
    for flag, on in (("--hybrid-alpha", getattr(args, "hybrid_alpha", None) is not None), ("--group-by-paper", getattr(args, "group_by_paper", False)),
                     ("--min-score", getattr(args, "min_score", None) is not None),
                     ("--nprobe / --ivf-lists", getattr(args, "nprobe", None) is not None or getattr(args, "ivf_lists", None) is not None),
                     ("--binary-candidates", getattr(args, "binary_candidates", None) is not None),
                     ("--where-file", getattr(args, "where_filters", None) is not None)):
        if on:
            return f"--boost-key cannot be combined with {flag}: a boosted variant of that search is out of scope"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--boost-key needs a single GPU rank: more than one rank is out of scope"
    return None


def check_topics_args(args) -> Optional[str]:
    """-> an error message for an unusable --topics / --topics-iters, else None.  (The other flags are read with getattr: absent = off.)"""
    if getattr(args, "topics", None) is None:
        return None
    if not (1 <= args.topics <= 4096):
        return f"--topics {args.topics} must be in [1, 4096]"
    if getattr(args, "topics_iters", 20) < 1:
        return f"--topics-iters {args.topics_iters}: at least one iteration"
    if not getattr(args, "queries", None):
        return "--topics needs --queries: it clusters under the filters of the search step"
    if getattr(args, "where_filters", None) is not None:
        return "--topics cannot be combined with --where-file: it clusters one set of chunks"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--topics needs a single GPU rank: a rank sees only its own rows"
    return None


def topic_clusters(chunks: List[Dict], shard: "ShardSink", n_topics: int, iters: int = 20, seed: int = 0, where=None,
                   where_document: Optional[Dict] = None, *, keep_mask: Optional[np.ndarray] = None, where_on_device: bool = False,
                   document_regex: bool = False, representatives: int = 3, output_dir: str = "./embeddings_saved"):
    """`--topics`: spherical k-means (`topics.fit_shard`, INTEGRATION.md "Topics") over the fp16 rows the encode step left in HBM, under
    the row filters the search step uses (`retrieval.RowFilters`: `where`, `where_document`, `keep_mask`), written to `topics.json`
    beside the other output files: `{n_topics, iters, seed, sizes, objective, iterations, representatives}`, the representatives being
    each topic's nearest allowed chunks as chunk ids.  -> what was written."""
    from . import topics as T
    from .index import ShardIndex
    from .retrieval import RowFilters
    metadata = [c.get("metadata") or {} for c in chunks]
    filters = RowFilters(metadata, shard.rows.device, keep_mask=keep_mask, texts=lambda: [c.get("text") or "" for c in chunks],
                         where_on_device=where_on_device, document_regex=document_regex)
    allow, _ = filters.allow_of(where, where_document)
    res = T.fit_shard(ShardIndex(shard.rows, idx_base=0), allow, n_topics, iters=iters, seed=seed, representatives=representatives)
    out = {"n_topics": int(n_topics), "iters": int(iters), "seed": int(seed), "sizes": res["sizes"].tolist(), "objective": res["objective"],
           "iterations": res["iterations"],
           "representatives": [[chunks[int(r)].get("chunk_id", f"chunk_{shard.lo + int(r)}") for r in rows if r >= 0] for rows in res["rep_rows"]]}
    with open(Path(output_dir) / "topics.json", "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=2, ensure_ascii=False)
    print(f"✅ {n_topics} topics over {int(res['sizes'].sum())} chunks written to {Path(output_dir) / 'topics.json'}")
    return out


def facet_counts(chunks: List[Dict], device, keys: Sequence[str], top: int = 10, where=None, where_document: Optional[Dict] = None, *,
                 keep_mask: Optional[np.ndarray] = None, where_on_device: bool = False, document_regex: bool = False,
                 output_dir: str = "./embeddings_saved"):
    """`--facets`: the facet counts of `keys` (`facets.count`, INTEGRATION.md "Facet counts") over the metadata of `chunks`, under the
    row filters the search step uses (`retrieval.RowFilters`: `where`, `where_document`, `keep_mask`), written to `facets.json` beside
    the other output files: `{"keys", "top", "facets"}`, `facets` being one list of per-key results (`{key, values, counts, distinct,
    missing, unbinned, total}`), or with a per-query `where` list one such list per entry.  -> what was written under `facets`."""
    from . import facets as F
    from .retrieval import RowFilters
    from .where_device import MetadataColumns
    metadata = [c.get("metadata") or {} for c in chunks]
    n = len(chunks)
    filters = RowFilters(metadata, device, 0, n, keep_mask=keep_mask, texts=lambda: [c["text"] for c in chunks],
                         where_on_device=where_on_device, document_regex=document_regex)
    cols = filters.columns() if where_on_device else MetadataColumns(metadata, 0, n, device)
    if isinstance(where, (list, tuple)):
        bitmaps, filter_of, _ = filters.per_query(len(where), where, where_document)
        per_filter = F.count(cols, list(keys), bitmaps, top)
        result = [per_filter[f] for f in filter_of]
    else:
        allow, _ = filters.allow_of(where, where_document)
        result = F.count(cols, list(keys), allow, top)[0]
    with open(Path(output_dir) / "facets.json", "w", encoding="utf-8") as fh:
        json.dump({"keys": list(keys), "top": top, "facets": result}, fh, indent=2, ensure_ascii=False)
    print(f"✅ Facet counts of {', '.join(keys)} written to {Path(output_dir) / 'facets.json'}")
    return result


GROUP_MAX_PAPERS, GROUP_MAX_CHUNKS = 32, 8    # arx_topk_search_grouped: papers per query (the search's k limit), chunks per paper


def check_group_args(args) -> Optional[str]:
    """-> an error message for an unusable --group-by-paper / --chunks-per-paper, else None."""
    if not args.group_by_paper:
        if args.chunks_per_paper != 1:
            return f"--chunks-per-paper {args.chunks_per_paper} needs --group-by-paper: it counts the chunks returned for each paper"
        return None
    if not args.queries:
        return "--group-by-paper needs --queries: it groups the results of the search step"
    if args.rerank_model:
        return "--group-by-paper cannot be combined with --rerank-model: the cross-encoder ranks chunks, not papers"
    if args.hybrid_alpha is not None:
        return "--group-by-paper cannot be combined with --hybrid-alpha: the BM25 keyword search has no groups"
    if args.mmr_lambda is not None:
        return "--group-by-paper cannot be combined with --mmr-lambda: MMR re-orders the cosine search's chunk candidates only"
    if getattr(args, "where_file", None) is not None:
        return "--group-by-paper cannot be combined with --where-file: the grouped search takes one filter per call"
    if not (1 <= args.top_k <= GROUP_MAX_PAPERS):
        return f"--top-k {args.top_k}: the grouped search returns between 1 and {GROUP_MAX_PAPERS} papers per query"
    if not (1 <= args.chunks_per_paper <= GROUP_MAX_CHUNKS):
        return f"--chunks-per-paper {args.chunks_per_paper}: the grouped search returns between 1 and {GROUP_MAX_CHUNKS} chunks per paper"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--group-by-paper needs a single GPU rank: a paper may straddle two ranks, and a cross-rank fold is out of scope"
    return None


RANGE_MAX_TOP_K = 1024     # arx_range_search: rows per query


def check_range_args(args) -> Optional[str]:
    """-> an error message for an unusable --min-score, else None.  (The other flags are read with getattr: absent = off.)"""
    min_score = getattr(args, "min_score", None)
    if min_score is None:
        return None
    if min_score != min_score:
        return f"--min-score {min_score}: the threshold must be a number (use -inf for \"every chunk\")"
    if not getattr(args, "queries", None):
        return "--min-score needs --queries: it is a threshold on the results of the search step"
    if getattr(args, "rerank_model", None):
        return "--min-score cannot be combined with --rerank-model: reranking a long range list is out of scope for the CLI"
    if getattr(args, "hybrid_alpha", None) is not None:
        return "--min-score cannot be combined with --hybrid-alpha: the BM25 keyword search has no score threshold"
    if getattr(args, "mmr_lambda", None) is not None:
        return "--min-score cannot be combined with --mmr-lambda: MMR picks among at most 32 candidates of the top-k search"
    if getattr(args, "group_by_paper", False):
        return "--min-score cannot be combined with --group-by-paper: the grouped search ranks papers, not chunks above a threshold"
    if getattr(args, "where_file", None) is not None:
        return "--min-score cannot be combined with --where-file: the range search takes one filter per call"
    top_k = getattr(args, "top_k", 10)
    if not (1 <= top_k <= RANGE_MAX_TOP_K):
        return f"--top-k {top_k}: with --min-score the search returns between 1 and {RANGE_MAX_TOP_K} chunks per query"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--min-score needs a single GPU rank: a cross-rank merge of lists of up to 1024 rows is out of scope"
    return None


def check_where_args(args) -> Optional[str]:
    """-> an error message for an unusable --where, else None.  On success `args.where_filter` holds the parsed filter (None without --where)."""
    args.where_filter = None
    if args.where is None:
        return None
    if args.hybrid_alpha is not None and not getattr(args, "hybrid_filters", False):
        return "--where cannot be combined with --hybrid-alpha: the BM25 keyword search has no row filter"
    try:
        parsed = json.loads(args.where)
    except ValueError as e:
        return f"--where is not valid JSON: {e}"
    from .where import compile_where
    try:
        compile_where(parsed)
    except ValueError as e:
        return f"--where: {e}"
    args.where_filter = parsed
    return None


def read_query_lines(path) -> List[str]:
    """The queries of --queries: the file's non-empty lines, stripped."""
    return [ln.strip() for ln in Path(path).read_text(encoding="utf-8").splitlines() if ln.strip()]


def check_where_file_args(args) -> Optional[str]:
    """-> an error message for an unusable --where-file, else None.  On success `args.where_filters` holds one parsed filter or None per
    query of --queries (None without --where-file)."""
    args.where_filters = None
    if getattr(args, "where_file", None) is None:
        return None
    if args.where is not None:
        return "--where-file cannot be combined with --where: the file holds the filter of every query"
    if args.hybrid_alpha is not None and not getattr(args, "hybrid_filters", False):
        return "--where-file cannot be combined with --hybrid-alpha: the BM25 keyword search has no row filter"
    if not args.queries:
        return "--where-file needs --queries: it holds one filter per query"
    try:
        lines = [ln.strip() for ln in Path(args.where_file).read_text(encoding="utf-8").splitlines() if ln.strip()]
        n_queries = len(read_query_lines(args.queries))
    except OSError as e:
        return f"--where-file: {e}"
    from .where import compile_where
    filters = []
    for no, ln in enumerate(lines, 1):
        try:
            parsed = json.loads(ln)
        except ValueError as e:
            return f"--where-file line {no} is not valid JSON: {e}"
        if parsed is not None:
            if not isinstance(parsed, dict):
                return f"--where-file line {no}: a filter object or null, got {ln}"
            try:
                compile_where(parsed)
            except ValueError as e:
                return f"--where-file line {no}: {e}"
        filters.append(parsed)
    if len(filters) != n_queries:
        return f"--where-file holds {len(filters)} filters for the {n_queries} queries of --queries: it needs one line per query"
    args.where_filters = filters
    return None


def check_where_device_args(args) -> Optional[str]:
    """-> an error message for an unusable --where-on-device, else None."""
    if not getattr(args, "where_on_device", False):
        return None
    if args.where is None and getattr(args, "where_file", None) is None:
        return "--where-on-device needs --where or --where-file: it chooses where those filters are evaluated"
    return None


def check_where_document_args(args) -> Optional[str]:
    """-> an error message for an unusable --where-document, else None.  On success `args.where_document_filter` holds the parsed filter
    (None without --where-document)."""
    args.where_document_filter = None
    if args.where_document is None:
        if getattr(args, "where_document_regex", False):
            return "--where-document-regex needs --where-document: the filter still arrives through it"
        return None
    if args.hybrid_alpha is not None and not getattr(args, "hybrid_filters", False):
        return "--where-document cannot be combined with --hybrid-alpha: the BM25 keyword search has no row filter"
    try:
        parsed = json.loads(args.where_document)
    except ValueError as e:
        return f"--where-document is not valid JSON: {e}"
    from .where_document import compile_where_document
    try:
        compile_where_document(parsed, regex=getattr(args, "where_document_regex", False))
    except ValueError as e:
        return f"--where-document: {e}"
    args.where_document_filter = parsed
    return None


def main(argv: Optional[Sequence[str]] = None, model_factory: Optional[Callable] = None) -> int:
    global _model, _model_name
    args = build_parser().parse_args(argv)
    err = (check_rerank_args(args) or check_hybrid_args(args) or check_hybrid_filters_args(args) or check_hybrid_device_args(args) or check_keyword_build_args(args) or check_where_args(args) or check_where_file_args(args) or check_where_device_args(args)
           or check_where_document_args(args)
           or check_mmr_args(args) or check_dedup_args(args) or check_group_args(args) or check_range_args(args) or check_facets_args(args) or check_topics_args(args) or check_ivf_args(args)
           or check_binary_args(args) or check_pq_args(args) or check_graph_args(args) or check_boost_args(args))
    if err:
        print(f"Error: {err}")
        return 2
    input_dir = Path(args.input_dir)
    if not input_dir.exists():
        print(f"Error: Directory {input_dir} not found")
        return 1
    if args.model_dir:
        os.environ["ARX_MODEL_DIR"] = args.model_dir
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        init_distributed()
    cpu_count = effective_cpus()                                # usable by this job (cgroup quota), not the machine's logical CPUs
    print("=" * 80)
    print("PARALLEL EMBEDDING GENERATION - MI355X")
    print("=" * 80)
    print(f"\nSystem: {cpu_count} CPU cores, {world} GPU rank(s)")
    print("Configuration:")
    print(f"  Model: {args.model}")
    print(f"  Min quality: {args.min_quality}")
    print(f"  Batch size: {args.batch_size}")
    print(f"  Load workers: {args.load_workers or default_load_workers()}")
    print(f"  Store batch size: {args.store_batch_size}")
    print(f"  ChromaDB: {args.chroma_db}\n")
    meta_prefetch = None
    try:
        t_start = time.time()
        span = None
        if world > 1:
            # per-rank loading: every rank parses its slice of the sorted file list and ends up holding only the chunks it encodes
            rc_ = load_chunks_for_rank(input_dir, args.min_quality, args.load_workers, args.chunks_per_worker, world, rank)
            chunks, span, n_chunks = rc_.chunks, (rc_.lo, rc_.hi, rc_.total), rc_.total
        else:
            chunks = load_chunks_parallel(input_dir, min_quality=args.min_quality, num_workers=args.load_workers)
            n_chunks = len(chunks)
        if not n_chunks:
            print("No chunks found!")
            return 1
        load_time = time.time() - t_start
        print(f"Loading completed in {load_time:.1f} seconds\n")
        try:
            _model, _model_name = None, None
            init_worker_model(args.model, model_factory)
        except (ImportError, FileNotFoundError, OSError, RuntimeError) as e:
            print(f"Error: embedding backend not available: {e}")
            return 1
        # metadata.json is serialised beside the GPU work (this rank's entries when the chunks are per rank); renamed into place by the writer
        if span is not None:
            meta_prefetch = MetadataPrefetch(chunks, "./embeddings_saved", first_index=span[0], fragment_of_rank=rank)
            meta_prefetch.start()
        elif rank == 0:
            meta_prefetch = MetadataPrefetch(chunks, "./embeddings_saved")
            meta_prefetch.start()
        t0 = time.time()
        qs = []
        if args.queries:
            qs = read_query_lines(args.queries)
        # the search step works on the rows where the encoder leaves them: an fp16 shard in this rank's HBM
        sink = make_shard_sink(_model, n_chunks, args.chunks_per_worker, world, rank) if (qs or args.dedup_threshold is not None) else None
        if world > 1:
            # one process per GPU: every rank encodes, keeps and writes its own contiguous row range
            embeddings, lo, hi = generate_embeddings_sharded(chunks, args.model, args.batch_size, args.chunks_per_worker, sink=sink, span=span)
        else:
            embeddings = generate_embeddings_parallel(chunks, model_name=args.model, batch_size=args.batch_size,
                                                      num_workers=args.embedding_workers, chunks_per_worker=args.chunks_per_worker,
                                                      sink=sink)
        embedding_time = time.time() - t0
        print(f"Embedding generation completed in {embedding_time:.1f} seconds ({embedding_time / 60:.1f} min)\n")
        if world > 1:
            save_embeddings_sharded(chunks, embeddings, lo, hi, output_dir="./embeddings_saved", out_dtype=args.out_dtype,
                                    prefetch=meta_prefetch, total=n_chunks)
        elif rank == 0:
            print("Saving embeddings to disk as backup...")
            save_embeddings_to_disk_fallback(chunks, embeddings, output_dir="./embeddings_saved", out_dtype=args.out_dtype,
                                             prefetch=meta_prefetch)
            print()
        meta_prefetch = None
        keep_mask = None
        if args.dedup_threshold is not None:
            if sink is None:
                print("⚠️  --dedup-threshold needs the HIP encoder (the self-join runs over the shard it leaves in HBM): skipped")
            else:
                keep_mask = find_shard_duplicates(sink, chunks, args.dedup_threshold)
        if qs:
            if sink is None:
                print("⚠️  --queries needs the HIP encoder (the search step runs over the shard it leaves in HBM): skipped")
            else:
                reranker = None
                if args.rerank_model:
                    from .rerank import HipCrossEncoder
                    reranker = HipCrossEncoder.from_dir(args.rerank_model, device=_model.encoder.device)
                search_queries(_model, chunks, sink, qs, top_k=args.top_k, chunk_base=span[0] if span else 0,
                               reranker=reranker, rerank_top_k=args.rerank_top_k, hybrid_alpha=args.hybrid_alpha,
                               where=args.where_filters if args.where_filters is not None else args.where_filter, where_document=args.where_document_filter,
                               mmr_lambda=args.mmr_lambda, mmr_fetch_k=args.mmr_fetch_k, keep_mask=keep_mask,
                               **({"group_by_paper": True, "chunks_per_paper": args.chunks_per_paper} if args.group_by_paper else {}),
                               **({"where_on_device": True} if args.where_on_device else {}),
                               **({"min_score": args.min_score} if args.min_score is not None else {}),
                               **({"hybrid_filters": True} if args.hybrid_filters else {}),
                               **({"hybrid_on_device": True} if args.hybrid_on_device else {}),
                               **({"keyword_build_on_device": True} if args.keyword_build_on_device else {}),
                               **({"document_regex": True} if args.where_document_regex else {}),
                               **({"nprobe": args.nprobe, "ivf_lists": args.ivf_lists, "ivf_iters": args.ivf_iters, "ivf_seed": args.ivf_seed}
                                  if args.nprobe is not None else {}),
                               **({"binary_candidates": args.binary_candidates, "binary_centre": args.binary_centre}
                                  if args.binary_candidates is not None else {}),
                               **({"pq_candidates": args.pq_candidates, "pq_dsub": args.pq_dsub, "pq_centre": args.pq_centre}
                                  if args.pq_candidates is not None else {}),
                               **({"graph_ef": args.graph_ef, "graph_degree": args.graph_degree, "graph_entries": args.graph_entries}
                                  if args.graph_ef is not None else {}),
                               **({"boost_spec": boost_spec_of(args), "boost_weight": args.boost_weight} if args.boost_key is not None else {}))
                if args.facet_keys is not None:
                    facet_counts(chunks, _model.encoder.device, args.facet_keys, args.facets_top,
                                 where=args.where_filters if args.where_filters is not None else args.where_filter,
                                 where_document=args.where_document_filter, keep_mask=keep_mask, where_on_device=args.where_on_device,
                                 document_regex=args.where_document_regex)
                if args.topics is not None:
                    topic_clusters(chunks, sink, args.topics, args.topics_iters, args.topics_seed, where=args.where_filter,
                                   where_document=args.where_document_filter, keep_mask=keep_mask, where_on_device=args.where_on_device,
                                   document_regex=args.where_document_regex)
        store_time = 0.0
        if rank == 0 and not args.skip_chroma:
            try:
                import chromadb                                        # noqa: F401
            except ImportError:
                print("Error: chromadb not available")
                print("Install with: pip install chromadb")
                return 1
            t0 = time.time()
            if world > 1:                       # rank 0 only holds its shard: ingest from the files all ranks just wrote
                embeddings = np.load(Path("./embeddings_saved") / "embeddings.npy", mmap_mode="r")
                chunks = load_chunks_parallel(input_dir, min_quality=args.min_quality, num_workers=args.load_workers)
            try:
                store_in_chroma_batched(chunks, embeddings, db_path=args.chroma_db, collection_name=args.collection_name,
                                        batch_size=args.store_batch_size)
                store_time = time.time() - t0
                print(f"Storage completed in {store_time:.1f} seconds")
            except Exception as e:                                     # noqa: BLE001
                store_time = time.time() - t0
                print(f"⚠️  ChromaDB storage failed after {store_time:.1f} seconds: {e}")
                print("✅ Embeddings are safely saved to ./embeddings_saved/")
        total = time.time() - t_start
        print("\n" + "=" * 80)
        print("EMBEDDING GENERATION COMPLETE")
        print("=" * 80)
        print(f"Chunks processed: {n_chunks:,}")
        print(f"Embeddings generated: {n_chunks if world > 1 else len(embeddings):,}")
        if len(embeddings):
            print(f"Embedding dimensions: {len(embeddings[0])}")
        print(f"Stored in: {args.chroma_db}\n")
        print("Timing:")
        print(f"  Loading: {load_time:.1f}s")
        print(f"  Embedding: {embedding_time:.1f}s ({embedding_time / 60:.1f} min)")
        print(f"  Storage: {store_time:.1f}s")
        print(f"  Total: {total:.1f}s ({total / 60:.1f} min)")
        print("=" * 80)
        return 0
    except KeyboardInterrupt:
        print("\n\n⚠️  Process interrupted by user")
        return 1
    except Exception as e:                                             # noqa: BLE001
        print(f"\n\n❌ Fatal error: {e}")
        traceback.print_exc()
        return 1
    finally:
        if meta_prefetch is not None:            # the run ended before the writer took the file: nothing half-written stays behind
            meta_prefetch.discard()


if __name__ == "__main__":
    sys.exit(main())
