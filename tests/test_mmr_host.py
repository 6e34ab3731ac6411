"""Host side of MMR retrieval, no GPU: the float64 definition on a hand-worked case and on the cluster construction, the CLI flags and their
refusals, the C-ABI declarations, and the candidate-row exchange over a world-2 gloo group."""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd.mmr import cosines_f64, mmr_reference_f64
from tests.mmr_cases import LADDER_PERM, cluster_case, ladder_case

ROOT = Path(__file__).resolve().parents[1]


def _cosd(deg):
    return math.cos(math.radians(deg))


def test_reference_on_a_hand_worked_case():
    """q at 0 degrees; slots at 10, 10 (the same vector: a tie), -20, 50, 0 (id -1: never picked, though it is the most relevant) and 90
    degrees.  rel = cos(angle), sim = cos(angle difference); the expected picks and objectives below are worked out by hand from those."""
    ang = [10.0, 10.0, -20.0, 50.0, 0.0, 90.0]
    cand = np.array([[_cosd(a), math.sin(math.radians(a))] for a in ang])
    cand[1] = cand[0]
    q = np.array([1.0, 0.0])
    ids = np.array([7, 8, 9, 10, -1, 12])
    inf = math.inf
    # lam = 1: pure relevance; the tie of slots 0 and 1 goes to slot 0; five valid slots, so the sixth entry is (-1, -inf)
    o, v = mmr_reference_f64(q, cand, ids, 6, 1.0)
    assert o.tolist() == [[0, 1, 2, 3, 5, -1]]
    assert np.allclose(v[0, :5], [_cosd(10), _cosd(10), _cosd(20), _cosd(50), _cosd(90)], rtol=0, atol=1e-15) and v[0, 5] == -inf
    # lam = 0: every first objective is 0 -> the lowest VALID slot; then the slot least similar to the picks:
    #   after {10}: 90 (cos 80 = 0.17) < 50 (cos 40 = 0.77) < -20 (cos 30 = 0.87) < the duplicate (1)
    #   after {10, 90}: 50 -> max(cos 40, cos 40), -20 -> max(cos 30, cos 110): slot 3; then slot 2, then the duplicate
    o, v = mmr_reference_f64(q, cand, ids, 6, 0.0)
    assert o.tolist() == [[0, 5, 3, 2, 1, -1]]
    assert np.allclose(v[0, :5], [0.0, -_cosd(80), -_cosd(40), -_cosd(30), -1.0], rtol=0, atol=1e-15) and v[0, 5] == -inf
    # lam = 0.5: slot 0 (0.4924; tie with slot 1); then 0.5 (rel - max sim): slot 1 -0.0076, slot 2 0.5 (cos 20 - cos 30) = 0.0368,
    # slot 3 0.5 (cos 50 - cos 40) = -0.0616, slot 5 0.5 (0 - cos 80) = -0.0868 -> slot 2; -20 degrees is farther from slots 1, 3, 5 than 10 degrees is, so
    # their maxima stay and slot 1, then slot 3 follow; slot 5 is picked last, when its nearest pick is slot 3 (cos 40)
    o, v = mmr_reference_f64(q, cand, ids, 6, 0.5)
    assert o.tolist() == [[0, 2, 1, 3, 5, -1]]
    want = [0.5 * _cosd(10), 0.5 * (_cosd(20) - _cosd(30)), 0.5 * (_cosd(10) - 1.0), 0.5 * (_cosd(50) - _cosd(40)), 0.5 * (_cosd(90) - _cosd(40))]
    assert np.allclose(v[0, :5], want, rtol=0, atol=1e-15) and v[0, 5] == -inf
    # m below the number of valid slots: a prefix; no valid slot at all: only padding
    assert mmr_reference_f64(q, cand, ids, 2, 0.5)[0].tolist() == [[0, 2]]
    o, v = mmr_reference_f64(q, cand, np.full(6, -1), 3, 0.5)
    assert o.tolist() == [[-1, -1, -1]] and (v == -inf).all()
    # a zero row and a zero query: the cosine is 0, not nan
    cand0 = cand.copy()
    cand0[2] = 0.0
    rel, sim = cosines_f64(q, cand0)
    assert rel[2] == 0.0 and not sim[2].any() and not sim[:, 2].any() and np.isfinite(sim).all()
    assert not cosines_f64(np.zeros(2), cand)[0].any()
    with pytest.raises(ValueError):
        mmr_reference_f64(q, cand, ids, 7, 0.5)
    with pytest.raises(ValueError):
        mmr_reference_f64(q, cand, ids, 3, 1.5)


def test_reference_on_the_cluster_case():
    q, cand, ids = cluster_case()
    rel, sim = cosines_f64(q, cand)
    grp = np.arange(32) // 4
    same = grp[:, None] == grp[None, :]
    assert sim[same].min() >= 0.99 and np.abs(sim[~same]).max() <= 0.3
    assert (np.diff(rel) < 0).all()                             # relevance decreases with the position
    o, _ = mmr_reference_f64(q, cand, ids, 8, 0.5)
    assert sorted(grp[o[0]].tolist()) == list(range(8)), "lam = 0.5 must pick one row of every group"
    assert o[0].tolist() == [0, 4, 8, 12, 16, 20, 24, 28]
    o, _ = mmr_reference_f64(q, cand, ids, 8, 1.0)
    assert o[0].tolist() == list(range(8))
    # a batch is its queries one by one
    q2, c2, i2 = ladder_case(64)
    ob, vb = mmr_reference_f64(np.stack([q, q]), np.stack([cand, cand[::-1]]), np.stack([ids, ids]), 5, 0.5)
    assert ob[0].tolist() == [0, 4, 8, 12, 16] and ob[1].tolist() == [31, 27, 23, 19, 15]
    assert mmr_reference_f64(q2, c2, i2, 17, 1.0)[0][0].tolist() == np.argsort(np.array(LADDER_PERM)).tolist()


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_mmr_flags(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    p = GEN.build_parser()
    a = p.parse_args(["in"])
    assert a.mmr_lambda is None and a.mmr_fetch_k == 32 and a.top_k == 10
    assert GEN.check_mmr_args(a) is None
    assert GEN.check_mmr_args(p.parse_args(["in", "--mmr-fetch-k", "99"])) is None          # without --mmr-lambda the flag is not read
    assert GEN.check_mmr_args(p.parse_args(["in", "--mmr-lambda", "0.5", "--mmr-fetch-k", "16", "--top-k", "5"])) is None
    assert GEN.check_mmr_args(p.parse_args(["in", "--mmr-lambda", "0"])) is None and GEN.check_mmr_args(p.parse_args(["in", "--mmr-lambda", "1"])) is None
    refusals = [(["--mmr-lambda", "1.5"], "--mmr-lambda"), (["--mmr-lambda", "-0.1"], "--mmr-lambda"), (["--mmr-lambda", "nan"], "--mmr-lambda"),
                (["--mmr-lambda", "0.5", "--mmr-fetch-k", "33"], "--mmr-fetch-k"),
                (["--mmr-lambda", "0.5", "--mmr-fetch-k", "5", "--top-k", "6"], "--mmr-fetch-k"),
                (["--mmr-lambda", "0.5", "--top-k", "33"], "--top-k"),
                (["--mmr-lambda", "0.5", "--rerank-model", "m"], "--rerank-model"),
                (["--mmr-lambda", "0.5", "--hybrid-alpha", "0.5"], "--hybrid-alpha")]
    for argv, flag in refusals:
        msg = GEN.check_mmr_args(p.parse_args(["in"] + argv))
        assert msg and flag in msg and "--mmr-lambda" in msg + " ".join(argv), (argv, msg)
        assert GEN.main([str(tmp_path)] + argv) == 2, argv
        out = capsys.readouterr().out
        assert flag in out, (argv, out)


def test_search_queries_refuses_before_it_touches_the_model():
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    with pytest.raises(ValueError, match="hybrid_alpha"):
        GEN.search_queries(None, [], None, ["q"], mmr_lambda=0.5, hybrid_alpha=0.5)
    with pytest.raises(ValueError, match="reranker"):
        GEN.search_queries(None, [], None, ["q"], mmr_lambda=0.5, reranker=object())
    with pytest.raises(ValueError, match="mmr_lambda"):
        GEN.search_queries(None, [], None, ["q"], mmr_lambda=1.5)
    with pytest.raises(ValueError, match="mmr_fetch_k"):
        GEN.search_queries(None, [], None, ["q"], 10, mmr_lambda=0.5, mmr_fetch_k=33)
    with pytest.raises(ValueError, match="mmr_fetch_k"):
        GEN.search_queries(None, [], None, ["q"], 10, mmr_lambda=0.5, mmr_fetch_k=9)


def test_cabi_declares_and_exports_the_mmr_entry_points():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    for name in ("arx_gather_rows", "arx_mmr_select"):
        assert name in declared, f"{name} is not declared in include/arx.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    assert len(_lib.EXPORTS["arx_gather_rows"][1]) == 8 and len(_lib.EXPORTS["arx_mmr_select"][1]) == 11
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = _lib.load()
    assert hasattr(lib, "arx_gather_rows") and hasattr(lib, "arx_mmr_select")


# ---- world size 2 (gloo, CPU) ---------------------------------------------------------------------------------------------------------------
_WORKER = r'''
import os, sys, zlib
import numpy as np
sys.path.insert(0, os.environ["ARX_ROOT"])
import torch
import torch.distributed as dist
from arxiv_rag_amd.mmr import exchange_candidate_rows
from arxiv_rag_amd.index import shard_bounds
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rs = np.random.RandomState(0)
N, Q, n, D = 101, 5, 12, 64
corpus = (rs.standard_normal((N, D)) * rs.choice([1e-3, 1.0, 300.0], size=(N, 1))).astype(np.float16)
ids = np.stack([rs.choice(N, size=n, replace=False) for _ in range(Q)])
ids[1, -3:] = -1
lo, hi = shard_bounds(N, world, rank)
mine = (ids >= lo) & (ids < hi)                       # what arx_gather_rows leaves on this rank: its own rows, zeros elsewhere
rows = np.where(mine[..., None], corpus[np.clip(ids, 0, N - 1)], np.float16(0))
out = exchange_candidate_rows(torch.from_numpy(rows.copy()))
assert out.dtype == torch.float16 and tuple(out.shape) == (Q, n, D)
if rank == 0:
    print("RESULT", zlib.crc32(out.numpy().tobytes()), int((out.numpy() != 0).sum()))
dist.barrier()
dist.destroy_process_group()
'''


def _run_world(tmp_path, world):
    w = tmp_path / "worker.py"
    w.write_text(_WORKER)
    env = {**os.environ, "ARX_ROOT": str(ROOT), "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", f"--nproc-per-node={world}", "--master-port",
                        str(29740 + world), str(w)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0]


def test_exchange_candidate_rows_world_size_2_gloo_equals_world_1(tmp_path):
    """Exactly one rank holds each row and the other holds zeros, so the fp16 sum over the ranks is the single-process buffer bit for bit."""
    two, one = _run_world(tmp_path, 2), _run_world(tmp_path, 1)
    assert two == one and int(one.split()[2]) > 0
    # without a process group: the identity
    import torch
    from arxiv_rag_amd.mmr import exchange_candidate_rows
    t = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    assert exchange_candidate_rows(t) is t
