"""Constructed inputs and the float64 certificate shared by tests/test_mmr_host.py and tests/test_gpu_mmr.py (no test in here)."""
import math

import numpy as np

from arxiv_rag_amd.mmr import cosines_f64


def eps_of(dim):
    """The certificate's tolerance in cosine units, derived (not measured) — see test_gpu_mmr.test_certificate_against_float64."""
    return (2 * dim + 16) * 2.0 ** -24


def cluster_case(dim=64, dtype=np.float64):
    """32 candidates = 8 groups of 4 near-duplicates, relevance decreasing with the position 4 g + j.
    q = e_0; candidate (g, j) = cos(a) e_0 + sin(a) e_(1 + g) with a = 71 + 6.8 g + 2 j degrees: the members of a group lie within 6
    degrees of each other (cosine >= 0.9945), two groups share only the e_0 component (|cosine| = |cos a cos a'| <= 0.27), and
    rel = cos a falls from 0.33 to -0.57 in steps of at least 0.011 (0.033 inside a group).
    -> (q [dim], cand [32, dim], ids [32]) in `dtype`."""
    assert dim >= 9
    q = np.zeros(dim)
    q[0] = 1.0
    cand = np.zeros((32, dim))
    for g in range(8):
        for j in range(4):
            a = math.radians(71.0 + 6.8 * g + 2.0 * j)
            cand[4 * g + j, 0], cand[4 * g + j, 1 + g] = math.cos(a), math.sin(a)
    return q.astype(dtype), cand.astype(dtype), np.arange(100, 132, dtype=np.int64)


LADDER_PERM = [5, 12, 0, 9, 16, 3, 14, 7, 1, 10, 15, 4, 8, 13, 2, 11, 6]


def ladder_case(dim=64, dtype=np.float64):
    """17 candidates with relevances 0.9, 0.85, ..., 0.1 and nothing else in common: slot s = r q^ + sqrt(1 - r^2) e_(1 + s) with
    r = 0.9 - 0.05 LADDER_PERM[s], so sim[s][s'] = r r' and the relevance order is not the slot order."""
    assert dim >= 18
    q = np.zeros(dim)
    q[0] = 1.0
    cand = np.zeros((17, dim))
    for s, rank in enumerate(LADDER_PERM):
        r = 0.9 - 0.05 * rank
        cand[s, 0], cand[s, 1 + s] = r, math.sqrt(1.0 - r * r)
    return q.astype(dtype), cand.astype(dtype), np.arange(17, dtype=np.int64)


def step_gaps_f64(q, cand, ids, order, lam):
    """Per step of the float64 greedy pass along `order`: best objective minus second-best objective over the valid unpicked slots
    (inf where one slot is left)."""
    rel, sim = cosines_f64(q, cand)
    free = np.asarray(ids) >= 0
    worst = np.full(rel.shape[0], -np.inf)
    gaps = []
    for t, p in enumerate(order):
        obj = lam * rel if t == 0 else lam * rel - (1.0 - lam) * worst
        vals = np.sort(obj[free])[::-1]
        gaps.append(float(vals[0] - vals[1]) if vals.shape[0] > 1 else math.inf)
        free[p] = False
        worst = np.maximum(worst, sim[:, p])
    return gaps


def certify(q, cand, ids, order, mmr, lam, eps):
    """The float64 certificate of ONE query's answer (AssertionError if it does not hold).  At each step t, given the answer's own earlier
    picks: the pick is a valid unpicked slot whose float64 objective is within 2 eps of the best one, and the returned value is within
    eps of that objective; once no valid slot is left the answer is (-1, -inf)."""
    rel, sim = cosines_f64(q, cand)
    free = np.asarray(ids) >= 0
    worst = np.full(rel.shape[0], -np.inf)
    for t in range(len(order)):
        p = int(order[t])
        if not free.any():
            assert p == -1 and mmr[t] == -np.inf, f"step {t}: no valid slot is left but the answer is ({p}, {mmr[t]})"
            continue
        assert 0 <= p < rel.shape[0] and ids[p] >= 0, f"step {t}: slot {p} is not a valid slot"
        assert free[p], f"step {t}: slot {p} was picked before"
        obj = lam * rel if t == 0 else lam * rel - (1.0 - lam) * worst
        best = obj[free].max()
        assert obj[p] >= best - 2 * eps, f"step {t}: slot {p} has objective {obj[p]!r}, the best is {best!r} (2 eps = {2 * eps:.3e})"
        assert abs(float(mmr[t]) - obj[p]) <= eps, f"step {t}: returned {float(mmr[t])!r}, float64 objective {obj[p]!r} (eps = {eps:.3e})"
        free[p] = False
        worst = np.maximum(worst, sim[:, p])
