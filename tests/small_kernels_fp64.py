"""Plain references of the small kernels that sit between the large ones, written independently of the code under test (numpy and
Python lists only; no torch on the reference side):
  merge_ref      arx_topk_merge: all valid entries of all parts, sorted by (score desc, id asc), padded with (-inf, -1);
  max_norm_ref   arx_rows_max_norm_f16: the float64 maximum row norm of fp16 rows, and norm_window, the interval the kernel's
                 rounded-UP result must lie in;
  cosine_ref     arx_adjacent_cosine: float64 dot / (|a| |b|) of consecutive rows, with S = sum |a_i b_i| / (|a| |b|) for cosine_budget;
  bf16_rne_ref   arx_f32_to_bf16: round-to-nearest-even on the integer bit pattern;
  pool_ref       the pooled row: tests/helpers.py pool_fp64 (the encoder's float64 helper; there is one definition of it).
The optional `fault` of a reference computes a nearby WRONG operation, so that a test can show that the reference or its budget would
catch that mistake.  The seeded input builders of the CPU and the GPU tests live here too, so both test the same data."""
import math

import numpy as np

from tests.helpers import pool_fp64 as pool_ref  # noqa: F401  (re-exported)

U24 = 2.0 ** -24
MERGE_FAULTS = ("tie_high_id", "skip_last_part")
COSINE_FAULTS = ("drop_last4", "row+2")
BF16_FAULTS = ("trunc", "half_up", "add_7fff")


# ---- merge of partial top-k lists ------------------------------------------------------------------------------------------------------
def merge_ref(scores, ids, k, fault=None):
    """scores f32 [P, nq, kk], ids int64 [P, nq, kk] -> (f32 [nq, k], int64 [nq, k]).
    fault: "tie_high_id" (equal scores ordered by id descending), "skip_last_part" (part P - 1 never read)."""
    assert fault in (None,) + MERGE_FAULTS, fault
    P, nq, kk = scores.shape
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    parts = range(P - 1 if fault == "skip_last_part" else P)
    for q in range(nq):
        ent = [(float(scores[p, q, e]), int(ids[p, q, e])) for p in parts for e in range(kk) if ids[p, q, e] >= 0]
        ent = sorted(ent, key=(lambda t: (-t[0], -t[1])) if fault == "tie_high_id" else (lambda t: (-t[0], t[1])))
        for j, (s, i) in enumerate(ent[:k]):
            out_s[q, j], out_i[q, j] = s, i
    return out_s, out_i


def last_slot_start(P, k):
    """The merge kernel deals candidate c = part * k + entry to lane c % 64, slot c // 64: the first candidate of the last used slot."""
    return 64 * ((P * k - 1) // 64)


def merge_inputs(P, k, nq, seed, sort_lists=True):
    """Partial lists [P, nq, k] as the producers write them (each list sorted by score descending, empty entries (-inf, -1) last), ids
    distinct within a query and up to 2^40.  Query q plays role q % 6:
      0  continuous scores; the two best entries tie, the lower id in the LATER part (P = 1: in the later entry);
      1  every part empty;
      2  fewer than k valid entries overall;
      3  the best k entries all in the last slot of their lanes (only where that slot starts on a part boundary; else as role 5);
      4  scores from a small set of values: ties at every rank, across parts, lanes and slots;
      5  continuous scores; three entries of different parts tie exactly at rank k, ids descending with the part.
    Parts p % 5 == 3 are entirely empty in every query, and part p % 7 == 2 keeps only its first k // 2 entries.
    sort_lists=False: every list is shuffled afterwards (the kernel's contract does not need the order)."""
    rs = np.random.RandomState(seed)
    n = P * k
    s = np.empty((P, nq, k), np.float32)
    i = np.empty((P, nq, k), np.int64)
    for q in range(nq):
        role = q % 6
        pool = np.unique(np.concatenate([rs.randint(0, 2 ** 40, size=2 * n + 8), [0, 2 ** 40]]))
        assert len(pool) >= n
        qi = rs.permutation(pool)[:n].reshape(P, k).astype(np.int64)
        if q == 0:
            qi[P - 1, 0] = 2 ** 40 if 2 ** 40 not in qi else qi[P - 1, 0]
        qs = rs.standard_normal((P, k)).astype(np.float32)
        if role == 4:
            qs = rs.randint(0, max(2, n // 3), size=(P, k)).astype(np.float32)
        valid = np.ones((P, k), bool)
        for p in range(P):
            if P > 1 and p % 5 == 3:
                valid[p] = False
            if p % 7 == 2:
                valid[p, k // 2:] = False
        if role == 1:
            valid[:] = False
        if role == 2:
            valid[:] = False
            for c in rs.choice(n, size=min(n, max(0, k - 1 - (q // 6) % 3)), replace=False):
                valid[c // k, c % k] = True
        start = last_slot_start(P, k)
        if role == 3 and start % k == 0 and n - start >= k:
            valid[start // k:] = True
            qs[start // k:] += 100.0
        vp = [p for p in range(P) if valid[p].any()]
        if role == 0 and len(vp) >= 2:
            a, b = vp[0], vp[-1]
            ea, eb = int(np.argmax(valid[a])), int(np.argmax(valid[b]))
            qs[a, ea] = qs[b, eb] = 50.0
            lo, hi = sorted((int(qi[a, ea]), int(qi[b, eb])))
            qi[a, ea], qi[b, eb] = hi, lo
        if role == 0 and P == 1 and k >= 2 and valid[0, :2].all():
            qs[0, 0] = qs[0, 1] = 50.0
            qi[0, :2] = sorted(qi[0, :2].tolist(), reverse=True)
        if role == 5 and len(vp) >= 3 and valid.sum() > k:
            kth = np.sort(qs[valid])[::-1][k - 1]
            pick = [vp[0], vp[len(vp) // 2], vp[-1]]
            ent = [int(rs.choice(np.flatnonzero(valid[p]))) for p in pick]
            tid = sorted((int(qi[p, e]) for p, e in zip(pick, ent)), reverse=True)
            for (p, e), t in zip(zip(pick, ent), tid):
                qs[p, e], qi[p, e] = kth, t
        qs[~valid] = -np.inf
        qi[~valid] = -1
        for p in range(P):                                           # each list sorted descending, empty entries last
            o = np.argsort(-qs[p].astype(np.float64), kind="stable")
            if not sort_lists:
                o = rs.permutation(k)
            qs[p], qi[p] = qs[p][o], qi[p][o]
        s[:, q], i[:, q] = qs, qi
    return s, i


# ---- maximum row norm ------------------------------------------------------------------------------------------------------------------
def row_norms_ref(rows_f16):
    """float64 L2 norm of every fp16 row (exact products, float64 sums), in row chunks"""
    rows = np.asarray(rows_f16)
    assert rows.dtype == np.float16 and rows.ndim == 2
    out = np.empty(rows.shape[0], np.float64)
    step = max(1, (1 << 22) // rows.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, rows.shape[0], step):
            x = rows[a:a + step].astype(np.float64)
            out[a:a + step] = np.sqrt((x * x).sum(1))
    return out


def max_norm_ref(rows_f16):
    """float64 maximum row norm; NaN if any row holds a NaN"""
    nr = row_norms_ref(rows_f16)
    return float("nan") if np.isnan(nr).any() else float(nr.max())


def norm_window(ref, dim):
    """[lo, hi] for the kernel's rounded-up bound: ref <= got <= ref (1 + 2^-12)(1 + D 2^-24)(1 + 2^-22).  The factors: the kernel's own
    upward factor 1 + 2^-12; the bound on the fp32 sum of squares its comment states (relative error below D 2^-24; the square root
    halves it, the window keeps the whole); two f32 roundings (the square root and the product).  Derived, not measured."""
    return ref, ref * (1 + 2.0 ** -12) * (1 + dim * U24) * (1 + 2.0 ** -22)


def norm_pool(dim, seed, n=61):
    """fp16 rows [4 n, dim] of four families, n rows each, in this order: unit rows; norm 1e-3 (fp16-subnormal components at
    dim >= 768); norms log-uniform in [0.01, 8]; +-60 000 in every component."""
    rs = np.random.RandomState(seed)
    u = rs.standard_normal((3 * n, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[n:2 * n] *= 1e-3
    u[2 * n:] *= np.exp(rs.uniform(np.log(0.01), np.log(8.0), size=(n, 1)))
    big = 60000.0 * np.sign(rs.standard_normal((n, dim)))
    return np.concatenate([u, big], 0).astype(np.float16)


def emulate_max_norm_f32(rows_f16, fault=None):
    """The kernel's arithmetic in fp32 on the host (sequential fp32 sum of the exact squares, f32 square root, the upward factor).
    fault: "no_up_factor" (sqrt of the fp32 sum as it is), "first_512" (only columns < 512 are read)."""
    assert fault in (None, "no_up_factor", "first_512")
    x = np.asarray(rows_f16).astype(np.float32)
    if fault == "first_512":
        x = x[:, :512]
    best = np.float32(0)
    for r in x:
        best = max(best, np.cumsum(r * r, dtype=np.float32)[-1])
    nrm = np.sqrt(best, dtype=np.float32)
    return float(nrm) if fault == "no_up_factor" else float(np.float32(nrm * np.float32(1 + 1 / 4096)))


# ---- adjacent cosine -------------------------------------------------------------------------------------------------------------------
def cosine_ref(e, fault=None):
    """e f32 [n, D] -> (cos [n - 1], S [n - 1]) float64: cos_i = e_i . e_{i+1} / (|e_i| |e_{i+1}|) and S_i = sum_j |e_ij e_{i+1,j}| /
    (|e_i| |e_{i+1}|), the scale of the dot product's roundings.  A zero row gives NaN on both sides of it, as the quotient does.
    fault: "drop_last4" (the last 4 columns never read), "row+2" (row i + 2, clamped, instead of row i + 1)."""
    assert fault in (None,) + COSINE_FAULTS, fault
    x = np.asarray(e).astype(np.float64)
    n = x.shape[0]
    if n < 2:
        return np.zeros(0), np.zeros(0)
    a = x[:-1]
    b = x[np.minimum(np.arange(n - 1) + 2, n - 1)] if fault == "row+2" else x[1:]
    if fault == "drop_last4":
        a, b = a[:, :-4], b[:, :-4]
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1))
        return (a * b).sum(1) / den, np.abs(a * b).sum(1) / den


def cosine_budget(dim, S):
    """|kernel - cosine_ref| <= (ceil(D / 256) * 4 + 14) 2^-24 S per pair: a lane's chain of ceil(D / 256) * 4 fused multiply-adds, the
    six-step butterfly, two square roots, a product and a quotient.  Derived, not measured."""
    return (math.ceil(dim / 256) * 4 + 14) * U24 * S


def cosine_rows(n, dim, seed):
    """f32 [n, dim]: random rows of per-row scale in [1e-3, 1e3]; where n allows, rows (1, 2) identical, (3, 4) exactly negated, row 5
    all-positive before a +-halves row 6 (half of the components +1 / sqrt(D), half -1 / sqrt(D): the dot product's partial sums climb
    and cancel), and one zero row: row n // 2 (n >= 12) or row 0 (n == 6)."""
    rs = np.random.RandomState(seed)
    e = (rs.standard_normal((n, dim)) * np.exp(rs.uniform(np.log(1e-3), np.log(1e3), size=(n, 1)))).astype(np.float32)
    if n >= 3:
        e[2] = e[1]
    if n >= 5:
        e[4] = -e[3]
    if n >= 8:
        e[5] = np.abs(e[5])
        sign = np.where(rs.permutation(dim) < dim // 2, 1.0, -1.0)
        e[6] = (sign / np.sqrt(dim) + 0.01 * rs.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
    if n >= 12:
        e[n // 2] = 0
    elif n == 6:
        e[0] = 0
    return e


def emulate_cosine_f32(e):
    """a plain fp32 cosine (numpy float32 sums), standing in for a faithful kernel"""
    x = np.asarray(e, np.float32)
    a, b = x[:-1], x[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = (a * b).sum(1, dtype=np.float32)
        return dot / (np.sqrt((a * a).sum(1, dtype=np.float32)) * np.sqrt((b * b).sum(1, dtype=np.float32)))


# ---- f32 -> bf16 -------------------------------------------------------------------------------------------------------------------
def bf16_rne_ref(bits_u32, fault=None):
    """f32 bit patterns (uint32) -> bf16 bit patterns (uint16), round to nearest, ties to even, on the integers: add 0x7FFF plus the
    lowest kept bit, drop the low half.  A carry out of the mantissa moves to the next exponent, so a finite value above the largest
    bf16 becomes inf.  A NaN stays a NaN: its high half with the quiet bit set (the rounding could carry a payload away).
    fault: "trunc" (drop the low half), "half_up" (add 0x8000: ties away from zero), "add_7fff" (the rounding without the NaN case)."""
    assert fault in (None,) + BF16_FAULTS, fault
    b = np.asarray(bits_u32).astype(np.uint64)
    if fault == "trunc":
        return (b >> 16).astype(np.uint16)
    if fault == "half_up":
        return (((b + 0x8000) >> 16) & 0xFFFF).astype(np.uint16)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    if fault != "add_7fff":
        nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
        r = np.where(nan, (b >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def bf16_is_nan(h):
    h = np.asarray(h).astype(np.uint32)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def f32_is_nan(bits_u32):
    b = np.asarray(bits_u32).astype(np.uint64)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)


BF16_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def bf16_exhaustive_bits():
    """all 65 536 high halves x the low halves that decide a rounding: exact, just above, just below a tie, the tie (on both parities
    of the kept bit), just above it, all ones.  Holds every subnormal high half, +-0, +-inf, the largest finite f32 and NaNs whose
    payload sits only in the low half."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    return (hi[:, None] | np.array(BF16_LOW_HALVES, np.uint32)[None, :]).reshape(-1)


def bf16_random_bits(seed=0):
    return np.random.RandomState(seed).randint(0, 1 << 32, size=(1 << 20) + 3, dtype=np.uint64).astype(np.uint32)
