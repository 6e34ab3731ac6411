"""Shared by the exact top-k search suites (test_gpu_search_fp64.py, test_gpu_search_large.py, test_search_cases_host.py): the row and query
generators, a plain-Python restatement of the dispatch of csrc/search.hip (`regime`), the planter that puts decisive rows into every
sixteenth of a shard, and the pass-A assertions."""
from collections import namedtuple

import numpy as np
import torch

from tests.helpers import U24, row_norms_fp64

F = torch.nn.functional


def _gen(seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    return g


def _unit(n, d, g):
    return F.normalize(torch.randn((n, d), generator=g, device="cuda"), dim=1)


def _adversarial(n, d, g):
    """(b) every component positive and of nearly equal size (1/sqrt(d) with a few f16 ulps of jitter): the partial sums of an
    accumulation chain grow linearly, its worst case."""
    j = torch.randint(-4, 5, (n, d), generator=g, device="cuda").float()
    return (1.0 + j * 2.0 ** -10) / d ** 0.5


def _tiny(n, d, g):
    """(e) norm 1e-3: at d >= 768 most components are fp16 subnormals (< 2^-14)."""
    return _unit(n, d, g) * 1e-3


def _queries(nq, d, g):
    """query 0 all zero (f), 1..40 rounding-adversarial (positive), 41..50 tiny (subnormal components), the rest unit, every 7th of
    those scaled to norm 8."""
    q = _unit(nq, d, g)
    m = min(40, nq - 1)
    if m > 0:
        q[1:1 + m] = _adversarial(m, d, g)
    m = min(10, nq - 41)
    if m > 0:
        q[41:41 + m] = _tiny(m, d, g)
    q[51::7] *= 8.0
    q[0] = 0.0
    return q.half().contiguous()


def _layout(n, nq):
    """Offsets of the fp16 pass's workspace (csrc/search.hip topk_layout): 256 bytes of counters, gmax [groups][ldg] f32, two selection
    arrays of nsplit x ldg x 36 words, then the aux words in gmax's shape; every region 256-byte aligned."""
    r256 = lambda b: (b + 255) // 256 * 256
    n_groups = (n + 63) // 64
    ldg = (min(nq, 1024) + 63) // 64 * 64
    n_super = (n_groups + 15) // 16
    nsplit = max(1, min(256, (n_super + 7) // 8))
    return n_groups, ldg, 256, 256 + r256(n_groups * ldg * 4) + 2 * r256(nsplit * ldg * 36 * 4)


# ---- the dispatch of topk_search_impl, restated ----------------------------------------------------------------------------------------------
GROUP, SUPER, SEL_WAVES, QBATCH = 64, 16, 4, 1024                 # csrc/search_consts.h: GROUP_ROWS, SUPER, SEL_SPLIT_WAVES, QBATCH_MAX
INBLOCK_MAX_SUPER, AUX16_MAX_NQ, NSPLIT_MAX = 1024, 256, 256
LINE = 1 << 20
N_SPANS = 16

Regime = namedtuple("Regime", "n_groups n_super nsplit per slices lists tail sel")


def _cdiv(a, b):
    return -(-a // b)


def regime(n, nq, k, int8, no_single=False):
    """What a search of nq queries for k rows over an n-row shard runs (csrc/search.hip: topk_layout, tail_single_ok, run_i8_single's
    `inblock`; no_single = ARX_TOPK_NO_SINGLE_ROW_TAIL):
      n_groups, n_super   64-row groups, 16-group super-groups;
      nsplit, per         select lists per query and super-groups per wave slice of select_groups_kernel (4 slices fill one list);
      slices, lists       wave slices / lists that hold a super-group (the others are written as -1);
      tail                f16-inblock | i8-inblock | select-rescore-NT1024 | select-rescore-NT256 | i8-collect (the first internal pass's;
                          i8-pair-collect: the int8 pass with no_single, rescore_kernel's COLLECT form);
      sel                 launches of select_groups_kernel: none on the in-block tails, else one per internal pass of 1 024 queries."""
    n_groups = _cdiv(n, GROUP)
    n_super = _cdiv(n_groups, SUPER)
    nsplit = max(1, min(NSPLIT_MAX, _cdiv(n_super, 8)))
    per = _cdiv(n_super, SEL_WAVES * nsplit)
    slices = _cdiv(n_super, per)
    lists = _cdiv(slices, SEL_WAVES)
    passes = _cdiv(nq, QBATCH)
    first = min(nq, QBATCH)
    small = n_super <= INBLOCK_MAX_SUPER
    if int8 and not no_single:
        tail = "i8-inblock" if (small and k <= 10) else "i8-collect"
    elif int8:
        tail = "i8-pair-collect"
    elif k <= 10 and nq <= AUX16_MAX_NQ and small and not no_single:
        tail = "f16-inblock"
    elif k > 10 or first <= 128:
        tail = "select-rescore-NT1024"
    else:
        tail = "select-rescore-NT256"
    sel = 0 if tail.endswith("inblock") else passes
    return Regime(n_groups, n_super, nsplit, per, slices, lists, tail, sel)


def last_list_first_row(n):
    """the first row of the last select list that holds a super-group"""
    r = regime(n, 1, 10, False)
    return SEL_WAVES * (r.lists - 1) * r.per * SUPER * GROUP


# ---- the planter -------------------------------------------------------------------------------------------------------------------------------
# Master query batch of a shard: _queries(N_MASTER) with the planted queries written over unit queries 51 ... 67; a case's batch of nq
# queries is the first nq of PRIORITY in ascending order, so that batches are nested, the zero query stays first and every batch of 18 or
# more holds all the planted queries.
N_MASTER, N_GRADED, PLANT_K = 1100, 16, 10
GRADED0, TIED_Q = 51, 67
PRIORITY = [0, TIED_Q] + list(range(GRADED0, TIED_Q)) + list(range(1, GRADED0)) + list(range(TIED_Q + 1, N_MASTER))
GRADES = [0] + [1 << j for j in range(PLANT_K + 2)]              # ulp moves of the k + 3 near-copies: 0, 1, 2, 4, ... 2048


def batch_indices(nq):
    return sorted(PRIORITY[:nq])


def span_of(row, n):
    return row // _cdiv(n, N_SPANS)


def tie_rows(n):
    """Rows of an n-row shard that hold a copy of the tied vector: the first row of each of the 16 spans (row 0 among them), the last row
    (inside the ragged group), rows 2^20 - 1 and 2^20 where they exist, the first row of the last non-empty select list."""
    span = _cdiv(n, N_SPANS)
    rows = {s * span for s in range(N_SPANS)} | {n - 1, last_list_first_row(n)} | {r for r in (LINE - 1, LINE) if r < n}
    assert all(0 <= r < n for r in rows)
    return rows


def plant_rows(prefixes):
    """prefixes: the row counts of the shards that share one tensor (each a prefix view of the longest) ->
    (graded, ties): graded[n] int64 [16, k + 3]: rank r of planted query j of shard n lies in span (j + r) mod 16 of that shard, at a
    spacing that spreads a shard's planted rows over as many groups as the last (shortest) span allows; query 15's best row is moved into
    the last non-empty select list where that list has room; ties: the sorted rows of the tied vector (tie_rows of every prefix).  No
    row is used twice: a graded row that meets a used one moves up by one."""
    ties = set()
    for n in prefixes:
        ties |= tie_rows(n)
    used = set(ties)
    graded = {}
    m = PLANT_K + 3
    assert m <= N_SPANS
    for n in prefixes:
        span = _cdiv(n, N_SPANS)
        last_len = n - (N_SPANS - 1) * span
        assert last_len >= N_GRADED * N_SPANS + 3, (n, "shard too short for the planter")
        step = (last_len - 3) // (N_GRADED * N_SPANS)
        rows = np.zeros((N_GRADED, m), np.int64)
        for j in range(N_GRADED):
            for r in range(m):
                row = ((j + r) % N_SPANS) * span + 1 + (j * N_SPANS + r) * step
                if j == N_SPANS - 1 and r == 0 and last_list_first_row(n) + 2 < n:
                    row = max(row, last_list_first_row(n) + 1)
                while row in used:
                    row += 1
                assert row < n - 1 and span_of(row, n) == (j + r) % N_SPANS, (n, j, r, row)
                used.add(row)
                rows[j, r] = row
        graded[n] = rows
    return graded, sorted(ties)


def near_copies(q16, grades=GRADES):
    """q16: one fp16 vector (numpy) -> [len(grades), d] fp16: copy i has grades[i] one-ulp moves towards zero, dealt round the
    components (component c takes m // d, and one more if c < m % d), so each copy's score against q16 is at most the one before's."""
    u = q16.view(np.uint16).astype(np.int64)
    d = u.shape[0]
    out = np.zeros((len(grades), d), np.uint16)
    for i, m in enumerate(grades):
        t = m // d + (np.arange(d) < m % d)
        out[i] = ((u & 0x8000) | np.maximum((u & 0x7FFF) - t, 0)).astype(np.uint16)
    return out.view(np.float16)


# ---- pass A's group maxima in a SCAN_ONLY workspace ----------------------------------------------------------------------------------------------
def pass_a_reference(e, c, n):
    """e [nq, n] float64 scores, c the fp16 rows -> (e_g [nq, G, 64] with -inf beyond the shard, cn [G, 64] float64 row norms with zeros
    beyond it, emax [nq, G], cmax [G])"""
    G = (n + 63) // 64
    nq = e.shape[0]
    pad = torch.full((nq, G * 64 - n), float("-inf"), dtype=torch.float64, device=e.device)
    e_g = torch.cat([e, pad], dim=1).view(nq, G, 64)
    cn = torch.cat([row_norms_fp64(c), torch.zeros(G * 64 - n, dtype=torch.float64, device=e.device)]).view(G, 64)
    return e_g, cn, e_g.max(dim=2).values, cn.max(dim=1).values


def check_pass_a_workspace(ws, n, nq, A, qn, e_g, cn, emax, cmax, what, aux):
    """ws: the workspace a SCAN_ONLY call of nq queries left (filled with 0xFF before it).  Every group maximum within A |q| max|c| of the
    float64 maximum of its group; with `aux` also the aux words: the high half bounds every row outside the 4-row block at (aux & 63)
    from above, and that block holds the group's maximum.  -> the largest |gmax - max e| / (u |q| max|c|) over the full groups"""
    G, ldg, off_g, off_aux = _layout(n, nq)
    gm = ws[off_g:off_g + G * ldg * 4].view(torch.float32).view(G, ldg)[:, :nq].T.double()      # [nq, G]
    bud = A * qn[:nq, None] * cmax[None, :]
    em = emax[:nq]
    full = slice(0, G - 1)
    err = (gm[:, full] - em[:, full]).abs()
    assert torch.isfinite(gm).all(), what
    assert (err <= bud[:, full]).all(), (what, "pass A outside A(D)", ((err - bud[:, full]).max().item()))
    # the ragged last group: rows past the shard may enter the maximum as zeros (a conservative bound), never as anything else
    assert (gm[:, -1] >= em[:, -1] - bud[:, -1]).all() and (gm[:, -1] <= em[:, -1].clamp_min(0) + bud[:, -1]).all(), what
    assert (gm[0] == 0).all(), (what, "zero query")
    scale = U24 * qn[:nq, None] * cmax[None, :]
    ok = scale[:, full] > 0
    worst = (err[ok] / scale[:, full][ok]).max().item()
    if aux:
        aw = ws[off_aux:off_aux + G * ldg * 4].view(torch.int32).view(G, ldg)[:, :nq].T         # [nq, G]
        ub2 = (aw & -65536).view(torch.float32).double()
        arg = (aw & 63).long()
        assert (arg % 4 == 0).all(), what
        lowered = e_g[:nq] - A * qn[:nq, None, None] * cn[None]             # [nq, G, 64]: a lower bound of each pass-A score
        raised = e_g[:nq] + A * qn[:nq, None, None] * cn[None]
        blk = arg[:, :, None] + torch.arange(4, device=ws.device)[None, None, :]
        others = lowered.clone(); others.scatter_(2, blk, float("-inf"))
        o2 = others.max(dim=2).values
        fin = torch.isfinite(o2)
        assert (ub2[fin] >= o2[fin]).all(), (what, "aux bound below a row outside the arg-max block", (o2 - ub2)[fin].max().item())
        # the block is the arg-max of keys whose low 6 bits carry the position: it holds the maximum to within 63 ulp
        inblk = raised[:, full].gather(2, blk[:, full]).max(dim=2).values
        assert (inblk >= gm[:, full] - gm[:, full].abs() * 2.0 ** -17).all(), (what, "the arg-max block does not hold the group maximum")
        assert (ub2 - gm - gm.abs() * 0.008 <= 1e-9).all(), (what, "aux above the group maximum")
    return worst


def plant_values(graded_rows, ties, q16, v16):
    """graded_rows [16, k + 3] (plant_rows), ties: rows of the tied vector, q16 [16, d] fp16 planted queries, v16 [d] the tied vector
    (numpy) -> (rows [N] int64, values [N, d] fp16) to write into the shard"""
    rows = [graded_rows.reshape(-1)]
    vals = [np.concatenate([near_copies(q16[j]) for j in range(graded_rows.shape[0])])]
    if len(ties):
        rows.append(np.asarray(ties, np.int64))
        vals.append(np.repeat(v16[None, :], len(ties), axis=0))
    return np.concatenate(rows), np.concatenate(vals)
