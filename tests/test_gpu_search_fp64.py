"""Exact top-k search checked against float64 with the certificate's own rounding budgets (tests/helpers.py: A(D), B(D)), over the whole
admitted range: dims 64 ... 8192 (odd numbers of 64-wide k-tiles included), k = 1 ... 32, rows of any norm (fp16-subnormal components
included), every pass-A kernel form and every branch of topk_search_impl (csrc/search.hip)."""
import zlib

import numpy as np
import pytest

from tests.helpers import U24, check_topk_fp64, pass_a_budget, scores_fp64
from tests.search_cases import (_adversarial, _gen, _layout, _queries, _tiny, _unit, check_pass_a_workspace,  # noqa: F401
                                pass_a_reference)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = torch.nn.functional
PASS_A_DIMS = (64, 192, 320, 768, 1024, 1536, 4096, 8192)


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _cancelling(n, d, g):
    """(c) +-halves (half of the components +1/sqrt(d), half -1/sqrt(d), in random positions) plus a small signal: against a positive
    query the partial sums climb to ~|q||c|/2 and cancel to nearly nothing."""
    sign = torch.where(torch.rand((n, d), generator=g, device="cuda").argsort(dim=1) < d // 2, 1.0, -1.0)
    return sign / d ** 0.5 + 0.01 * torch.randn((n, d), generator=g, device="cuda") / d ** 0.5


def _norms(n, d, g):
    """(d) unit directions with norms from 0.01 to 8."""
    return _unit(n, d, g) * torch.exp(torch.empty((n, 1), device="cuda").uniform_(np.log(0.01), np.log(8.0), generator=g))


def _mixed_corpus(d, n_groups, g, ragged=29):
    """Whole 64-row groups of each family (so that a group's budget, relative to its largest row, is tight), tiny rows also mixed into
    unit groups at d >= 768, and a ragged last group."""
    fams = [_unit, _adversarial, _cancelling, _norms] + ([_tiny] if d >= 768 else [])
    parts = [fams[j % len(fams)](64, d, g) for j in range(n_groups)]
    if d >= 768:
        mix = _unit(64, d, g); mix[::2] = _tiny(32, d, g); parts.append(mix)
    parts.append(_unit(ragged, d, g))
    return torch.cat(parts).half().contiguous()


def test_pass_a_group_maxima_within_budget_every_dim_and_kernel_form(hip):
    """Pass A checked directly: a SCAN_ONLY call leaves the group maxima in the workspace; each must lie within A(D) |q| max_{r in g} |c_r|
    of the float64 maximum of its group — every row family, every kernel form (per-tile 64 / 128 / 256-query tiles, the persistent one,
    with and without aux words).  Where the single-row tail applies (k <= 10, <= 256 queries) the aux word too: its high half bounds every
    row outside the 4-row block at (aux & 63) from above (by e - A(D) |q| |c|), and that block holds the group's maximum (to the 63
    ulp of the position bits)."""
    from arxiv_rag_amd.index import ShardIndex
    SCAN, NOP = hip.TOPK_SCAN_ONLY, hip.TOPK_NO_PERSISTENT
    for d in PASS_A_DIMS:
        g = _gen(d)
        n_groups_full = 40 if d >= 4096 else 60
        C_ = _mixed_corpus(d, n_groups_full, g)
        n = C_.shape[0]
        Qall = _queries(300, d, g)
        A = pass_a_budget(d)
        idx = ShardIndex(C_)
        e_all = scores_fp64(Qall, C_)                                              # [300, n]
        e_g, cn, emax, cmax = pass_a_reference(e_all, C_, n)                      # [300, G, 64], [G, 64], [300, G], [G]
        qn = Qall.double().norm(dim=1)
        forms = [(40, 10, 0), (40, 32, 0), (100, 10, 0), (100, 32, 0), (200, 10, 0), (200, 32, 0), (300, 10, 0)]
        if d % 128 == 0:
            forms += [(200, 10, NOP), (200, 32, NOP)]                               # the per-tile 256-query kernel where the persistent one applies
        worst = 0.0
        for nq, k, fl in forms:
            what = (d, nq, k, fl)
            Q_ = Qall[:nq]
            ws = idx.alloc_workspace(nq, k)
            ws.fill_(0xFF)                                                          # (NaN patterns: a value the pass did not write cannot pass)
            idx.search(Q_, k, ws=ws, flags=SCAN | fl)
            torch.cuda.synchronize()
            worst = max(worst, check_pass_a_workspace(ws, n, nq, A, qn, e_g, cn, emax, cmax, what, aux=k <= 10 and nq <= 256))
        print(f"pass A, D = {d}: largest |gmax - max e| / (u |q| max|c|) = {worst:.2f}   (budget 0.25 D = {0.25 * d:g})")


def _near_tied(d, n, g, n_planted=60, n_queries=4):
    """A shard of unit rows with `n_planted` (> KSEL_BIG = 36) groups holding one row each that ties, or nearly ties, the best match of
    queries 1..n_queries (constant vectors; query 0 is zero): permutations of one positive jittered vector (the same dot product in real
    arithmetic, a different one after either pass's rounding) with 0 ... 256 of their components moved by one fp16 ulp, i.e. spaced
    from 0 to ~A(D) apart."""
    C_ = _unit(n, d, g).half()
    base = (_adversarial(1, d, g) * 0.9).half()[0]
    groups = torch.randperm(n // 64, generator=g, device="cuda")[:n_planted]
    for j, grp in enumerate(groups.tolist()):
        v = base[torch.randperm(d, generator=g, device="cuda")].clone()
        m = 0 if j % 2 == 0 else min(d, 1 << (j % 9))
        if m:
            pos = torch.randperm(d, generator=g, device="cuda")[:m]
            bits = v[pos].view(torch.int16) + torch.randint(-1, 2, (m,), generator=g, device="cuda").to(torch.int16)
            v[pos] = bits.view(torch.float16)
        C_[grp * 64 + int(torch.randint(64, (1,), generator=g, device="cuda"))] = v
    q = _unit(n_queries + 8, d, g).half()
    q[1:1 + n_queries] = torch.full((d,), 1.0 / d ** 0.5, device="cuda").half()
    q[0] = 0.0                                                                       # (f) the zero query
    # query n_queries + 1 (unit): exact copies of it and copies with 1 ... 64 components moved by one ulp, in `n_planted` more groups
    qc = q[n_queries + 1]
    groups2 = torch.randperm(n // 64, generator=g, device="cuda")
    groups2 = groups2[~torch.isin(groups2, groups)][:n_planted]
    for j, grp in enumerate(groups2.tolist()):
        v = qc.clone()
        m = 0 if j % 3 == 0 else min(d, 1 << (j % 7))
        if m:
            pos = torch.randperm(d, generator=g, device="cuda")[:m]
            v[pos] = (v[pos].view(torch.int16) + torch.randint(-1, 2, (m,), generator=g, device="cuda").to(torch.int16)).view(torch.float16)
        C_[grp * 64 + int(torch.randint(64, (1,), generator=g, device="cuda"))] = v
    return C_.contiguous(), q.contiguous()


# One case per branch of topk_search_impl (csrc/search.hip), drawn pairwise from k in {1, 2, 10, 11, 12, 16, 31, 32}, the fp16 dims above,
# int8 dims {128, 640, 896, 1024}, n in {1, k - 1, 63, 64, 65, 256 m + 1, 1 048 577 at d = 64} and idx_base up to 2^33.
# sel = launches of the select kernel (ARX_K_SEARCH_SELECT) expected: 0 on the in-block single-row tails, one per internal pass otherwise.
NO_ST = 8
CASES = [
    # fp16 single-row tail (k <= 10, <= 256 queries, <= 1 M rows)
    dict(id="f16-single-n1", d=64, n=1, nq=3, k=1, rows="unit", sel=0),
    dict(id="f16-single-n=k-1", d=192, n=9, nq=17, k=10, base=7, rows="mixed", sel=0),
    dict(id="f16-single-65", d=320, n=65, nq=256, k=2, base=1 << 33, rows="mixed", sel=0),
    dict(id="f16-single-1536", d=1536, n=256 * 40 + 1, nq=64, k=10, base=5, rows="mixed", sel=0),
    dict(id="f16-single-tiny-shard", d=768, n=64 * 40, nq=20, k=10, rows="tiny", sel=0),
    # select + rescore, KSEL_SMALL, 16-wave blocks (<= 128 queries) and 4-wave blocks
    dict(id="f16-ksmall-nt1024-flag", d=768, n=63, nq=128, k=10, flags=NO_ST, rows="mixed", sel=1),
    dict(id="f16-ksmall-nt1024-1M", d=64, n=1048577, nq=16, k=10, base=3, rows="unit", sel=1),
    dict(id="f16-ksmall-nt256-flag", d=1024, n=256 * 30 + 1, nq=200, k=2, base=1 << 33, flags=NO_ST, rows="mixed", sel=1),
    dict(id="f16-ksmall-nt256-300q", d=4096, n=64 * 64, nq=300, k=1, rows="unit", sel=1),
    # select + rescore, KSEL_BIG
    dict(id="f16-kbig-8192-ties", d=8192, n=64 * 130, nq=8, k=32, rows="ties", sel=1),
    dict(id="f16-kbig-4096-ties", d=4096, n=64 * 150, nq=130, k=16, base=11, rows="ties", sel=1),
    dict(id="f16-single-192-ties", d=192, n=64 * 200 + 5, nq=7, k=10, rows="ties", sel=0),
    dict(id="f16-kbig-320-ties", d=320, n=64 * 200, nq=7, k=32, base=1 << 33, rows="ties", sel=1),
    dict(id="f16-kbig-320", d=320, n=256 * 7 + 1, nq=40, k=31, rows="mixed", sel=1),
    dict(id="f16-kbig-64", d=64, n=64, nq=5, k=12, base=1 << 33, rows="unit", sel=1),
    dict(id="f16-kbig-1025q", d=192, n=64 * 100 + 1, nq=1025, k=11, rows="mixed", sel=2),
    dict(id="f16-kbig-2049q", d=128, n=64 * 100 + 1, nq=2049, k=32, base=1 << 33, rows="unit", sel=3),
    # int8 pre-filter: single tail in-block (KSEL_SMALL), KSEL_BIG (select kernel in front), the kernel pair, the fp16 pass above the crossover
    dict(id="i8-single-640", d=640, n=256 * 20 + 1, nq=33, k=10, pre="int8", centre=False, rows="mixed", sel=0),
    dict(id="i8-single-896-centred", d=896, n=65, nq=200, k=1, pre="int8", centre=True, base=1 << 33, rows="unit", sel=0),
    dict(id="i8-kbig-1024-centred", d=1024, n=256 * 40 + 1, nq=64, k=32, pre="int8", centre=True, base=9, rows="mixed", sel=1),
    dict(id="i8-kbig-n=k-1", d=128, n=10, nq=3, k=11, pre="int8", rows="unit", sel=1),
    dict(id="i8-kbig-128-ties", d=128, n=64 * 200, nq=7, k=12, pre="int8", rows="ties", sel=1),
    dict(id="i8-single-640-ties", d=640, n=64 * 200 + 1, nq=7, k=10, pre="int8", centre=True, rows="ties", sel=0),
    dict(id="i8-pair-flag", d=640, n=256 * 12 + 1, nq=100, k=2, pre="int8", flags=NO_ST, rows="mixed", sel=1),
    dict(id="i8-above-crossover-k16", d=896, n=256 * 9 + 1, nq=100, k=16, pre="int8", i8max=64, rows="mixed", sel=1),
    dict(id="i8-above-crossover-k10", d=896, n=256 * 9 + 1, nq=100, k=10, pre="int8", i8max=64, rows="mixed", sel=0),
    dict(id="i8-kbig-1025q", d=1024, n=64 * 60 + 1, nq=1025, k=11, pre="int8", centre=True, rows="unit", sel=2),
    dict(id="i8-kbig-2049q", d=128, n=64 * 100 + 1, nq=2049, k=32, pre="int8", centre=False, base=1 << 33, rows="mixed", sel=3),
    # int8 overflow exits: one unit row repeated, so every group's first and second bound is >= the true score = s_k > thr whatever the
    # quantisation: more group candidates than I8D_CAP_GROUPS = 512 (the single tail's exhaustive exit), than PAIR_CAP_PER_QUERY = 4096
    # (flagged by merge_survivors_kernel, re-run through tail_single_kernel<only_if> / rescore_kernel<only_if>)
    dict(id="i8-single-dup-overflow", d=128, n=64 * 600, nq=3, k=10, pre="int8", centre=False, rows="dup", sel=0),
    dict(id="i8-kbig-dup-redo", d=128, n=64 * 4200, nq=3, k=11, pre="int8", centre=False, rows="dup", sel=1),
    dict(id="i8-pair-dup-redo", d=128, n=64 * 4200, nq=3, k=2, pre="int8", centre=False, flags=NO_ST, rows="dup", sel=1),
]


def _case_data(c):
    g = _gen(zlib.crc32(c["id"].encode()))
    d, n, nq = c["d"], c["n"], c["nq"]
    if c["rows"] == "ties":
        C_, q = _near_tied(d, n, g)
        q = torch.cat([q, _unit(nq - q.shape[0], d, g).half()]) if nq > q.shape[0] else q[:nq]
        return C_.contiguous(), q.contiguous()
    if c["rows"] == "dup":
        return _unit(1, d, g).half().repeat(n, 1).contiguous(), _queries(nq, d, g)
    if c["rows"] == "unit":
        C_ = _unit(n, d, g)
    elif c["rows"] == "tiny":
        C_ = _tiny(n, d, g)
    else:                                                                            # families (a) - (e) row by row
        fams = [_unit, _adversarial, _cancelling, _norms] + ([_tiny] if d >= 768 else [])
        C_ = torch.cat([f(n, d, g)[None] for f in fams]).gather(0, torch.randint(len(fams), (1, n, 1), generator=g, device="cuda").expand(1, n, d))[0]
    return C_.half().contiguous(), _queries(nq, d, g)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_search_dispatch_matrix_fp64_and_bitwise_equal_to_the_exhaustive_scan(hip, case):
    """Every branch of the search against float64 (check_topk_fp64: pass-B budget, completeness, order, ids, padding); the certified answer
    equals the exhaustive one (tau_mult = 1e9: every group rescored) in ids AND score bits — both rank the same pass-B values, whose
    summation order is fixed; the zero query answers rows 0..k-1 with score 0 through the slow path; the select kernel's launch count
    says the intended branch ran."""
    from arxiv_rag_amd.index import ShardIndex
    c = case
    C_, Q_ = _case_data(c)
    k, base, flags = c["k"], c.get("base", 0), c.get("flags", 0)
    idx = ShardIndex(C_, idx_base=base, prefilter=c.get("pre"), i8_max_queries=c.get("i8max"), centre_query=c.get("centre"))
    if c.get("pre"):
        assert idx.centre_query == bool(c.get("centre", idx.centre_query))
    hip.prof_classes(["search_select"]); hip.prof_reset(); hip.prof_enable(True)
    try:
        s, i = idx.search(Q_, k, flags=flags)
        sel = hip.prof_read()["search_select"][1]
    finally:
        hip.prof_enable(False); hip.prof_classes(None); hip.prof_reset()
    flagged, _ = idx.certificate_stats()
    assert sel == c["sel"], (c["id"], "select launches", sel)
    check_topk_fp64(C_, Q_, s, i, k, idx_base=base, what=c["id"])
    kk = min(k, C_.shape[0])
    assert torch.equal(i[0, :kk], base + torch.arange(kk, device="cuda")) and (s[0, :kk] == 0).all(), (c["id"], "zero query")
    fp16_pass = not c.get("pre") or c["nq"] > c.get("i8max", 1024)
    if fp16_pass and (C_.shape[0] + 63) // 64 > (12 if k <= 10 else 36):       # (a shard of no more groups than the selection keeps leaves none out)
        assert flagged >= 1, (c["id"], "the zero query took the fast path")
    if c["rows"] == "dup":                                                          # every non-zero query overflowed its candidate lists
        assert flagged >= c["nq"] - 1, (c["id"], "slow-path queries", flagged)
        assert torch.equal(i, (base + torch.arange(k, device="cuda")).repeat(c["nq"], 1)), (c["id"], "identical rows: ids 0..k-1 in order")
    s1, i1 = idx.search(Q_, k, flags=flags, tau_mult=1e9)
    assert torch.equal(i1, i) and torch.equal(s1.view(torch.int32), s.view(torch.int32)), (c["id"], "certified != exhaustive")


@pytest.mark.parametrize("d", [1536, 4096, 8192])
def test_certificate_tolerance_is_the_stated_one(hip, d):
    """The certificate's tolerance itself: tau = (0.3125 D + 4) u |q| max|c| (search.hip tau_scale).  Twelve groups hold an exact copy of
    the query (they fill the 12 groups the selection keeps for k = 1), a thirteenth — left out — a copy with components moved towards zero
    by one ulp until its float64 score is below the copies' by `margin`.  A margin of 0.6 tau must send the query to the slow path (a
    tolerance narrower than stated would certify it), 1.6 tau must not (wider than stated); the answer is the first copy either way."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(d + 1)
    q = _unit(1, d, g).half()
    qn = float(q.double().norm())
    for frac, want_flag in ((0.6, True), (1.6, False)):
        C_ = (_unit(64 * 40, d, g) * 0.5).half()
        for grp in range(12):
            C_[grp * 64 + 5] = q[0]
        idx = ShardIndex(C_)
        tau = (0.3125 * d + 4) * U24 * qn * max(idx.max_row_norm(), 1 + 2 ** -9)
        qv = q[0].cpu().numpy()
        order = np.random.RandomState(d).permutation(d)                           # (one ulp of a component moves the score by ~ A(D) / D)
        lowered = np.nextafter(qv, np.float16(0)).astype(np.float16)
        drop = np.cumsum((qv.astype(np.float64) - lowered.astype(np.float64))[order] * qv.astype(np.float64)[order])
        m = int(np.searchsorted(drop, frac * tau)) + 1
        assert m <= d, (d, frac, "not enough components to reach the margin")
        v = qv.copy(); v[order[:m]] = lowered[order[:m]]
        C_[20 * 64 + 7] = torch.from_numpy(v).cuda()
        idx = ShardIndex(C_)
        s, i = idx.search(q, 1)
        flagged, _ = idx.certificate_stats()
        e = scores_fp64(q, C_)[0]
        margin = (e[5] - e[20 * 64 + 7]).item()
        assert abs(margin / tau - frac) < 0.1, (d, frac, margin / tau)
        assert i[0, 0].item() == 5, (d, frac)
        assert flagged == (1 if want_flag else 0), (d, frac, "margin / tau", margin / tau, "flagged", flagged)


@pytest.mark.parametrize("d,k,nq", [(320, 16, 40), (192, 10, 200), (576, 31, 300)])
def test_split_scan_and_tail_equal_the_single_call_bitwise(hip, d, k, nq):
    """SCAN_ONLY then TAIL_ONLY on one workspace (what search_many does per lane) at dims with an odd number of 64-wide k-tiles (the
    per-tile pass A with its 4-phase k-rotation) and k > 10: the same ids and score bits as one call."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(d + k)
    C_ = _mixed_corpus(d, 300, g)
    Q_ = _queries(nq, d, g)
    idx = ShardIndex(C_, idx_base=1 << 33)
    s, i = idx.search(Q_, k)
    ws = idx.alloc_workspace(nq, k)
    idx.search(Q_, k, ws=ws, flags=hip.TOPK_SCAN_ONLY)
    s2, i2 = idx.search(Q_, k, ws=ws, flags=hip.TOPK_TAIL_ONLY)
    assert torch.equal(i2, i) and torch.equal(s2.view(torch.int32), s.view(torch.int32))
    check_topk_fp64(C_, Q_, s, i, k, idx_base=1 << 33)


def test_search_rejects_unknown_keywords(hip):
    """A misspelled hook (`tau_mul`, `flag`) would be dropped and make a test vacuous: it is a TypeError."""
    from arxiv_rag_amd.index import ShardIndex
    idx = ShardIndex(_unit(100, 128, _gen(1)).half())
    q = _unit(2, 128, _gen(2)).half()
    for bad in (dict(tau_mul=1e9), dict(flag=hip.TOPK_SCAN_ONLY), dict(drop=1)):
        with pytest.raises(TypeError):
            idx.search(q, 5, **bad)
    idx.search(q, 5, tau_mult=1e9, drop_best=1, flags=0)


def test_int8_switch_off_ignores_batches_above_the_crossover(hip):
    """An adaptive int8 index with i8_max_queries = 64: a 300-query batch takes the fp16 pass, whose counters count uncertified selections
    (every query here: all rows identical, every group tied) — not int8 candidate lists overflowing.  The pre-filter must stay on."""
    from arxiv_rag_amd.index import ShardIndex
    C_ = _unit(1, 128, _gen(3)).half().repeat(64 * 300, 1).contiguous()
    Q_ = _unit(300, 128, _gen(4)).half()
    idx = ShardIndex(C_, prefilter="int8", adaptive=True, i8_max_queries=64)
    for _ in range(2):
        s, i = idx.search(Q_, 10)
        assert idx.certificate_stats()[0] * 4 > 300                                  # the fp16 certificate flagged > a quarter of the batch
        assert not idx.prefilter_disabled
    assert torch.equal(i, torch.arange(10, device="cuda").repeat(300, 1))
