"""The plain exact top-k search (csrc/search.hip: `ShardIndex.search`, fp16 and int8 first passes) against float64 on shards of 600 k to 2 M
rows, where the tail kernels' stages differ from what the toy shards of test_gpu_search_fp64.py reach: the in-block tails with every one
of their 16 waves holding candidates (up to 1 024 super-groups = 2^20 rows), the select + rescore pair and the int8 COLLECT pipeline just
beyond that line, the 256-list cap of the select kernel (first reached at 2 041 super-groups; beyond it slices of three super-groups and
trailing empty lists), and a 4.4 GB shard whose rows lie beyond byte 2^31 and 2^32.

Shards (n, dim; tests/test_search_cases_host.py checks the figures on the CPU) are prefix views of one tensor per dim:
  A   625 000 x 768     the production shard: 611 super-groups, ragged group of 40 rows
  B1  1 047 581 x 128   1 024 super-groups, the last of ONE group, ragged 29 rows
  B2  1 048 576 x 128   1 024 full super-groups
  B3  1 048 577 x 128   1 025 super-groups: first size off the in-block tails; 129 lists, 513 wave slices used
  C1  2 088 989 x 128   2 041 super-groups: first size with 256 lists
  C2  2 097 181 x 128   2 049 super-groups: 3 per slice, lists 171 ... 255 empty
  D   2 162 717 x 1024  as C2, 4.43 GB
Rows are unit rows with planted ones (tests/search_cases.py): each shard has 16 graded queries whose k + 3 = 13 best rows are near-copies
of the query (0, 1, 2, 4, ... 2 048 one-ulp moves) in 13 of the shard's 16 spans, rotated so that every span holds some query's best row,
and the dim's tied query has one exact copy at the head of every span of every prefix, at every prefix's last row, at rows 2^20 - 1 and
2^20 and at the first row of every prefix's last non-empty select list.  A case's query batch is nested in the shard's master batch
(_queries: the zero query, adversarial, tiny and scaled unit queries stay).

Every reference is float64 (tests/helpers.py check_topk_fp64 and the pass-A budget A(D)); no tolerance is added here."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import check_topk_fp64, pass_a_budget, scores_fp64
from tests.search_cases import (GRADED0, LINE, N_MASTER, TIED_Q, _gen, _queries, _unit, batch_indices, check_pass_a_workspace,
                                pass_a_reference, plant_rows, plant_values, regime)
from tests.test_search_cases_host import TABLE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NO_ST = 8                                                       # ARX_TOPK_NO_SINGLE_ROW_TAIL (asserted against the library in `hip`)
CHUNK = 1 << 18
E_NQ = {"A": 64, "B1": 256, "B2": 256, "B3": 200, "C1": 200, "C2": 130, "D": 200}     # queries of the float64 score matrix kept per shard
PLANTED = list(range(GRADED0, TIED_Q + 1))                      # master indices of the 16 graded queries and the tied one


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available() and _lib.TOPK_NO_SINGLE_ROW_TAIL == NO_ST
    return _lib


class _Shard:
    def __init__(self, name, T, Qm, graded, ties):
        self.name, (self.n, self.d) = name, TABLE[name][:2]
        self.C, self.Qm, self.graded = T[:self.n], Qm, graded
        self.ties = [r for r in ties if r < self.n]
        self._e = None

    def batch(self, nq):
        """(queries [nq, d], {master index: position})"""
        b = batch_indices(nq)
        return self.Qm[torch.tensor(b, device="cuda")].contiguous(), {m: p for p, m in enumerate(b)}

    def e(self, nq):
        """float64 scores [nq, n] of batch(nq): rows of one matrix computed once per shard"""
        big = batch_indices(E_NQ[self.name])
        if self._e is None:
            self._e = scores_fp64(self.Qm[torch.tensor(big, device="cuda")], self.C)
        if nq == len(big):
            return self._e
        where = {m: p for p, m in enumerate(big)}
        return self._e[torch.tensor([where[m] for m in batch_indices(nq)], device="cuda")]


def _build_dim(d):
    names = [nm for nm, v in TABLE.items() if v[1] == d]
    ns = [TABLE[nm][0] for nm in names]
    g = _gen(9000 + d)
    T = torch.empty((max(ns), d), dtype=torch.float16, device="cuda")
    for a in range(0, max(ns), CHUNK):
        T[a:a + CHUNK] = _unit(min(CHUNK, max(ns) - a), d, g).half()
    graded, ties = plant_rows(ns)
    v16 = _unit(1, d, g).half()[0]
    shards = {}
    for j, (nm, n) in enumerate(zip(names, ns)):
        Qm = _queries(N_MASTER, d, g)
        pq = _unit(TIED_Q - GRADED0, d, g).half()
        Qm[GRADED0:TIED_Q] = pq
        Qm[TIED_Q] = v16
        rows, vals = plant_values(graded[n], ties if j == 0 else [], pq.cpu().numpy(), v16.cpu().numpy())
        T[torch.from_numpy(rows).cuda()] = torch.from_numpy(vals).cuda()
        shards[nm] = _Shard(nm, T, Qm.contiguous(), graded[n], ties)
    return SimpleNamespace(d=d, T=T, shards=shards)


@pytest.fixture(scope="module")
def shards():
    """name -> the shard; one dim's tensor (and its float64 score matrices) lives at a time, left unchanged while it does"""
    held = {}

    def get(name):
        d = TABLE[name][1]
        if d not in held:
            held.clear()
            torch.cuda.empty_cache()
            held[d] = _build_dim(d)
        return held[d].shards[name]
    torch.cuda.reset_peak_memory_stats()
    yield get
    print(f"\nlarge search shards: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    held.clear()
    torch.cuda.empty_cache()


def _bits_equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def _case(shard, pre, k, nq, tail, **kw):
    name = f"{shard}-{'i8' if pre else 'f16'}-k{k}-{nq}q" + "".join(f"-{a}" for a in kw.pop("tag", "").split() if a)
    return dict(id=name, shard=shard, pre=pre, k=k, nq=nq, tail=tail, **kw)


F16_IN, I8_IN, NT1024, NT256, I8_COLLECT = "f16-inblock", "i8-inblock", "select-rescore-NT1024", "select-rescore-NT256", "i8-collect"
CASES = [
    _case("A", None, 10, 64, F16_IN),
    _case("A", "int8", 10, 64, I8_IN, centre=True, tag="centred"),
    _case("A", "int8", 32, 16, I8_COLLECT),
]
for _b in ("B1", "B2"):
    CASES += [
        _case(_b, None, 10, 40, F16_IN),
        _case(_b, None, 1, 256, F16_IN),                        # the persistent pass A with aux words
        _case(_b, "int8", 10, 33, I8_IN),
        _case(_b, None, 10, 40, NT1024, flags=NO_ST, tag="flag"),
    ]
CASES += [
    _case("B3", None, 10, 40, NT1024),
    _case("B3", None, 2, 130, NT256),
    _case("B3", None, 32, 16, NT1024),
    _case("B3", "int8", 10, 33, I8_COLLECT, centre=True, tag="centred"),
    _case("B3", "int8", 2, 130, I8_COLLECT, centre=True, tag="centred"),
    _case("B3", "int8", 10, 33, I8_COLLECT, centre=False, tag="uncentred"),
]
for _c in ("C1", "C2"):
    CASES += [
        _case(_c, None, 10, 16, NT1024),
        _case(_c, None, 10, 130, NT256),
        _case(_c, None, 32, 16, NT1024),                        # K = 36, R = 9
        _case(_c, "int8", 10, 16, I8_COLLECT),
        _case(_c, "int8", 11, 16, I8_COLLECT),
    ]
CASES += [
    _case("D", None, 10, 8, NT1024, base=1 << 33, tag="base33"),
    _case("D", "int8", 10, 8, I8_COLLECT, base=1 << 33, tag="base33"),
    # two internal passes, the aux-region decision on the call's query count; float64 on queries 0-15, 1016-1031 and the last 16
    _case("B3", None, 10, 1100, NT256, subset=list(range(16)) + list(range(1016, 1032)) + list(range(1084, 1100))),
]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_large_shard_dispatch_fp64_and_bitwise_equal_to_the_exhaustive_scan(hip, shards, case):
    """Per case: the select kernel's launch count is the one `regime` states for the intended tail (branch); check_topk_fp64 passes for every
    query (exactness; the 1 100-query case on its named subset); the certified answer equals the tau_mult = 1e9 answer in ids and score
    bits (certificate); the zero query answers rows 0 ... k - 1 with score 0; the tied query answers its lowest planted rows in ascending
    order with equal score bits."""
    from arxiv_rag_amd.index import ShardIndex
    c = case
    sh = shards(c["shard"])
    k, nq, base, flags = c["k"], c["nq"], c.get("base", 0), c.get("flags", 0)
    Q_, where = sh.batch(nq)
    R = regime(sh.n, nq, k, bool(c["pre"]), no_single=bool(flags & NO_ST))
    assert R.tail == c["tail"] and R[:2] == TABLE[sh.name][2:4], (c["id"], R)
    idx = ShardIndex(sh.C, idx_base=base, prefilter=c["pre"], centre_query=c.get("centre"))
    if c["pre"] and c.get("centre") is not None:
        assert idx.centre_query == c["centre"]
    hip.prof_classes(["search_select"]); hip.prof_reset(); hip.prof_enable(True)
    try:
        s, i = idx.search(Q_, k, flags=flags)
        sel = hip.prof_read()["search_select"][1]
    finally:
        hip.prof_enable(False); hip.prof_classes(None); hip.prof_reset()
    flagged, extra = idx.certificate_stats()
    print(f"{c['id']}: {R.tail}, select launches {sel}; n_super {R.n_super}, nsplit {R.nsplit}, per {R.per}, lists used {R.lists}; "
          f"certificate counters ({flagged}, {extra})")
    assert sel == R.sel, (c["id"], "select launches", sel, R)
    if c.get("subset"):
        qs = torch.tensor(c["subset"], device="cuda")
        Qs = Q_[qs].contiguous()
        check_topk_fp64(sh.C, Qs, s[qs], i[qs], k, idx_base=base, e=scores_fp64(Qs, sh.C), what=c["id"])
    else:
        check_topk_fp64(sh.C, Q_, s, i, k, idx_base=base, e=sh.e(nq), what=c["id"])
    assert torch.equal(i[0], base + torch.arange(k, device="cuda")) and (s[0] == 0).all(), (c["id"], "zero query")
    p = where[TIED_Q]
    m = min(k, len(sh.ties))
    assert i[p, :m].tolist() == [base + r for r in sh.ties[:m]], (c["id"], "tied query", i[p].tolist())
    assert (s[p, :m].view(torch.int32) == s[p, 0].view(torch.int32)).all() and s[p, 0] > 0.99, (c["id"], "tied query's score bits")
    s1, i1 = idx.search(Q_, k, flags=flags, tau_mult=1e9)
    assert _bits_equal((s1, i1), (s, i)), (c["id"], "certified != exhaustive")


@pytest.mark.parametrize("pre", [None, "int8"], ids=["f16", "i8"])
@pytest.mark.parametrize("shard", ["B2", "C1", "D"])
def test_planted_answers_have_the_same_bits_on_every_path(hip, shards, shard, pre):
    """The answers (k = 10) to the 17 planted queries are bit-equal however they are asked: each alone, inside the 40-, 130- and 300-query
    batches, with and without NO_SINGLE_ROW_TAIL, with NO_PERSISTENT: every path ranks exact_row_score values by (score desc, row asc)."""
    from arxiv_rag_amd.index import ShardIndex
    sh = shards(shard)
    idx = ShardIndex(sh.C, prefilter=pre)
    k = 10
    Q40, where = sh.batch(40)
    pos = torch.tensor([where[m] for m in PLANTED], device="cuda")
    s, i = idx.search(Q40, k)
    ref = (s[pos].clone(), i[pos].clone())
    assert set(ref[1][0].tolist()) <= set(sh.graded[0].tolist()) and ref[1][-1].tolist() == sh.ties[:k], (shard, pre, "the planted rows do not decide")
    for j, m in enumerate(PLANTED):
        got = idx.search(sh.Qm[m:m + 1].contiguous(), k)
        assert _bits_equal(got, (ref[0][j:j + 1], ref[1][j:j + 1])), (shard, pre, "alone", m)
    for nq in (40, 130, 300):
        Q_, where = sh.batch(nq)
        pos = torch.tensor([where[m] for m in PLANTED], device="cuda")
        for fl in (0, NO_ST) + ((hip.TOPK_NO_PERSISTENT,) if nq > 128 else ()):
            s, i = idx.search(Q_, k, flags=fl)
            assert _bits_equal((s[pos], i[pos]), ref), (shard, pre, nq, fl)


@pytest.mark.parametrize("shard", ["B1", "B2", "B3", "C1", "D"])
def test_pass_a_group_maxima_within_budget_on_large_shards(hip, shards, shard):
    """SCAN_ONLY into a workspace filled with 0xFF, the per-tile 64-query kernel (40 queries), the persistent one (200) and the per-tile
    256-query one (200, NO_PERSISTENT): every group maximum within A(D) |q| max|c| of the float64 maximum of its group (the assertions of
    test_gpu_search_fp64's pass-A test, tests/search_cases.py); on B1 and B2, where the fp16 pass writes aux words, their bounds too."""
    from arxiv_rag_amd.index import ShardIndex
    sh = shards(shard)
    idx = ShardIndex(sh.C)
    A = pass_a_budget(sh.d)
    SCAN, NOP = hip.TOPK_SCAN_ONLY, hip.TOPK_NO_PERSISTENT
    aux = regime(sh.n, 200, 10, False).tail == F16_IN
    assert aux == (shard in ("B1", "B2"))
    for nq in (40, 200):
        Q_, _ = sh.batch(nq)
        e_g, cn, emax, cmax = pass_a_reference(sh.e(nq), sh.C, sh.n)
        qn = Q_.double().norm(dim=1)
        for fl in ((0,) if nq == 40 else (0, NOP)):
            ws = idx.alloc_workspace(nq, 10)
            ws.fill_(0xFF)
            idx.search(Q_, 10, ws=ws, flags=SCAN | fl)
            torch.cuda.synchronize()
            worst = check_pass_a_workspace(ws, sh.n, nq, A, qn, e_g, cn, emax, cmax, (shard, nq, fl), aux=aux)
            print(f"pass A, {shard}, {nq} queries, flags {fl}: largest |gmax - max e| / (u |q| max|c|) = {worst:.2f}   (budget 0.25 D = {0.25 * sh.d:g})")
            del ws
        del e_g, cn, emax, cmax


def test_int8_overflow_exit_on_a_large_shard(hip, shards):
    """B3 (int8, uncentred, k = 10: the COLLECT pipeline) with one copy of a vector v in one row of each of 4 200 groups spread over the
    shard, the last in the ragged group, two either side of row 2^20: query v has more candidate groups than PAIR_CAP_PER_QUERY = 4 096
    and must leave through merge_survivors -> tail_single_kernel<only_if>.  The counter says so, its answer is the 10 lowest planted rows
    in order and passes float64, and the unit query beside it gets the bits it gets in a call without v."""
    from arxiv_rag_amd.index import ShardIndex
    sh = shards("B3")
    n, k, n_planted = sh.n, 10, 4200
    G = (n + 63) // 64
    g = _gen(4200)
    C_ = sh.C.clone()
    v = _unit(1, sh.d, g).half()[0]
    groups = np.unique(np.round(np.linspace(0, G - 1, n_planted)).astype(np.int64))
    groups[-2] = G - 2
    assert groups.shape[0] == n_planted == np.unique(groups).shape[0] and groups[-1] == G - 1 and n - (G - 1) * 64 == 1
    rows = groups * 64 + (groups * 7) % 64
    rows[-2:] = [LINE - 1, LINE]
    assert rows.max() == n - 1 and (rows // 64 == groups).all()
    C_[torch.from_numpy(rows).cuda()] = v
    unit = sh.Qm[TIED_Q + 1:TIED_Q + 2]
    Q_ = torch.cat([torch.zeros_like(unit), v[None], unit]).contiguous()
    idx = ShardIndex(C_, prefilter="int8", centre_query=False)
    assert regime(n, 3, k, True).tail == I8_COLLECT
    s0, i0 = idx.search(Q_[[0, 2]].contiguous(), k)
    flagged0, _ = idx.certificate_stats()
    s, i = idx.search(Q_, k)
    flagged, cand = idx.certificate_stats()
    print(f"int8 overflow exit, {n_planted} planted groups: queries sent to the exhaustive kernel {flagged} (without v: {flagged0}), candidates {cand}")
    assert flagged == flagged0 + 1, ("query v did not take the overflow exit", flagged, flagged0)
    assert i[1].tolist() == np.sort(rows)[:k].tolist(), i[1].tolist()
    assert (s[1].view(torch.int32) == s[1, 0].view(torch.int32)).all()
    check_topk_fp64(C_, Q_, s, i, k, what="int8 overflow exit")
    assert _bits_equal((s[2:3], i[2:3]), (s0[1:2], i0[1:2])), "the unit query's answer changed beside the overflowing query"
    assert torch.equal(i[0], torch.arange(k, device="cuda")) and (s[0] == 0).all()
