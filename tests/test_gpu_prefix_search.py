"""Exact top-k with a row limit per query on the device (-m gpu): `ShardIndex.search_prefix` / `nearest_earlier` (csrc/prefix.hip).
The definition it is held to is the one the repository already has for "exact top-k of the allowed rows": `ShardIndex.search(allow=bitmap of
rows < limit)`, bit for bit, plus `check_topk_fp64` over the prefix; every path (library's choice, masked scan, exhaustive, masked scan
with a one-entry candidate list = the fallback) must return the same bits, and a row's answer must not depend on the batch it is in."""
import numpy as np
import pytest

from tests.helpers import allow_below as _allow_below, check_against_filtered_and_fp64 as _check_against_filtered_and_fp64
from tests.helpers import check_prefix_answer

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_gpu_search_fp64 import _case_data, _gen, _unit  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


# n: 1, 2, 63, 64, 65, 257 (two tiles), 256*5+1, 64*200+5, 2200 (three internal query slices in the self-join); every dim and k of the
# issue pairwise; `ties` rows need 120 groups or more (tests/test_gpu_search_fp64.py::_near_tied)
CASES = [
    dict(id="n1", d=64, n=1, nq=3, k=1, rows="unit"),
    dict(id="n2", d=128, n=2, nq=5, k=10, rows="unit"),
    dict(id="n63", d=320, n=63, nq=17, k=32, rows="mixed", base=7),
    dict(id="n64", d=768, n=64, nq=64, k=1, rows="mixed"),
    dict(id="n65", d=1024, n=65, nq=65, k=10, rows="unit", base=1 << 33),
    dict(id="n257", d=64, n=257, nq=129, k=32, rows="mixed"),
    dict(id="n1281", d=128, n=256 * 5 + 1, nq=300, k=10, rows="mixed", base=5),
    dict(id="n12805-ties-k10", d=320, n=64 * 200 + 5, nq=12, k=10, rows="ties"),
    dict(id="n12805-ties-k32", d=64, n=64 * 200 + 5, nq=70, k=32, rows="ties", base=1 << 33),
    dict(id="n12805-ties-k1", d=768, n=64 * 200 + 5, nq=12, k=1, rows="ties"),
    dict(id="n2200-k1", d=128, n=2200, nq=70, k=1, rows="unit"),
    dict(id="n2200-k32", d=1024, n=2200, nq=130, k=32, rows="mixed", base=3),
]
KINDS = ["self", "zero", "all", "one", "random", "const", "above"]
_DATA = {}


def _data(c):
    """One corpus / query set / index per case, shared by its limit kinds and left unchanged."""
    if c["id"] not in _DATA:
        from arxiv_rag_amd.index import ShardIndex
        _DATA.clear()                                             # (one case's tensors at a time)
        C_, Q_ = _case_data(c)
        _DATA[c["id"]] = (C_, Q_, ShardIndex(C_, idx_base=c.get("base", 0)))
    return _DATA[c["id"]]


def _limits(kind, n, nq, seed):
    rs = np.random.RandomState(seed)
    if kind == "zero":
        return np.zeros(nq, np.int64)
    if kind == "all":
        return np.full(nq, n, np.int64)
    if kind == "one":
        return np.ones(nq, np.int64)
    if kind == "random":
        return rs.randint(0, n + 1, size=nq).astype(np.int64)
    if kind == "const":
        return np.full(nq, min(n, (2 * n // 3) | 1), np.int64)      # odd: never a multiple of 64
    assert kind == "above"
    lim = n + 1 + rs.randint(0, 1000, size=nq).astype(np.int64)
    lim[::3] = rs.randint(0, n + 1, size=lim[::3].shape[0])       # (mixed with limits inside the shard)
    lim[-1] = (1 << 40) + 5
    return lim


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_prefix_search_every_path_same_bits_equal_to_the_filtered_search_and_fp64(hip, case, kind):
    c = case
    C_, Qc, idx = _data(c)
    n, k, base = C_.shape[0], c["k"], c.get("base", 0)
    what = (c["id"], kind)
    if kind == "self":
        Q_, lim = C_, np.arange(n, dtype=np.int64)
    else:
        Q_, lim = Qc, _limits(kind, n, Qc.shape[0], n + len(kind))
    nq = Q_.shape[0]
    lim_d = torch.from_numpy(lim).cuda()
    lim_c = np.clip(lim, 0, n)
    s, i = idx.search_prefix(Q_, lim_d, k)
    over0, _ = idx.prefix_stats()
    assert s.shape == (nq, k) and i.shape == (nq, k) and s.dtype == torch.float32 and i.dtype == torch.int64
    # every path, and the fallback forced wherever two groups are candidates: the same bits
    for kw in (dict(path=1), dict(path=2), dict(path=1, cand_cap=1)):
        s1, i1 = idx.search_prefix(Q_, lim_d, k, **kw)
        assert torch.equal(i1, i) and torch.equal(_bits(s1), _bits(s)), (what, kw)
    over, _ = idx.prefix_stats()
    two_groups = int((lim_c > 64).sum())                          # queries with rows below the limit in two groups or more
    if k >= 2:                                                    # min(k, groups) groups reach the k-th largest maximum: two or more candidates
        assert over == two_groups, (what, "fallback count with a one-entry list", over, two_groups)
    else:
        assert over <= two_groups, (what, over, two_groups)
    assert over0 <= two_groups
    # no id at or beyond the limit, over ALL queries; the padding is exactly the missing rows
    check_prefix_answer(s, i, lim_c, k, base, what)
    if kind == "all":                                             # the whole batch against the filtered search with every row allowed
        ones = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
        fs, fi = idx.search(Q_, k, allow=ones)
        assert torch.equal(fi, i) and torch.equal(_bits(fs), _bits(s)), (what, "all-ones bitmap")
    if kind == "self":
        must = [r for r in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, n - 1) if r < n]
        rest = np.random.RandomState(n).choice(n, size=min(n, 64), replace=False).tolist()
        sample = list(dict.fromkeys(must + rest))[:64]
    else:
        sample = np.random.RandomState(nq).choice(nq, size=min(nq, 64), replace=False).tolist()
    _check_against_filtered_and_fp64(idx, C_, Q_, lim_c, s, i, k, sample, what)
    if kind == "self":
        s2, i2 = idx.nearest_earlier(0, n, k)
        assert torch.equal(i2, i) and torch.equal(_bits(s2), _bits(s)), (what, "nearest_earlier")


def test_a_rows_answer_does_not_depend_on_the_range_it_is_asked_in(hip):
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(77)
    n, d, k = 2200, 128, 10
    C_ = _unit(n, d, g).half().contiguous()
    C_[1500:1600] = C_[100:200]                                   # some exact copies: ties on the row number
    idx = ShardIndex(C_, idx_base=11)
    s, i = idx.nearest_earlier(0, n, k)
    assert i[0].eq(-1).all() and int(i[1, 0]) == 11 and (i[1, 1:] == -1).all()
    assert torch.equal(i[1500:1600, 0], 11 + torch.arange(100, 200, device="cuda"))
    for a, b in ((37, 1501), (1023, 1026), (1100, 1101), (n - 1, n), (0, 1), (5, 5)):
        s1, i1 = idx.nearest_earlier(a, b, k)
        assert s1.shape == (b - a, k)
        assert torch.equal(i1, i[a:b]) and torch.equal(_bits(s1), _bits(s[a:b])), (a, b)
    s1, i1 = idx.nearest_earlier(1100, 1101, k, path=2)
    assert torch.equal(i1, i[1100:1101]) and torch.equal(_bits(s1), _bits(s[1100:1101]))
    with pytest.raises(ValueError):
        idx.nearest_earlier(5, n + 1)
    with pytest.raises(TypeError):
        idx.nearest_earlier(0, 5, tau_mult=2.0)


def test_argument_checks(hip):
    from arxiv_rag_amd.index import ShardIndex
    lib = hip.load()
    C_ = _unit(100, 64, _gen(1)).half().contiguous()
    idx = ShardIndex(C_)
    lim = torch.arange(100, device="cuda")
    assert lib.arx_topk_prefix_workspace_bytes(100, 4, 96, 10) == -1 and lib.arx_topk_prefix_workspace_bytes(100, 4, 64, 33) == -1
    assert lib.arx_topk_prefix_workspace_bytes(100, 4, 64, 32) > 0
    for kw in (dict(path=3), dict(cand_cap=8193), dict(cand_cap=-1)):
        with pytest.raises(hip.ArxError):
            idx.search_prefix(C_, lim, 5, **kw)
    with pytest.raises(hip.ArxError):
        idx.search_prefix(C_, lim, 5, ws=torch.empty(64, dtype=torch.uint8, device="cuda"))
    s, i = idx.search_prefix(C_, lim, 5, cand_cap=8192)
    assert int(i[99, 0]) >= 0 and idx.prefix_stats()[0] == 0
    assert ShardIndex(C_).prefix_stats() == (0, 0)


def test_self_join_of_200001_rows_against_the_filtered_search(hip):
    """196 internal query slices: rows 1, 63, 64, 65, the last row and the rows on either side of slice boundaries, bit for bit against the
    filtered search over the bitmap of earlier rows."""
    from arxiv_rag_amd.index import ShardIndex
    n, d = 200001, 64
    C_ = _unit(n, d, _gen(5)).half().contiguous()
    idx = ShardIndex(C_, idx_base=1 << 33)
    s, i = idx.nearest_earlier(0, n, 1)
    assert int(i[0, 0]) == -1 and ((i[1:, 0] - (1 << 33)) < torch.arange(1, n, device="cuda")).all() and (i[1:, 0] >= 1 << 33).all()
    bound = [1024 * j + o for j in np.linspace(1, 195, 25).astype(int).tolist() for o in (-1, 0)]
    rows = list(dict.fromkeys([1, 63, 64, 65, n - 1, 1023, 1024] + bound))[:64]
    assert len(rows) <= 64 and 1024 * 195 in rows and 1024 * 195 - 1 in rows
    for r in rows:
        fs, fi = idx.search(C_[r:r + 1], 1, allow=_allow_below(r, n), n_allowed=r)
        assert torch.equal(fi, i[r:r + 1]) and torch.equal(_bits(fs), _bits(s[r:r + 1])), r


def test_planted_copies_report_their_first_original_and_overflow_the_candidate_list(hip):
    """500 rows of a 5 000-row unit corpus copied to later positions — one of them ("boilerplate") into every free slot of 70 000 appended
    rows, so that its late copies see more than 1 024 groups tied at the top and go to the exhaustive path.  Every copy reports the first
    original (the lowest earlier identical row) and all copies of one original report the same score bits."""
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(9)
    n0, extra, d = 5000, 70000, 64
    rs = np.random.RandomState(9)
    base = _unit(n0, d, g).half()
    src = rs.choice(n0, size=500, replace=False)
    boiler = int(src[0])
    origin = np.full(extra, boiler, np.int64)
    slots = rs.choice(extra, size=3 * 499, replace=False)
    origin[slots] = np.repeat(src[1:], 3)                         # the other 499 rows: three copies each, scattered
    origin_t = torch.from_numpy(origin).cuda()
    C_ = torch.cat([base, base[origin_t]]).contiguous()
    idx = ShardIndex(C_)
    s, i = idx.nearest_earlier(0, C_.shape[0], 1)
    over, cand = idx.prefix_stats()
    assert over > 0, "no query overflowed the default candidate list: the fallback was not exercised"
    assert torch.equal(i[n0:, 0], origin_t), "a copy does not report its first original"
    for o in (boiler, int(src[1]), int(src[499])):
        bits = _bits(s[n0:, 0][origin_t == o])
        assert (bits == bits[0]).all(), ("copies of one original with different score bits", o)
    # the originals themselves are not copies of anything earlier: unit rows of dimension 64 stay well below 0.9
    assert float(s[1:n0, 0].max()) < 0.9 and float(s[n0:, 0].min()) > 0.99
    # a late boilerplate copy, alone and by the exhaustive path: the same bits
    r = C_.shape[0] - 1
    for kw in (dict(), dict(path=2), dict(cand_cap=8192)):
        s1, i1 = idx.nearest_earlier(r, r + 1, 1, **kw)
        assert torch.equal(i1, i[r:]) and torch.equal(_bits(s1), _bits(s[r:])), kw
