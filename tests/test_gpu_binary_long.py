"""arx_binary_candidates where one block scans thousands of rows and where a call is cut into query slices (-m gpu).

A scan block cuts a query's LDS list back to its R best keys whenever the next round of 256 rows could overflow its 1024 slots, and from
then on appends only keys above the list's threshold.  That path needs more than 1024 rows per block: here 9000 rows at
rows_per_block = default (2048), 4096 and 8192, compared exactly against `binary.candidates_host`.  `schedule` (tests/key_list_cases.py,
shared with the PQ scan's suite) restates the block's bookkeeping (which lists are cut before which round, how many keys a non-zero
threshold turns away) so that the tests can assert that the runs really contain cut and uncut lists, tiles whose eight lists are not cut
together, and rejections.

Further down: the one-word load at odd W above 1 (dims 192 and 8128), W = 128 (dim 8192: the whole of the query words' LDS array), and a
shard of 2^21 + 197 rows whose planted rows put a query's candidates beyond row 2^20, across it, and in the ragged last wave."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import binary as B
from arxiv_rag_amd.index import ShardIndex
from arxiv_rag_amd.where import pack_bitmap
from tests.key_list_cases import schedule_distances as schedule      # (distance asc, row asc): the restated bookkeeping of a list

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NQ = 9000, 70
DEFAULT_RPB = 2048                                              # what the library picks for 9000 rows x 9 query tiles


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


_BASE = {}


def base(dim):
    if dim not in _BASE:
        rs = np.random.RandomState(1000 + dim)
        X = (rs.randn(N, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        Q = (rs.randn(NQ, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
        X[7000] = X[10]
        Q[0] = X[10]
        centre = X.astype(np.float32).mean(axis=0)
        codes, qcodes = B.pack_host(X, centre), B.pack_host(Q, centre)
        half = rs.rand(N) < 0.5
        w = dict(codes=codes, qcodes=qcodes, half=half, d=B.distances_host(codes, qcodes), host={},
                 dcodes=dev(codes.view(np.int64), np.int64), dqcodes=dev(qcodes.view(np.int64), np.int64),
                 dhalf=dev(pack_bitmap(half).view(np.int64), np.int64))
        _BASE[dim] = w
    return _BASE[dim]


def host(w, R, masked):
    if (R, masked) not in w["host"]:
        w["host"][(R, masked)] = B.candidates_host(w["codes"], w["qcodes"], R, w["half"] if masked else None)
    return w["host"][(R, masked)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dim", [64, 768])
def test_blocks_of_thousands_of_rows_equal_the_definition(dim, masked):
    w = base(dim)
    allow = w["dhalf"] if masked else None
    for R in (1, 10, 256):
        want = host(w, R, masked)
        for rpb in (None, 4096, 8192, 64):
            got = B.candidates_device(w["dcodes"], w["dqcodes"], R, allow=allow, rows_per_block=rpb)
            assert same(got, want), (dim, masked, R, rpb)
    if not masked:
        assert host(w, 256, False)[0][0, :2].tolist() == [10, 7000] and host(w, 256, False)[1][0, :2].tolist() == [0, 0]


@pytest.mark.parametrize("dim", [64, 768])
def test_those_runs_cut_some_lists_and_not_others(dim):
    """What the runs above exercised, from the restated bookkeeping: lists cut once and several times, lists never cut (the short last
    block, every block at rows_per_block = 64), a tile whose lists are not all cut before the same round, and keys turned away."""
    w = base(dim)
    everything = np.ones(N, bool)
    cut_counts, mixed, turned_total = set(), 0, 0
    for rpb, visible in ((8192, everything), (4096, everything), (DEFAULT_RPB, everything), (8192, w["half"])):
        for lo in range(0, N, rpb):
            tile = [schedule(w["d"][q], visible, lo, min(lo + rpb, N), 256) for q in range(8)]      # the first tile's eight lists
            cut_counts |= {len(c) for c, _ in tile}
            turned_total += sum(t for _, t in tile)
            rounds = set().union(*[set(c) for c, _ in tile])
            mixed += sum(1 for r in rounds if 0 < sum(r in c for c, _ in tile) < 8)
    assert 0 in cut_counts and 1 in cut_counts and max(cut_counts) >= 2, cut_counts
    assert mixed >= 1 and turned_total > 1000, (mixed, turned_total)
    assert schedule(w["d"][0], everything, 0, 64, 256) == ([], 0)


def test_more_queries_than_one_slice_and_a_raised_rows_per_block():
    """300 queries: a slice of 256 and one of 44, each with its own offsets into qcodes and the outputs.  At rows_per_block = 64 the
    9000 rows would make 141 partial lists per query, more than the workspace's 2^15 slots hold for 256 queries (128): raised."""
    w = base(64)
    rs = np.random.RandomState(5)
    qcodes = rs.randint(0, 2 ** 63, (300, 1), dtype=np.int64).view(np.uint64) * np.uint64(2) + rs.randint(0, 2, (300, 1)).astype(np.uint64)
    qcodes[256:] = w["qcodes"][:44]
    dq = dev(qcodes.view(np.int64), np.int64)
    for R in (10, 256):
        want = B.candidates_host(w["codes"], qcodes, R)
        for rpb in (None, 64):
            assert same(B.candidates_device(w["dcodes"], dq, R, rows_per_block=rpb), want), (R, rpb)
        assert np.array_equal(want[0][256:], host(w, R, False)[0][:44])
    want = B.candidates_host(w["codes"], qcodes, 32, w["half"])
    assert same(B.candidates_device(w["dcodes"], dq, 32, allow=w["dhalf"]), want)


def test_a_rescore_of_more_than_1024_queries():
    rs = np.random.RandomState(9)
    X = (rs.randn(200, 64) / 8 + 0.05).astype(np.float16)
    Q = (rs.randn(1100, 64) / 8 + 0.05).astype(np.float16)
    bi = B.BinaryIndex.build(ShardIndex(dev(X, np.float16), idx_base=300, prefilter=None), centre="mean")
    s, i, n = (t.cpu().numpy() for t in bi.search(dev(Q, np.float16), 10, 40))
    centre = bi.centre.cpu().numpy()
    ws, wi, wn = B.search_host(X, B.pack_host(X, centre), B.pack_host(Q, centre), Q, 10, 40)
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(i, wi + 300) and np.array_equal(n, wn) and (n == 40).all()


def test_tensors_of_the_wrong_kind_are_value_errors():
    w = base(64)
    for bad, part in ((dict(codes=w["dcodes"].cpu()), "codes"), (dict(codes=w["dcodes"].int()), "codes"), (dict(qcodes=w["dqcodes"][:, :0]), "qcodes"),
                      (dict(qcodes=w["dqcodes"].float()), "qcodes"), (dict(allow=w["dhalf"][:-1]), "allow"), (dict(allow=w["dhalf"].cpu()), "allow"),
                      (dict(allow=w["dhalf"][::2]), "allow")):
        args = {"codes": w["dcodes"], "qcodes": w["dqcodes"], "allow": None, **bad}
        with pytest.raises(ValueError, match=part):
            B.candidates_device(args["codes"], args["qcodes"], 10, allow=args["allow"])
    x = torch.zeros((4, 64), dtype=torch.float16, device=DEV)
    for rows, centre, part in ((x.float(), None, "rows"), (x.cpu(), None, "rows"), (x[:, ::1].t(), None, "rows"), (x, torch.zeros(64, device=DEV).double(), "centre"),
                               (x, torch.zeros(65, device=DEV), "centre")):
        with pytest.raises(ValueError, match=part):
            B.pack_device(rows, centre)


# ---- odd W above 1, and W = 128 -----------------------------------------------------------------------------------------------------------
N_W, LINE = 1000, 1 << 20
N_BIG = 2 * LINE + 64 * 3 + 5                                    # three blocks at rows_per_block = 2^20; the last wave holds 5 rows


@pytest.fixture(scope="module")
def wide():
    """dim -> random code words of 1000 rows and 70 queries (the scan reads words, whatever packed them), two identical rows and a query
    equal to them, a half-random bitmap, and the host lists at R = 256 (a shorter list is their prefix); built once, left unchanged"""
    built = {}

    def get(dim):
        if dim not in built:
            W = dim // 64
            rs = np.random.RandomState(dim)
            codes = rs.randint(0, 2 ** 63, (N_W, W), dtype=np.int64).view(np.uint64) * np.uint64(2) + rs.randint(0, 2, (N_W, W)).astype(np.uint64)
            qcodes = codes[rs.randint(0, N_W, NQ)] ^ (rs.randint(0, 2 ** 62, (NQ, W), dtype=np.int64).view(np.uint64)
                                                      & rs.randint(0, 2 ** 62, (NQ, W), dtype=np.int64).view(np.uint64))
            codes[700] = codes[10]
            qcodes[0] = codes[10]
            half = rs.rand(N_W) < 0.5
            built[dim] = dict(codes=codes, qcodes=qcodes, half=half, dcodes=dev(codes.view(np.int64), np.int64),
                              dqcodes=dev(qcodes.view(np.int64), np.int64), dhalf=dev(pack_bitmap(half).view(np.int64), np.int64),
                              want=B.candidates_host(codes, qcodes, 256), want_half=B.candidates_host(codes, qcodes, 256, half))
        return built[dim]
    yield get
    built.clear()


def prefix(full, R):
    cand, dist, count = full
    return cand[:, :R], dist[:, :R], np.minimum(count, R)


@pytest.mark.parametrize("dim", [192, 8128, 8192])
def test_odd_word_counts_above_one_and_the_widest_code(wide, dim):
    """W = 3 and W = 127 take the one-word load (W odd) with a row stride that is no multiple of 16 bytes; W = 128 fills the query
    words' LDS array.  1000 rows, 70 queries (a full tile and a ragged one), exactly `candidates_host`."""
    w = wide(dim)
    assert w["codes"].shape[1] == dim // 64 and (dim // 64) % 2 == (0 if dim == 8192 else 1)
    for R in (1, 256):
        for rpb in (None, 64):
            assert same(B.candidates_device(w["dcodes"], w["dqcodes"], R, rows_per_block=rpb), prefix(w["want"], R)), (dim, R, rpb)
        assert same(B.candidates_device(w["dcodes"], w["dqcodes"], R, allow=w["dhalf"]), prefix(w["want_half"], R)), (dim, R, "half")
    cand, dist, _ = w["want"]
    assert cand[0, :2].tolist() == [10, 700] and dist[0, :2].tolist() == [0, 0]
    assert len(set(dist[:, 0].tolist())) > 5 and dist[:, 255].min() > 0      # the queries are not all alike, and no list is all ties


# ---- beyond 2^20 rows ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """2^21 + 197 rows of one random word, 9 queries.  Planted: query 0's 300 nearest rows (distance 1) all lie beyond 2^20, a thousand
    rows apart; query 1 has 260 rows at distance 0 across 2^20 - 130 ... 2^20 + 129; query 2's best row is the shard's last.  Random
    words lie at distance 8 or more from a query (a distance below 8 has probability 4e-11 per row, 2^21 rows)."""
    rs = np.random.RandomState(77)
    codes = rs.randint(0, 2 ** 63, (N_BIG, 1), dtype=np.int64).view(np.uint64) * np.uint64(2) + rs.randint(0, 2, (N_BIG, 1)).astype(np.uint64)
    qcodes = rs.randint(0, 2 ** 63, (9, 1), dtype=np.int64).view(np.uint64) * np.uint64(2) + rs.randint(0, 2, (9, 1)).astype(np.uint64)
    near = LINE + 1000 * np.arange(1, 301) + 3
    codes[near, 0] = qcodes[0, 0] ^ (np.uint64(1) << (np.arange(300) % 64).astype(np.uint64))
    codes[LINE - 130:LINE + 130, 0] = qcodes[1, 0]
    codes[N_BIG - 1, 0] = qcodes[2, 0]
    hidden = np.ones(N_BIG, bool)
    hidden[near[:3]] = False; hidden[[LINE - 1, LINE, N_BIG - 1]] = False
    words = pack_bitmap(hidden).copy()
    words[-1] |= np.uint64(0xffffff) << np.uint64(40)            # bits beyond the last row: they name no row
    half = rs.rand(N_BIG) < 0.5
    w = dict(codes=codes, qcodes=qcodes, near=near, dcodes=dev(codes.view(np.int64), np.int64), dqcodes=dev(qcodes.view(np.int64), np.int64),
             masks={"none": (None, None), "hidden": (hidden, dev(words.view(np.int64), np.int64)),
                    "half": (half, dev(pack_bitmap(half).view(np.int64), np.int64))})
    w["want"] = {name: B.candidates_host(codes, qcodes, 256, m) for name, (m, _) in w["masks"].items()}
    yield w
    w.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mask", ["none", "hidden", "half"])
def test_rows_beyond_2_20_enter_the_keys_low_word(big, mask):
    want = big["want"][mask]
    for R in (1, 256):
        for rpb in (None, LINE):
            got = B.candidates_device(big["dcodes"], big["dqcodes"], R, allow=big["masks"][mask][1], rows_per_block=rpb)
            assert same(got, prefix(want, R)), (mask, R, rpb)
    cand, dist, count = want
    assert (count == 256).all()
    near = big["near"]
    if mask == "none":
        assert cand[0].tolist() == near[:256].tolist() and (dist[0] == 1).all()
        assert cand[1].tolist() == list(range(LINE - 130, LINE + 126)) and (dist[1] == 0).all()
        assert cand[2, 0] == N_BIG - 1 and dist[2, 0] == 0 and dist[2, 1] >= 8
    if mask == "hidden":
        assert cand[0].tolist() == near[3:259].tolist()
        assert cand[1].tolist() == [r for r in range(LINE - 130, LINE + 130) if r not in (LINE - 1, LINE)][:256]
        assert cand[2, 0] != N_BIG - 1 and dist[2, 0] >= 8
    assert sum(int((cand[q] >= LINE).sum()) > 64 for q in range(9)) >= 3
