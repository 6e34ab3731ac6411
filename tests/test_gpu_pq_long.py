"""arx_pq_encode / arx_pq_lut / arx_pq_candidates (csrc/pq.hip) past the shapes of tests/test_gpu_pq.py: every reachable instantiation of
the scan kernel on both sides of every tile boundary, calls of more than one query slice, shards beyond 2^20 rows whose blocks are cut
many times, and encode / lut at the dsub and dim the small suite leaves out, up to dim 8192.

Every comparison is exact, against the numpy restatement of arxiv_rag_amd/pq.py (`encode_host`, `lut_host`, `sums_host`,
`candidates_host`, `search_host`).  The scan is integer work: the restatement is its high-precision reference.  The tests without the
`gpu` mark hold the arithmetic the GPU tests rely on (which instantiation an M takes, when rows_per_block is raised, how often the lists
of the large shard are cut) against constants read out of the sources: if a constant changes they fail, and the coverage does not move
silently."""
import numpy as np
import pytest

from arxiv_rag_amd import pq as P
from arxiv_rag_amd.where import pack_bitmap
from tests.key_list_cases import KEY_CAP, KEY_NT, KEY_QBATCH, KEY_R_MAX, constexpr, key_slots, pq_keys, rows_per_block, schedule

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
DEV = "cuda:0"

PQ_LDS_BLOCK = constexpr("pq.hip", "PQ_LDS_BLOCK")
PQ_RPB_LIMIT = constexpr("pq.hip", "PQ_RPB_LIMIT")
PQ_BLOCKS_TARGET = constexpr("pq.hip", "PQ_BLOCKS_TARGET")
PQ_RPB_MIN_DEFAULT = constexpr("pq.hip", "PQ_RPB_MIN_DEFAULT")
PQ_M_MAX = constexpr("pq.hip", "PQ_M_MAX")
LINE = 1 << 20


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host_of(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def same(got, want):
    return all(np.array_equal(g, x) for g, x in zip(host_of(got), want))


def cut(full, R, qs=slice(None)):
    """the lists at R from the lists at 256: a shorter list is a prefix by definition"""
    cand, sums, count = full
    return cand[qs, :R], sums[qs, :R], np.minimum(count[qs], R)


# ---- the scan's instantiations, restated ------------------------------------------------------------------------------------------------
def lists_bytes(qt):
    """pq_lists_bytes<QT>: sizeof(KeyLists<QT>) (keys, thresholds, counters; 8-byte aligned) rounded up to 16"""
    size = (qt * KEY_CAP * 8 + qt * 8 + qt * 4 + 7) // 8 * 8
    return (size + 15) // 16 * 16


def scan_smem(qt, M):
    return lists_bytes(qt) + qt * M * 256


def pq_tile(M):
    return next((qt for qt in (8, 4, 2) if scan_smem(qt, M) <= PQ_LDS_BLOCK), 1)


def instantiation(M):
    """(QT, V) of key_scan_kernel<PqCode<QT, V>> for M subspaces: pq_tile and PqScan::launch"""
    return pq_tile(M), 16 if M % 16 == 0 else 4 if M % 4 == 0 else 1


# M -> (dim, dsub) handed to the library: the scan reads M alone
SCAN_SHAPES = {4: (256, 64), 7: (448, 64), 8: (512, 64), 9: (576, 64), 16: (1024, 64), 47: (3008, 64), 48: (3072, 64), 52: (3328, 64), 127: (8128, 64),
               128: (8192, 64), 130: (4160, 32), 132: (2112, 16)}
SCAN_PAIRS = {4: (8, 4), 7: (8, 1), 8: (4, 4), 9: (4, 1), 16: (4, 16), 47: (4, 1), 48: (2, 16), 52: (2, 4), 127: (2, 1), 128: (1, 16), 130: (1, 1), 132: (1, 4)}


def test_the_shapes_take_every_reachable_instantiation_and_sit_on_every_boundary():
    """CPU only.  11 of the 12 (QT, V) pairs are reachable (QT = 8 holds M <= 7: no multiple of 16), the listed M take each of them,
    and they stand on both sides of every change of the tile, 7 | 8 (and 9, the first M of the tile of 4 with one-byte loads), 47 | 48 and
    127 | 128, where the dynamic LDS is within a few hundred bytes of PQ_LDS_BLOCK."""
    assert (KEY_NT, KEY_CAP, KEY_R_MAX, PQ_LDS_BLOCK, PQ_M_MAX) == (256, 1024, 256, 80 * 1024, 256)
    assert [lists_bytes(qt) for qt in (8, 4, 2, 1)] == [65632, 32816, 16416, 8208]
    reachable = {instantiation(M) for M in range(1, PQ_M_MAX + 1)}
    assert len(reachable) == 11 and (8, 16) not in reachable
    assert {M: instantiation(M) for M in SCAN_SHAPES} == SCAN_PAIRS and set(SCAN_PAIRS.values()) == reachable
    changes = [M for M in range(1, PQ_M_MAX) if pq_tile(M) != pq_tile(M + 1)]
    assert changes == [7, 47, 127]
    assert (pq_tile(7), pq_tile(8), pq_tile(9)) == (8, 4, 4) and {7, 8, 9, 47, 48, 127, 128} <= set(SCAN_SHAPES)
    assert [PQ_LDS_BLOCK - scan_smem(pq_tile(M), M) for M in (7, 47, 127)] == [1952, 976, 480]      # the fullest blocks of each tile
    assert scan_smem(1, PQ_M_MAX) == 73744 <= PQ_LDS_BLOCK
    for M, (dim, dsub) in SCAN_SHAPES.items():
        assert dim == M * dsub and P.check_dsub(dim, dsub) == M
    # the two-slice test: M = 8, 96, 256 are tiles of 4, 2 and 1 queries, so 256 + 45 queries end both slices of M = 8 and 96 ... ragged
    assert [pq_tile(M) for M in (8, 96, 256)] == [4, 2, 1] and 45 % 4 and 45 % 2 and 301 - KEY_QBATCH == 45


# ---- a. every instantiation: random code bytes and random table bytes ------------------------------------------------------------------------
N_A, NQ_A = 5000, 9                                             # 9 queries: the last tile is ragged for every QT


@pytest.fixture(scope="module")
def scan_cases():
    """M -> codes, tables (with tests/test_gpu_pq.py's zero, 255, 0 / 1 and long-tie tables), a bitmap with whole zero words and garbage
    bits past the last row, and the host lists at R = 256 with and without it; built on first use, left unchanged"""
    built = {}

    def get(M):
        if M not in built:
            rs = np.random.RandomState(9000 + M)
            codes = rs.randint(0, 256, (N_A, M)).astype(np.uint8)
            lut = rs.randint(0, 256, (NQ_A, M, 256)).astype(np.uint8)
            lut[1] = 0
            lut[2] = 255
            lut[3] = 0
            lut[3, 0, :128] = 1
            lut[4] = rs.randint(0, 2, (M, 256))
            codes[4000] = codes[10]
            mask = rs.rand(N_A) < 0.7
            mask[64:256] = False; mask[320:384] = False; mask[4992:] = False            # whole words of zeros, the last one among them
            words = pack_bitmap(mask).copy()
            words[-1] |= np.uint64(0xffffff) << np.uint64(40)                          # rows 5032 ... 5055: they name no row
            built[M] = dict(codes=codes, lut=lut, mask=mask, dcodes=dev(codes, np.uint8), dlut=dev(lut, np.uint8),
                            dallow=dev(words.view(np.int64), np.int64), want=P.candidates_host(codes, lut, 256),
                            want_masked=P.candidates_host(codes, lut, 256, mask))
        return built[M]
    yield get
    built.clear()


@gpu
@pytest.mark.parametrize("M", sorted(SCAN_SHAPES))
def test_every_scan_instantiation_equals_the_definition(scan_cases, M):
    w = scan_cases(M)
    dsub = SCAN_SHAPES[M][1]
    for R in (1, 40, 256):
        for rpb in (None, 64):
            got = P.candidates_device(w["dcodes"], w["dlut"], dsub, R, rows_per_block=rpb)
            assert same(got, cut(w["want"], R)), (M, R, rpb)
            got = P.candidates_device(w["dcodes"], w["dlut"], dsub, R, allow=w["dallow"], rows_per_block=rpb)
            assert same(got, cut(w["want_masked"], R)), (M, R, rpb, "masked")
    cand, sums, count = w["want"]
    assert cand[1].tolist() == list(range(256)) and (sums[1] == 0).all() and (sums[2] == 255 * M).all() and (count == 256).all()
    assert set(sums[3].tolist()) == {1} and len(set(sums[0].tolist())) > 3
    c = w["want_masked"][0]
    assert w["mask"][c[c >= 0]].all() and (w["want_masked"][2] == 256).all()


# ---- b. two slices ---------------------------------------------------------------------------------------------------------------------------
N_B, NQ_B = 9000, 301


@pytest.fixture(scope="module")
def slice_cases():
    """M -> 9000 rows and 301 tables, the last 45 copies of the first 45; the host lists of the first 256 tables (the copies' lists are
    copies), with and without a half-random bitmap"""
    built = {}

    def get(M):
        if M not in built:
            rs = np.random.RandomState(500 + M)
            codes = rs.randint(0, 256, (N_B, M)).astype(np.uint8)
            lut = rs.randint(0, 256, (NQ_B, M, 256)).astype(np.uint8)
            lut[KEY_QBATCH:] = lut[:NQ_B - KEY_QBATCH]
            half = rs.rand(N_B) < 0.5
            want = {}
            for name, m in (("all", None), ("half", half)):
                first = P.candidates_host(codes, lut[:KEY_QBATCH], 256, m)
                want[name] = tuple(np.concatenate([a, a[:NQ_B - KEY_QBATCH]]) for a in first)
            built[M] = dict(codes=codes, lut=lut, dcodes=dev(codes, np.uint8), dlut=dev(lut, np.uint8), want=want,
                            dallow={"all": None, "half": dev(pack_bitmap(half).view(np.int64), np.int64)})
        return built[M]
    yield get
    built.clear()


def test_a_second_slice_and_a_raised_rows_per_block_from_host_arithmetic():
    """CPU only: 301 queries are a slice of 256 and one of 45.  At rows_per_block = 64 the 9000 rows make 141 parts, more than the 128
    the workspace's 2^15 slots hold for each of 256 queries: the first slice's rows_per_block is raised to 128, the second's is not."""
    assert key_slots(N_B, NQ_B) == 1 << 15 and (N_B + 63) // 64 == 141 > (1 << 15) // KEY_QBATCH == 128
    for M in (8, 96, 256):
        kw = dict(blocks_target=PQ_BLOCKS_TARGET, rpb_min_default=PQ_RPB_MIN_DEFAULT)
        assert rows_per_block(N_B, NQ_B, pq_tile(M), 64, **kw) == [(256, 128, 71), (45, 64, 141)]
        first = (256, 2304, 4) if M == 256 else (256, 2048, 5)       # 256 tiles of one query: 4 blocks each are the default's target
        assert rows_per_block(N_B, NQ_B, pq_tile(M), 0, **kw) == [first, (45, 2048, 5)]


@gpu
@pytest.mark.parametrize("M", [8, 96, 256])
def test_more_queries_than_one_slice(slice_cases, M):
    """The second slice reads its tables at lut + 256 M 256 and writes at out + 256 R: its 45 tables are copies of the first 45, so its
    lists must equal those of the first slice, which are not all alike.  Copies alone would hide a second slice that read the call's first
    tables, so one more run moves the tables on by 100 queries."""
    w = slice_cases(M)
    dsub = 8
    for name in ("all", "half"):
        want = w["want"][name]
        for R in (10, 256):
            for rpb in (None, 64):
                got = host_of(P.candidates_device(w["dcodes"], w["dlut"], dsub, R, allow=w["dallow"][name], rows_per_block=rpb))
                assert all(np.array_equal(g, x) for g, x in zip(got, cut(want, R))), (M, name, R, rpb)
                for g in got:
                    assert np.array_equal(g[KEY_QBATCH:], g[:NQ_B - KEY_QBATCH]), (M, name, R, rpb, "the second slice")
        # the tables moved on by 100 queries: the second slice now holds tables 156 ... 200, which are nobody's copies
        got = host_of(P.candidates_device(w["dcodes"], torch.roll(w["dlut"], 100, 0).contiguous(), dsub, 10, allow=w["dallow"][name]))
        assert all(np.array_equal(g, np.roll(x, 100, axis=0)) for g, x in zip(got, cut(want, 10))), (M, name, "tables rolled by 100")
        assert not np.array_equal(want[0][156:201, :10], want[0][201:246, :10])      # (what a slice reading from the call's first table returns)
        first = want[0][:NQ_B - KEY_QBATCH, :10]
        assert len({tuple(r) for r in first.tolist()}) == NQ_B - KEY_QBATCH, (M, name, "the first 45 lists are not distinct")


# ---- c. beyond 2^20 rows -----------------------------------------------------------------------------------------------------------------
N_C, M_C, NQ_C = 2 * LINE + 64 * 3 + 5, 4, 9
RAMP = (LINE + 8192, LINE + 8192 + 65536)                        # rows whose byte 3 climbs by one every 1024 rows
_BIG = {}


def big_case():
    """2^21 + 197 rows of 4 code bytes and 9 tables, host data only (the CPU tests use it too), built once.  Byte value 255 is kept for
    the planted rows: in subspace 0 it occurs only at or beyond row 2^20 (about one row in 256 there), in subspace 1 only in the 260
    rows around 2^20, in subspace 2 only in the last row.
      table 0   zero but for [0][255]: the top sum belongs to rows >= 2^20 only; the list is the first R of them, ascending
      table 1   zero but for [1][255]: 260 rows tie at the top across 2^20 - 130 ... 2^20 + 129
      table 2   random below 200, no weight on a byte 255 but [2][255] = 255; the last row holds the best byte of every subspace
      table 3   zero: rows 0 ... R - 1
      table 4   zero but for [3][j] = j, and byte 3 is 192 + (row - RAMP[0]) / 1024 over RAMP and below 192 elsewhere: the sum climbs
                with the row there, so a block's list is cut again and again
      tables 5 ... 8 random"""
    if not _BIG:
        rs = np.random.RandomState(2021)
        codes = rs.randint(0, 256, (N_C, M_C)).astype(np.uint8)
        codes[:LINE, 0][codes[:LINE, 0] == 255] = 254
        codes[:, 1][codes[:, 1] == 255] = 254
        codes[:, 2][codes[:, 2] == 255] = 254
        codes[:, 3][codes[:, 3] >= 192] -= 64
        codes[RAMP[0]:RAMP[1], 3] = (192 + np.arange(RAMP[1] - RAMP[0]) // 1024).astype(np.uint8)
        codes[LINE - 130:LINE + 130, 1] = 255
        lut = rs.randint(0, 256, (NQ_C, M_C, 256)).astype(np.uint8)
        lut[0] = 0; lut[0, 0, 255] = 200
        lut[1] = 0; lut[1, 1, 255] = 255
        lut[2] = rs.randint(0, 200, (M_C, 256)); lut[2, :, 255] = 0; lut[2, 2, 255] = 255
        lut[3] = 0
        lut[4] = 0; lut[4, 3] = np.arange(256)
        codes[N_C - 1] = lut[2].argmax(axis=1)
        assert codes[N_C - 1, 2] == 255 and (codes[N_C - 1, [0, 1, 3]] != 255).all()
        top0 = np.flatnonzero(codes[:, 0] == 255)
        hidden = np.ones(N_C, bool)
        hidden[top0[:3]] = False; hidden[[0, LINE - 1, LINE, N_C - 1]] = False; hidden[RAMP[1] - 1024:RAMP[1]] = False
        words = pack_bitmap(hidden).copy()
        words[-1] |= np.uint64(0xffffff) << np.uint64(40)        # bits beyond the last row
        half = rs.rand(N_C) < 0.5
        masks = {"none": (None, None), "hidden": (hidden, words), "half": (half, pack_bitmap(half))}
        _BIG.update(codes=codes, lut=lut, top0=top0, masks=masks, sums=P.sums_host(codes, lut),
                    want={name: P.candidates_host(codes, lut, 256, m) for name, (m, _) in masks.items()})
    return _BIG


def test_the_large_shards_lists_are_cut_often_never_and_turn_keys_away():
    """CPU only, from the restated bookkeeping (tests/key_list_cases.py) over the blocks the three rows_per_block settings give: lists
    cut three times and more (table 4 over its ramp, a random table in a block of 2^20 rows), lists never cut (the last block of 197
    rows), keys turned away by a non-zero threshold; and what the planted tables promise."""
    w = big_case()
    kw = dict(blocks_target=PQ_BLOCKS_TARGET, rpb_min_default=PQ_RPB_MIN_DEFAULT)
    assert pq_tile(M_C) == 8
    default = rows_per_block(N_C, NQ_C, 8, 0, **kw)
    assert default == [(9, 4352, 482)] and default[0][1] > PQ_RPB_MIN_DEFAULT
    assert rows_per_block(N_C, NQ_C, 8, 4096, **kw) == [(9, 4096, 513)] and rows_per_block(N_C, NQ_C, 8, PQ_RPB_LIMIT, **kw) == [(9, LINE, 3)]
    everything = np.ones(N_C, bool)
    keys = [pq_keys(w["sums"][q]) for q in range(NQ_C)]
    found = {}
    for rpb, q, block, visible in ((4352, 4, (RAMP[0] + 8192) // 4352, everything), (4096, 4, (RAMP[0] + 8192) // 4096, everything),
                                   (4352, 3, 0, everything), (4352, 5, 100, everything), (4352, 5, 300, w["masks"]["half"][0]),
                                   (LINE, 5, 1, everything), (LINE, 0, 1, w["masks"]["hidden"][0]), (LINE, 6, 2, everything),
                                   (4352, 0, 481, everything)):
        lo = block * rpb
        found[(rpb, q, block)] = schedule(keys[q], visible, lo, min(lo + rpb, N_C), 256)
    counts = {key: (len(c), t) for key, (c, t) in found.items()}
    print("cuts and keys turned away per (rows_per_block, table, block):", counts)
    assert min(counts[(4352, 4, (RAMP[0] + 8192) // 4352)][0], counts[(4096, 4, (RAMP[0] + 8192) // 4096)][0]) >= 3, counts
    assert counts[(LINE, 5, 1)][0] >= 3 and counts[(LINE, 5, 1)][1] > 1 << 19, counts
    assert counts[(LINE, 6, 2)] == (0, 0) and counts[(4352, 3, 0)][0] >= 1 and counts[(4352, 3, 0)][1] > 2048, counts
    assert counts[(4352, 5, 100)][0] >= 1 and counts[(4352, 5, 100)][1] > 0 and counts[(4352, 5, 300)][0] >= 1, counts
    assert sum(1 for c, t in counts.values() if c == 0) >= 1 and sum(1 for c, t in counts.values() if c >= 3) >= 3, counts
    # the planted tables
    cand, sums, count = w["want"]["none"]
    top0 = w["top0"]
    assert top0[0] >= LINE and top0.shape[0] > 2000 and cand[0].tolist() == top0[:256].tolist() and (sums[0] == 200).all()
    assert cand[1].tolist() == list(range(LINE - 130, LINE + 126)) and (sums[1] == 255).all()
    assert cand[2, 0] == N_C - 1 and sums[2, 0] > sums[2, 1] and (N_C - 1) % 64 == 4 and N_C % KEY_NT == 197
    assert cand[3].tolist() == list(range(256)) and (sums[3] == 0).all()
    assert cand[4].tolist() == list(range(RAMP[1] - 1024, RAMP[1] - 768)) and (sums[4] == 255).all()
    hc = w["want"]["hidden"][0]
    assert hc[0].tolist() == top0[3:259].tolist() and hc[2, 0] != N_C - 1 and hc[3].tolist() == list(range(1, 257))
    assert hc[1].tolist() == [r for r in range(LINE - 130, LINE + 130) if r not in (LINE - 1, LINE)][:256]
    assert hc[4].tolist() == list(range(RAMP[1] - 2048, RAMP[1] - 2048 + 256))
    for name in ("none", "hidden", "half"):
        c = w["want"][name][0]
        assert (w["want"][name][2] == 256).all()
        assert sum(int((c[q] >= LINE).sum()) > 64 for q in range(NQ_C)) >= 3, name


@pytest.fixture(scope="module")
def big_on_device():
    w = big_case()
    d = dict(dcodes=dev(w["codes"], np.uint8), dlut=dev(w["lut"], np.uint8),
             dallow={name: None if words is None else dev(words.view(np.int64), np.int64) for name, (_, words) in w["masks"].items()})
    yield d
    d.clear()
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("mask", ["none", "hidden", "half"])
def test_rows_beyond_2_20_and_blocks_cut_many_times(big_on_device, mask):
    w, d = big_case(), big_on_device
    for R in (1, 256):
        for rpb in (None, 4096, PQ_RPB_LIMIT):
            got = P.candidates_device(d["dcodes"], d["dlut"], 64, R, allow=d["dallow"][mask], rows_per_block=rpb)
            assert same(got, cut(w["want"][mask], R)), (mask, R, rpb)


# ---- d. encode and lut at the dsub and dims the small suite leaves out ----------------------------------------------------------------------
ENC_SHAPES = ((64, 16), (64, 32), (1024, 4), (8192, 32), (8192, 64), (8128, 64))
N_ENC = (1, 255, 256, 257, 300)                                  # 300 rows: a full block of 256 and a ragged one


@pytest.fixture(scope="module")
def enc_cases():
    """(dim, dsub) -> 300 rows, 9 queries, a centre and codebooks with the special values of tests/test_gpu_pq.py's `enc_base` (NaN / inf
    rows, duplicated centroids, a zero query, queries with an inf and a NaN), and their host codes and tables; a row's code does not
    depend on the other rows, so a prefix's codes are a prefix of them"""
    built = {}

    def get(dim, dsub):
        if (dim, dsub) not in built:
            M = dim // dsub
            rs = np.random.RandomState(dim + dsub)
            X = (rs.randn(300, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
            centre = X.astype(np.float32).mean(axis=0)
            X[3, :5] = (np.nan, np.inf, -np.inf, -0.0, 65504.0)
            X[7] = np.nan
            X[270, -1] = np.inf
            X[299, 0] = -np.inf
            cb = np.ascontiguousarray((X[8:264].astype(np.float32) - centre).reshape(256, M, dsub).transpose(1, 0, 2))
            cb[:, 200] = cb[:, 17]
            cb[:, 255] = cb[:, 0]
            X[5] = (cb[:, 17].reshape(-1) + centre).astype(np.float16)
            Q = (rs.randn(9, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
            Q[2] = 0
            Q[4, dim // 2] = np.inf
            Q[5, 1] = np.nan
            built[(dim, dsub)] = dict(X=X, Q=Q, cb=cb, dcb=dev(cb, np.float32), dcentre=dev(centre, np.float32),
                                      codes=P.encode_host(X, cb, centre), codes0=P.encode_host(X, cb, None), lut=P.lut_host(Q, cb))
        return built[(dim, dsub)]
    yield get
    built.clear()


def test_the_encode_shapes_reach_the_largest_dynamic_lds():
    """CPU only: arx_pq_encode asks for 1 KiB dsub of codebook and 256 M code bytes; (8192, 32) and (8192, 64) are the two shapes at 96 KiB"""
    lds = {(dim, dsub): 256 * dsub * 4 + KEY_NT * (dim // dsub) for dim, dsub in ENC_SHAPES}
    assert lds[(8192, 32)] == lds[(8192, 64)] == 96 * 1024 == max(256 * ds * 4 + KEY_NT * min(8192 // ds, PQ_M_MAX) for ds in P.DSUBS)
    assert constexpr("pq.hip", "PQ_DIM_MAX") == 8192 and {ds for _, ds in ENC_SHAPES} == {4, 16, 32, 64}


@gpu
@pytest.mark.parametrize("dim,dsub", ENC_SHAPES)
def test_encode_and_lut_equal_the_definition(enc_cases, dim, dsub):
    w = enc_cases(dim, dsub)
    M = dim // dsub
    for n in N_ENC:
        x = dev(w["X"][:n], np.float16).reshape(n, dim)
        got = P.encode_device(x, dsub, w["dcentre"], w["dcb"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, M)
        assert np.array_equal(got.cpu().numpy(), w["codes"][:n]), (dim, dsub, n, "centre")
        assert np.array_equal(P.encode_device(x, dsub, None, w["dcb"]).cpu().numpy(), w["codes0"][:n]), (dim, dsub, n, "no centre")
    assert (w["codes"][7] == 0).all() and (w["codes"][5] == 17).all() or dsub < 8
    assert not (w["codes"] == 200).any() and not (w["codes"] == 255).any() and not np.array_equal(w["codes"], w["codes0"])
    assert len(np.unique(w["codes"])) > 100
    for nq in (1, 9):
        got = P.lut_device(dev(w["Q"][:nq], np.float16), dsub, w["dcb"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (nq, M, 256)
        assert np.array_equal(got.cpu().numpy(), w["lut"][:nq]), (dim, dsub, nq)
    assert not w["lut"][2].any() and not w["lut"][4].any() and not w["lut"][5].any()
    assert w["lut"][0].max() == 255 and w["lut"][0].min() == 0


# ---- e. end to end at dim 8192 -----------------------------------------------------------------------------------------------------------
@gpu
def test_search_at_dim_8192_equals_the_definition_and_the_filtered_search_over_the_candidates():
    from arxiv_rag_amd.index import ShardIndex
    dim, dsub, n, nq, k, R = 8192, 32, 300, 9, 10, 40
    M = dim // dsub
    rs = np.random.RandomState(8192)
    X = (rs.randn(n, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
    X[200] = X[10]
    Q = (rs.randn(nq, dim) / np.sqrt(dim) + 0.05).astype(np.float16)
    Q[0] = X[10]
    centre = X.astype(np.float32).mean(axis=0)
    cb = np.ascontiguousarray((X[rs.permutation(n)[:256]].astype(np.float32) - centre).reshape(256, M, dsub).transpose(1, 0, 2))
    codes, lut = P.encode_host(X, cb, centre), P.lut_host(Q, cb)
    dQ = dev(Q, np.float16)
    index = ShardIndex(dev(X, np.float16), prefilter=None)
    pi = P.PqIndex.build(index, dsub=dsub, centre=centre, codebooks=cb)
    assert np.array_equal(pi.codes.cpu().numpy(), codes)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    s, i, cnt = host_of(pi.search(dQ, k, R))
    ws, wi, wn = P.search_host(X, codes, lut, Q, k, R)
    assert np.array_equal(bits(s), bits(ws)) and np.array_equal(i, wi) and np.array_equal(cnt, wn) and (cnt == R).all()
    cand = P.candidates_host(codes, lut, R)[0]
    assert np.array_equal(pi.candidates(dQ, R)[0].cpu().numpy(), cand)
    for q in range(nq):
        mask = np.zeros(n, bool); mask[cand[q]] = True
        fs, fi = index.search(dQ[q:q + 1].contiguous(), k, allow=dev(pack_bitmap(mask).view(np.int64), np.int64))
        assert np.array_equal(bits(fs.cpu().numpy()), bits(s[q:q + 1])) and np.array_equal(fi.cpu().numpy(), i[q:q + 1]), q
    assert i[0, 0] == 10 and i[0, 1] == 200
