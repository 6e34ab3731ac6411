"""arx_cluster_sums / arx_cluster_sums_tuned / arx_cluster_finish (csrc/cluster.hip) on the device (-m gpu): bit for bit against the
numpy restatement (`topics.sums_host`, `topics.finish_host`), the same bits under every launch shape, float64 within the derived
two-level bound, and the defined behaviour on bad device data.  The labels are hand-made, not taken from an assign; every sum lands
between canary rows."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import topics as T
from tests import topics_fp64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 255, 256, 257, 600, 131)                        # 600 = three runs; the others sit on every run edge
CANARY = -12345.5
U = 2.0 ** -24


def hand_labels(n, sizes, seed):
    """labels with exactly these cluster sizes, the members interleaved over the rows."""
    assert sum(sizes) == n
    lab = np.concatenate([np.full(m, c) for c, m in enumerate(sizes)])
    return np.random.RandomState(seed).permutation(lab).astype(np.int32)


_CASES = {}


def case(dim, n=1500, sizes=SIZES):
    """(X fp16, labels, order, start, sums_host) of one shape, computed once and shared."""
    if (dim, n) not in _CASES:
        X = (np.random.RandomState(dim).randn(n, dim) * 0.3).astype(np.float16)
        labels = hand_labels(n, sizes, dim + 1)
        order, start, _ = T.members_host(labels, len(sizes))
        _CASES[(dim, n)] = (X, labels, order, start, T.sums_host(X, order, start))
    return _CASES[(dim, n)]


def device_sums(X, order, start, C, tuned=None):
    """`arx_cluster_sums` into the middle of a canary-filled buffer -> the sums, after checking the canaries."""
    dim = X.shape[1]
    buf = torch.full((C + 2, dim), CANARY, dtype=torch.float32, device=DEV)
    out = buf[1:C + 1]
    T.cluster_sums(torch.from_numpy(X).to(DEV), torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(DEV),
                   torch.from_numpy(np.ascontiguousarray(start, dtype=np.int64)).to(DEV), C, tuned=tuned, out=out)
    got = buf.cpu().numpy()
    assert (got[0] == CANARY).all() and (got[-1] == CANARY).all()
    return got[1:-1]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("dim", [64, 192])
def test_sums_equal_the_numpy_restatement_bit_for_bit(dim):
    X, labels, order, start, want = case(dim)
    got = device_sums(X, order, start, len(SIZES))
    assert same_bits(got, want)
    assert not got[0].any()                                      # the empty cluster


def test_sums_at_dim_8192():
    sizes = (0, 1, 255, 44)
    X, labels, order, start, want = case(8192, n=300, sizes=sizes)
    assert same_bits(device_sums(X, order, start, len(sizes)), want)


@pytest.mark.parametrize("block_threads", [64, 256, 1024])
@pytest.mark.parametrize("runs_per_block", [1, 3, 8])
def test_same_bits_under_every_launch_shape(block_threads, runs_per_block):
    for dim in (64, 192):
        X, labels, order, start, want = case(dim)
        assert same_bits(device_sums(X, order, start, len(SIZES), tuned=(block_threads, runs_per_block)), want), dim


@pytest.mark.parametrize("dim", [64, 192])
def test_sums_against_float64_within_the_two_level_bound(dim):
    """|S - S64| <= gamma_k sum|x| per (cluster, dim), k = 256 + ceil(m / 256), u = 2^-24: the standard bound of a sequential sum of
    256 terms followed by a sequential sum of ceil(m / 256) partials.  Derived, not tuned."""
    X, labels, order, start, _ = case(dim)
    got = device_sums(X, order, start, len(SIZES)).astype(np.float64)
    S64, A64 = R.cluster_sums(X, labels, len(SIZES))
    for c, m in enumerate(SIZES):
        err, bound = np.abs(got[c] - S64[c]), R.sum_bound(m) * A64[c]
        print(f"dim {dim} cluster {c} m {m}: max err {err.max():.3e}, min bound {bound.min():.3e}")
        assert (err <= bound).all(), c


def test_many_clusters_and_members_beyond_one_block_of_starts():
    """C = 1500 clusters (the scan of `start` takes several entries per thread) of 0 to 3 members each, and one of 5000."""
    rs = np.random.RandomState(9)
    C, dim = 1500, 64
    sizes = rs.randint(0, 4, C)
    sizes[700] = 5000
    n = int(sizes.sum())
    X = (rs.randn(n, dim) * 0.3).astype(np.float16)
    labels = rs.permutation(np.repeat(np.arange(C), sizes)).astype(np.int32)
    order, start, _ = T.members_host(labels, C)
    want = T.sums_host(X, order, start)
    assert same_bits(device_sums(X, order, start, C), want)
    assert same_bits(device_sums(X, order, start, C, tuned=(64, 5)), want)


def test_finish_against_float64_and_the_numpy_restatement():
    for dim in (64, 192, 8192):
        rs = np.random.RandomState(dim)
        S = (rs.randn(6, dim) * 20).astype(np.float32)
        S[2] = 0.0                                              # an all-zero sum keeps prev
        start = np.array([0, 10, 10, 20, 30, 40, 50])           # cluster 1 is empty and keeps prev
        prev = rs.randn(6, dim).astype(np.float32)
        c32, c16 = T.cluster_finish(torch.from_numpy(S).to(DEV), torch.from_numpy(start).to(DEV), torch.from_numpy(prev).to(DEV))
        assert torch.equal(c16.view(torch.int16), c32.half().view(torch.int16))
        got, got16 = c32.cpu().numpy(), c16.cpu().numpy()
        for c in (1, 2):
            assert same_bits(got[c], prev[c]), (dim, c)
        live = [0, 3, 4, 5]
        want = R.normalise(S[live])
        rel = np.abs(got[live] - want) / np.abs(want)
        print(f"dim {dim}: max relative error {rel.max():.3e}, bound {4 * dim * U:.3e}")
        assert (rel <= 4 * dim * U).all(), dim
        h32, h16 = T.finish_host(S, start, prev)
        assert same_bits(got, h32) and np.array_equal(got16.view(np.uint16), h16.view(np.uint16)), dim


def test_bad_order_entries_add_nothing():
    """`order` carrying -1 and n_rows: the sums of the remaining members, bit for bit (the bad entries keep their places in their
    runs; here every cluster is one run, so the remaining members form the same runs)."""
    rs = np.random.RandomState(4)
    n, dim = 400, 192
    X = (rs.randn(n, dim) * 0.3).astype(np.float16)
    good = [np.sort(rs.choice(n, 100, replace=False)).astype(np.int32), np.sort(rs.choice(n, 150, replace=False)).astype(np.int32)]
    bad = [np.insert(good[0], [0, 37, 100], [-1, n, -1]), np.insert(good[1], [5, 5, 150], [n, 2 ** 31 - 1, -(2 ** 31)])]
    want = T.sums_host(X, np.concatenate(good), np.array([0, 100, 250]))
    got = device_sums(X, np.concatenate(bad), np.array([0, 103, 256]), 2)
    assert same_bits(got, want)
    assert same_bits(T.sums_host(X, np.concatenate(bad), np.array([0, 103, 256])), want)


def test_a_start_that_decreases_gives_the_clamped_ranges():
    X, labels, order, start, want = case(64)
    s = start.copy()                                             # sizes 0 1 255 256 257 600 131 -> start 0 0 1 256 512 769 1369 1500
    s[4] = 100                                                   # decreases once: the running maximum makes it 256, so cluster 3 is empty
    s[7] = 99999                                                 # beyond n_members: clamped to 1500
    fixed = T.clamp_starts(s, len(order))
    assert fixed.tolist() == [0, 0, 1, 256, 256, 769, 1369, 1500]
    ref = T.sums_host(X, order, fixed)
    got = device_sums(X, order, s, len(SIZES))
    assert same_bits(got, ref) and same_bits(T.sums_host(X, order, s), ref)
    assert not got[3].any() and same_bits(got[[0, 1, 2, 5, 6]], want[[0, 1, 2, 5, 6]])
    neg = start.copy()
    neg[0] = -5                                                  # below 0: clamped to 0
    assert same_bits(device_sums(X, order, neg, len(SIZES)), want)


def test_no_members_gives_zero_sums():
    X = np.ones((10, 64), np.float16)
    got = device_sums(X, np.zeros(0, np.int32), np.zeros(4, np.int64), 3)
    assert not got.any()
