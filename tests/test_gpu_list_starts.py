"""`start` as the kernels read it (csrc/list_starts.h: every value clamped into [0, n_members], then a running maximum over lanes, waves
and the stretch of entries a thread owns), on the device (-m gpu), through both of its users: `ivf.ivf_search` (ivf_prepare_kernel,
1024 threads) against `ivf.search_host`, and `topics.cluster_sums` (cluster_partials_kernel, 256 threads and 1024) against
`topics.sums_host`.  Every comparison is exact, on ids, counts and f32 bits.  The list counts put an edge of a lane, a wave, a thread's
stretch and the block at 63 / 64, 1023 / 1024 and beyond (4096 lists: five entries a thread at 1024 threads, seventeen at 256); the
`start` arrays are built so that a maximum has to travel across all of them."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import ivf as I
from arxiv_rag_amd import topics as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, DIM, NQ, NPROBE, K = 1000, 64, 4, 4, 10
SPAN = 700                                                      # the even split hands out order[:SPAN]; the rest is reached through a peak alone
LISTS = (63, 64, 65, 1023, 1024, 1025, 4096)
PEAKS = (63, 64, 1023, 1024)                                    # the last entry of a wave and of the block at one entry per thread, and the next


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def case_names(n_lists):
    return ["honest", "early_peak"] + [f"peak_at_{p}" for p in PEAKS if p <= n_lists] + ["wild"]


def even(n_lists):
    return (np.arange(n_lists + 1, dtype=np.int64) * SPAN) // n_lists


def pad(lists, n_lists):
    """Four probes: the first four of `lists`, filled up with n_lists (outside [0, n_lists): such a probe is ignored)."""
    return ([int(c) for c in lists] + [n_lists] * NPROBE)[:NPROBE]


def build(n_lists, name, order):
    """(order, start, probes) of one case; `order`: the shared permutation of the rows (the honest split sorts its own)."""
    last = n_lists - 1
    if name == "honest":                                        # (a) `members_host` of random labels that leave four lists empty
        empty = [1, n_lists // 2, last - 1, last]
        labels = np.random.RandomState(n_lists).randint(0, n_lists, N)
        labels[np.isin(labels, empty)] = 0
        order, start, sizes = T.members_host(labels.astype(np.int32), n_lists)
        full = np.nonzero(sizes)[0]
        mid = len(full) // 2
        return order, start, [pad(full[:4], n_lists), pad(full[mid - 2:mid + 2], n_lists), pad(full[-4:], n_lists), empty]
    if name == "early_peak":                                    # (b) the largest value at index 1, then zeros: list 0 alone has rows
        start = np.zeros(n_lists + 1, np.int64)
        start[1] = SPAN
        far = [min(c, last) for c in (63, 64, 1023, 1024)]      # list 0 beside far lists: a maximum that got lost shortens the total
        return order, start, [[0, 1, 2, 3], [0, far[0], far[1], last], [0, far[2], far[3], n_lists // 2], [1, 2, n_lists // 2, last]]
    start = even(n_lists)
    if name == "wild":                                          # (d) negative and beyond n_members, also beyond 32 bits
        half, big = n_lists // 2, n_lists - n_lists // 4
        start[0], start[2], start[half], start[big] = -(2 ** 40), -7, -1, 2 ** 40
        return order, start, [[0, 1, 2, 3], [half - 1, half, half + 1, half + 2], [big - 1, big, 0, last], [big, big + 1, last - 1, last]]
    p = int(name.rsplit("_", 1)[1])                             # (c) a peak at entry p and a dip right after it
    base = start.copy()
    start[p] = base[p] + 250
    if p < n_lists:
        start[p + 1] = base[p] // 2
    s = T.clamp_starts(start, N)
    rows_before = [c for c in range(p - 1) if base[c + 1] > base[c]]
    shadowed = [c for c in range(p, n_lists) if base[c + 1] > base[c] and s[c + 1] == s[c]]      # rows in the even split, none behind the peak
    rows_after = [c for c in range(p, n_lists) if s[c + 1] > s[c]]
    return order, start, [pad([c for c in (p - 1, p, p + 1, p + 2) if c < n_lists], n_lists), pad(shadowed[:4], n_lists),
                          pad([rows_before[len(rows_before) // 2], p - 1] + rows_after[:1] + rows_after[-1:], n_lists),
                          pad(shadowed[-4:], n_lists)]


_WORLD, _CASES = {}, {}


def world():
    if not _WORLD:
        rs = np.random.RandomState(7)
        X = (rs.randn(N, DIM) / 8).astype(np.float16)
        Q = (rs.randn(NQ, DIM) / 8).astype(np.float16)
        _WORLD.update(X=X, Q=Q, order=rs.permutation(N).astype(np.int32))
    return _WORLD


def case(n_lists, name):
    """One case with its host answers, computed once and shared by the two tests; some query sees rows and some query sees none."""
    if (n_lists, name) not in _CASES:
        w = world()
        order, start, probes = build(n_lists, name, w["order"])
        probes = np.asarray(probes, np.int32)
        assert sorted(order.tolist()) == list(range(N)) and start.shape == (n_lists + 1,) and probes.shape == (NQ, NPROBE)
        found = I.search_host(w["X"], order, start, probes, w["Q"], K)
        assert (found[2] > 0).any() and (found[2] == 0).any(), (n_lists, name, found[2])
        _CASES[(n_lists, name)] = dict(order=order, start=start, probes=probes, found=found, sums=T.sums_host(w["X"], order, start),
                                       longest=int(np.diff(T.clamp_starts(start, N)).max()))
    return _CASES[(n_lists, name)]


PARAMS = [(n_lists, name) for n_lists in LISTS for name in case_names(n_lists)]


@pytest.mark.parametrize("n_lists,name", PARAMS)
def test_the_probe_search_reads_start_as_the_host_does(n_lists, name):
    w, c = world(), case(n_lists, name)
    got = I.ivf_search(dev(w["X"], np.float16), dev(c["order"], np.int32), dev(c["start"], np.int64), c["longest"], dev(w["Q"], np.float16),
                       dev(c["probes"], np.int32), K)
    s, i, n = (t.cpu().numpy() for t in got)
    want = c["found"]
    assert np.array_equal(bits(s), bits(want[0])) and np.array_equal(i, want[1]) and np.array_equal(n, want[2])


@pytest.mark.parametrize("n_lists,name", PARAMS)
def test_the_cluster_sums_read_start_as_the_host_does(n_lists, name):
    w, c = world(), case(n_lists, name)
    X, order, start = dev(w["X"], np.float16), dev(c["order"], np.int32), dev(c["start"], np.int64)
    for tuned in (None, (1024, 0)):                             # the default launch shape (256 threads) and 1024 threads
        got = T.cluster_sums(X, order, start, n_lists, tuned=tuned).cpu().numpy()
        assert np.array_equal(bits(got), bits(c["sums"])), tuned


def test_the_peaks_shadow_lists_the_probes_ask_for():
    """The cases are not vacuous: behind every peak at least one probed list has rows in the even split and none as the kernels read
    `start`, except where the peak is the last entry; and the wild values reach beyond 32 bits."""
    for n_lists in LISTS:
        for p in PEAKS:
            if p < n_lists - 1:
                c = case(n_lists, f"peak_at_{p}")
                s, base = T.clamp_starts(c["start"], N), even(n_lists)
                shadowed = [int(l) for l in c["probes"][1] if l < n_lists and base[l + 1] > base[l] and s[l + 1] == s[l]]
                assert shadowed and c["found"][2][1] == 0 and c["found"][2][0] >= 250
        assert np.abs(case(n_lists, "wild")["start"]).max() == 2 ** 40
