"""arx_graph_link and arx_graph_remap (csrc/graph.hip) against their numpy restatements `graph.link_host` and `graph.remap_host` on
the device (-m gpu; INTEGRATION.md "Keeping the graph").  Every comparison is exact and covers the whole neighbour array."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import graph as G
from arxiv_rag_amd.mutation import compact_rows_device, plan_device
from arxiv_rag_amd.where import pack_bitmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32_MAX = np.iinfo(np.int32).max
GUARD = 8                                                        # rows past n_rows, in the corpus and in the graph: never read as rows, never written
COUNTS = (0, 1, 63, 64, 65, 300)                                 # offers a target: around the 64-wide chunk, with the H old tail entries in front


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def unit_rows(n, dim, seed):
    X = np.random.RandomState(seed).randn(n, dim)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


def garbage_graph(rows, n, degree, seed):
    """a random graph with about 6 % of its entries bad: -1, n (a guard row), INT32_MAX, INT32_MIN, the row itself, a repeat"""
    rs = np.random.RandomState(seed)
    nb = rs.randint(0, n, (rows, degree)).astype(np.int32)
    kind = rs.randint(0, 100, (rows, degree))
    nb[kind == 0], nb[kind == 1], nb[kind == 2], nb[kind == 5] = -1, n, I32_MAX, np.iinfo(np.int32).min
    nb = np.where(kind == 3, np.arange(rows, dtype=np.int32)[:, None], nb)
    nb[:, 1:] = np.where(kind[:, 1:] == 4, nb[:, :1], nb[:, 1:])
    return nb


_worlds = {}


def world(n, dim):
    """X [n + GUARD, dim]: rows n // 2 and n // 2 + 1 copies of row 10, row 17 all NaN; computed once per shape"""
    if (n, dim) not in _worlds:
        X = unit_rows(n + GUARD, dim, n)
        X[n // 2] = X[n // 2 + 1] = X[10]
        X[17] = np.nan
        _worlds[(n, dim)] = (X, dev(X))
    return _worlds[(n, dim)]


def slots(n, seed):
    """(targets, offer_start, offers): ascending targets with every count of COUNTS (rows 10, 17 and n - 1 among them), and between
    them slots that must be skipped: a repeat, a descent, -1, n, INT32_MAX last.  A live slot's offers: random rows of [-3, n + 3),
    the target itself, row 10 and its two copies, the NaN row, and (from 63 offers on) every one of them twice."""
    rs = np.random.RandomState(seed)
    live = sorted(set(rs.choice(np.arange(20, n - 1), 2 * len(COUNTS) - 3, replace=False).tolist()) | {10, 17, n - 1})
    targets, lists = [], []
    for j, t in enumerate(live):
        c = COUNTS[j % len(COUNTS)]
        o = rs.randint(-3, n + 3, c).astype(np.int64)
        if c >= 63:
            o[:6] = [t, 10, n // 2, n // 2 + 1, 17, I32_MAX]
            o[c // 2:] = o[:c - c // 2]
        elif c == 1:
            o[0] = t if j % 2 else n // 2
        targets.append(t), lists.append(o.tolist())
        if j % 3 == 1:                                            # skipped slots, each with offers that would change a row
            for bad in (t, live[0], -1, n):
                targets.append(bad), lists.append(rs.randint(0, n, 5).tolist())
    targets.append(I32_MAX), lists.append([1, 2, 3])
    start = np.zeros(len(targets) + 1, np.int64)
    start[1:] = np.cumsum([len(o) for o in lists])
    return np.array(targets, np.int32), start.astype(np.int32), np.array([r for o in lists for r in o], np.int32)


def run(Xd, nb, t, start, offers, n, threads=None):
    nbd = dev(nb)
    G.graph_link(Xd, nbd, dev(t), dev(start), dev(offers), n_rows=n, threads=threads)
    return nbd.cpu().numpy()


@pytest.mark.parametrize("n,dim,degree", [(300, 64, 8), (300, 64, 32), (777, 128, 64), (777, 128, 32), (300, 768, 32)])
def test_link_equals_the_restatement_over_the_whole_array(n, dim, degree):
    X, Xd = world(n, dim)
    nb = garbage_graph(n + GUARD, n, degree, degree)
    t, start, offers = slots(n, degree + dim)
    with np.errstate(all="ignore"):
        want = G.link_host(X, nb, t, start, offers, n_rows=n)
    got = run(Xd, nb, t, start, offers, n)
    assert np.array_equal(got, want)
    H = degree // 2
    live = [int(v) for j, v in enumerate(t) if 0 <= v < n and v > max([-1] + [int(u) for u in t[:j] if u < n])]
    assert len(live) == 2 * len(COUNTS) and {10, 17, n - 1} <= set(live)
    others = np.ones(n + GUARD, bool)
    others[live] = False
    assert np.array_equal(got[others], nb[others]) and np.array_equal(got[:, :H], nb[:, :H])        # other rows, guard rows, every head
    assert sum(not np.array_equal(got[r], nb[r]) for r in live) >= len(live) - 2                    # the live slots did something
    for r in live:                                                # a tail: distinct valid rows outside the head, then -1
        tail = got[r, H:]
        v = tail[tail >= 0]
        assert np.all(tail[v.shape[0]:] == -1) and len(set(v.tolist())) == v.shape[0] and v.max(initial=0) < n
        assert r not in v and not set(v.tolist()) & set(nb[r, :H].tolist())
    for threads in (64, 128, 256):                                # every launch shape: the same bytes
        assert np.array_equal(run(Xd, nb, t, start, offers, n, threads=threads), want), threads


def test_bad_offer_ranges_skip_their_slot_and_nothing_else():
    n = 300
    X, Xd = world(n, 64)
    nb = garbage_graph(n + GUARD, n, 16, 3)
    offers = np.random.RandomState(5).randint(0, n, 40).astype(np.int32)
    t = np.array([20, 30, 40, 50, 60], np.int32)
    for start in ([0, 8, 4, 16, 24, 40], [-1, 8, 16, 24, 32, 40], [0, 8, 16, 24, 32, 41], [0, 8, 16, 24, 32, I32_MAX], [8, 0, 0, 0, 0, -5]):
        start = np.array(start, np.int32)
        want = G.link_host(X, nb, t, start, offers, n_rows=n)
        assert np.array_equal(run(Xd, nb, t, start, offers, n), want), start
        bad = [j for j in range(5) if start[j] < 0 or start[j + 1] < start[j] or start[j + 1] > 40]
        assert bad and all(np.array_equal(want[t[j]], nb[t[j]]) for j in bad), start
    none = run(Xd, nb, t[:0], np.zeros(1, np.int32), offers[:0], n)                # no slot: nothing is launched
    assert np.array_equal(none, nb)


def test_link_refusals_name_the_field_before_any_launch():
    from arxiv_rag_amd import _lib
    n = 300
    X, Xd = world(n, 64)
    nb = garbage_graph(n + GUARD, n, 16, 3)
    t, start, offers = dev(np.array([20], np.int32)), dev(np.array([0, 3], np.int32)), dev(np.array([1, 2, 3], np.int32))
    nbd = dev(nb)
    with pytest.raises(_lib.ArxError, match="threads=96"):
        G.graph_link(Xd, nbd, t, start, offers, n_rows=n, threads=96)
    lib = _lib.load()
    for kw, part in ((dict(degree=12), "degree=12"), (dict(degree=72), "degree=72"), (dict(dim=96), "dim=96"), (dict(n_rows=0), "n_rows=0"),
                     (dict(n_targets=-1), "n_targets=-1"), (dict(n_offers=-1), "n_offers=-1"), (dict(n_offers=1 << 31), "n_offers=")):
        a = {**dict(n_rows=n, dim=64, degree=16, n_targets=1, n_offers=3), **kw}
        rc = lib.arx_graph_link(Xd.data_ptr(), a["n_rows"], a["dim"], nbd.data_ptr(), a["degree"], t.data_ptr(), a["n_targets"], start.data_ptr(),
                                offers.data_ptr(), a["n_offers"], None)
        assert rc != 0 and part in lib.arx_last_error().decode(), (kw, lib.arx_last_error())
    assert lib.arx_graph_link(None, n, 64, nbd.data_ptr(), 16, t.data_ptr(), 1, start.data_ptr(), offers.data_ptr(), 3, None) != 0
    assert lib.arx_graph_remap(nbd.data_ptr(), 10, 12, t.data_ptr(), t.data_ptr(), 20, None) != 0 and "degree=12" in lib.arx_last_error().decode()
    assert lib.arx_graph_remap(nbd.data_ptr(), 30, 16, t.data_ptr(), t.data_ptr(), 20, None) != 0 and "count=30" in lib.arx_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(nbd.cpu().numpy(), nb)                  # nothing was launched


@pytest.mark.parametrize("n_old,degree", [(130, 8), (4096, 32)])
def test_remap_equals_the_restatement(n_old, degree):
    rs = np.random.RandomState(n_old)
    nb = garbage_graph(n_old, n_old, degree, 7)
    wild = rs.rand(n_old, degree) < 0.02
    nb[wild] = rs.randint(-1 << 31, (1 << 31) - 1, int(wild.sum())).astype(np.int32)      # any bit pattern is legal
    nbd = dev(nb)

    def without(frac):
        keep = np.ones(n_old, bool)
        keep[rs.choice(n_old, int(np.ceil(n_old * frac)), replace=False)] = False
        return keep
    masks = [without(0.0), without(0.01), without(0.5), np.arange(n_old) == n_old - 3]    # 0 %, 1 %, 50 % and all but one row deleted
    for keep in masks:
        words = dev(pack_bitmap(keep).view(np.int64))
        word_rank, count = plan_device(words, n_old)
        assert count == int(keep.sum())
        moved = torch.full((n_old + GUARD, degree), 7, dtype=torch.int32, device=DEV)
        compact_rows_device(nbd, moved, n_old, words, word_rank)
        G.graph_remap(moved, count, words, word_rank, n_old)
        got = moved.cpu().numpy()
        want = G.remap_host(nb[keep], keep)
        assert np.array_equal(got[:count], want), int(keep.sum())
        assert got[:count].max() < count and got[:count].min() >= -1 and np.all(got[count:] == 7)   # rows past count are not written
    G.graph_remap(moved, 0, words, word_rank, n_old)              # no row: nothing is launched
