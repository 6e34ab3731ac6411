"""arx_graph_search, arx_graph_link, arx_graph_remap (csrc/graph.hip) and `graph.assemble_device` where the first graph suites stop
(-m gpu; INTEGRATION.md "Graph search" / "Keeping the graph"): the visited table at its capacity of 8192 rows and under probe chains
of thousands of slots that wrap past the last slot, rows around and past 2^20, beam widths next to a multiple of 64, walks of up to
1023 iterations that turn the beam over, plateaus of identical rows across every cut, degrees 24 / 40 / 56, dims 192 .. 8192, a link
call of 3000 slots with an early large target, a remap over 2^20 + 197 rows and an assembly in slices.

Every comparison is bit for bit against the numpy restatements (`search_host`, `link_host`, `remap_host`, `assemble_host`); there is
no tolerance.  The cases are built in tests/graph_cases.py, and tests/test_graph_cases_host.py proves without a GPU that each lands on
the branch it is meant for."""
import functools

import numpy as np
import pytest
import torch

from arxiv_rag_amd import graph as G
from arxiv_rag_amd.mutation import compact_rows_device, plan_device
from arxiv_rag_amd.where import pack_bitmap
from tests import graph_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = 1 << 33


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def words(mask):
    return dev(pack_bitmap(mask).view(np.int64))


@functools.lru_cache(maxsize=None)
def big_dev():
    """the big corpus on the device: uploaded once a module"""
    return dev(np.array(C.big_corpus()))                          # (a writable copy: the shared one is read-only)


def same(got, want, k=None, idx_base=0):
    s, i, scored, expanded = (t.cpu().numpy() for t in got)
    ws, wi = (want[0], want[1]) if k is None else (want[0][:, :k], want[1][:, :k])
    assert np.array_equal(i, np.where(wi >= 0, wi + idx_base, wi))
    assert np.array_equal(bits(s), bits(ws))
    assert np.array_equal(scored, want[2]) and np.array_equal(expanded, want[3])


def search(c, Xd, nbd, entd, Qd, allow=None, k=None, ef=None, **kw):
    return G.graph_search(Xd, nbd, Qd, entd, c.k if k is None else k, c.ef if ef is None else ef, c.iters, allow=allow, n_rows=c.n_rows, **kw)


def every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, allow, base):
    for threads in (64, 128, 256):
        got = search(c, Xd, nbd, entd, Qd, allow=allow, threads=threads)
        assert all(torch.equal(x, y) for x, y in zip(got, base)), threads
    alone = [search(c, Xd, nbd, entd[q:q + 1].contiguous(), Qd[q:q + 1].contiguous(), allow=allow) for q in range(Qd.shape[0])]
    for j in range(4):
        assert torch.equal(torch.cat([r[j] for r in alone]), base[j]), j


# ---- 1, 2: the visited table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [d for d, _, _ in C.CAPACITY_SHAPES])
def test_table_at_capacity(degree):
    c = C.capacity_case(degree)
    Xd, nbd, entd, Qd = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q)
    for allow, want in ((None, c.want), (words(c.mask), c.want_allow)):
        base = search(c, Xd, nbd, entd, Qd, allow=allow)
        same(base, want)
        assert base[2].tolist() == [8192] * 3 and base[3].tolist() == [c.iters] * 3          # every row inserted once: none lost, none twice
        every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, allow, base)


@pytest.mark.parametrize("which", ["chain", "half", "last"])
def test_table_under_collision(which):
    c = C.collision_case(which)
    Xd, nbd, entd, Qd = big_dev(), dev(C.collision_graph(c)), dev(c.ent), dev(c.Q)
    base = search(c, Xd, nbd, entd, Qd)
    same(base, c.want)
    assert base[2].tolist() == [len(c.rows)] * len(c.Q)
    for threads in (64, 128, 256):
        assert all(torch.equal(x, y) for x, y in zip(search(c, Xd, nbd, entd, Qd, threads=threads), base)), threads


# ---- 3: rows around 2^20 --------------------------------------------------------------------------------------------------------------
def test_rows_around_two_to_the_twenty():
    c = C.high_rows_case()
    Xd, nbd, entd, Qd = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q)
    got = search(c, Xd, nbd, entd, Qd, idx_base=BASE)
    same(got, c.want, idx_base=BASE)
    assert (got[1][:, 0] - BASE).tolist() == C.HIGH_ROWS.tolist()
    for mask, want in zip(c.masks, c.want_masks):
        same(search(c, Xd, nbd, entd, Qd, allow=words(mask), idx_base=BASE), want, idx_base=BASE)
    none = search(c, Xd, nbd, entd, Qd, allow=words(c.masks[1]), idx_base=BASE)
    assert bool((none[1] == -1).all()) and bool(torch.isneginf(none[0]).all())


# ---- 4: beam widths and long walks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ef", [s[0] for s in C.EF_SHAPES])
def test_beam_widths_beside_a_multiple_of_64(ef):
    c = C.ef_case(ef)
    Xd, nbd, entd, Qd, allow = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q), words(c.mask)
    for k in (1, 31, 32):
        same(search(c, Xd, nbd, entd, Qd, k=k), c.want, k=k)
        same(search(c, Xd, nbd, entd, Qd, k=k, allow=allow), c.want_allow, k=k)
    every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, None, search(c, Xd, nbd, entd, Qd))


@pytest.mark.parametrize("ef", [64, 512])
def test_beam_turnover_over_a_thousand_iterations(ef):
    c = C.turnover_case(ef)
    Xd, nbd, entd, Qd = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q)
    base = search(c, Xd, nbd, entd, Qd)
    same(base, c.want)
    same(search(c, Xd, nbd, entd, Qd, allow=words(c.mask)), c.want_allow)
    every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, None, base)


# ---- 5: plateaus ----------------------------------------------------------------------------------------------------------------------
def test_plateaus_across_the_cuts_keep_the_lowest_rows():
    c = C.plateau_case()
    Xd, nbd, entd, Qd = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q)
    base = search(c, Xd, nbd, entd, Qd)
    same(base, c.want)
    same(search(c, Xd, nbd, entd, Qd, allow=words(c.mask), k=10), c.want_allow)
    every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, None, base)


# ---- 6: degrees and dims --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [24, 40, 56])
def test_degrees_between_the_powers_of_two(degree):
    c = C.degree_case(degree)
    Xd, nbd, entd, Qd = big_dev(), dev(c.nb), dev(c.ent), dev(c.Q)
    base = search(c, Xd, nbd, entd, Qd)
    same(base, c.want)
    same(search(c, Xd, nbd, entd, Qd, allow=words(c.mask)), c.want_allow)
    every_launch_shape_and_alone(c, Xd, nbd, entd, Qd, None, base)


@pytest.mark.parametrize("dim", C.DIMS)
def test_search_dims(dim):
    c = C.dim_case(dim)
    Xd, nbd, entd, Qd = dev(c.X), dev(c.nb), dev(c.ent), dev(c.Q)
    base = search(c, Xd, nbd, entd, Qd)
    same(base, c.want)
    for threads in (64, 128, 256):
        assert all(torch.equal(x, y) for x, y in zip(search(c, Xd, nbd, entd, Qd, threads=threads), base)), threads


def link(Xd, nbd, t, start, offers, n, threads=None):
    out = nbd.clone()
    G.graph_link(Xd, out, t, start, offers, n_rows=n, threads=threads)
    return out


@pytest.mark.parametrize("dim", C.DIMS + (8192,))
def test_link_dims(dim):
    c = C.link_dim_case(dim)
    Xd, nbd, t, start, offers = dev(c.X), dev(c.nb), dev(c.targets), dev(c.start), dev(c.offers)
    got = link(Xd, nbd, t, start, offers, c.n_rows).cpu().numpy()
    assert np.array_equal(got, c.want)
    others = np.ones(c.nb.shape[0], bool)
    others[c.live] = False
    assert np.array_equal(got[others], c.nb[others]) and np.array_equal(got[:, :8], c.nb[:, :8])
    assert sum(not np.array_equal(got[r], c.nb[r]) for r in c.live) >= len(c.live) - 4             # the live slots did something
    for threads in (64, 128, 256):
        assert np.array_equal(link(Xd, nbd, t, start, offers, c.n_rows, threads=threads).cpu().numpy(), c.want), threads


# ---- 7: link at scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [32, 64])
def test_link_over_three_thousand_slots(degree):
    p, nb = C.link_plan(), C.link_graph(degree)
    want = C.link_want(degree, nb)
    H = degree // 2
    Xd, nbd, t, start, offers = big_dev(), dev(nb), dev(p.targets), dev(p.start), dev(p.offers)
    got = link(Xd, nbd, t, start, offers, C.N_BIG)
    wantd = dev(want)
    assert torch.equal(got, wantd)                               # the whole neighbour array, guard rows included
    others = np.ones(nb.shape[0], bool)
    others[p.live] = False
    assert np.array_equal(want[others], nb[others]) and np.array_equal(want[:, :H], nb[:, :H])     # every non-live row and every head: the input's bytes
    assert sum(not np.array_equal(want[r], nb[r]) for r in p.live) >= len(p.live) - len(p.live) // 7 - 8       # (a slot with no offer may change nothing)
    for threads in (64, 128, 256):
        assert torch.equal(link(Xd, nbd, t, start, offers, C.N_BIG, threads=threads), wantd), threads


# ---- 8: remap at scale ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [64, 24, 8])
def test_remap_over_two_to_the_twenty_rows(degree):
    """Compared with `remap_host` on a sample (the host loop over a million rows is too slow): the first 4096 moved rows, the last
    4096 and a random 4096 between them; the range of every entry and the rows past `count` are checked over the whole array."""
    n_old = C.N_BIG
    nb = C.remap_graph(degree)
    nbd = dev(nb)
    moved = torch.empty((n_old + 8, degree), dtype=torch.int32, device=DEV)
    for j, (name, keep) in enumerate(C.remap_masks()):
        kw = words(keep)
        word_rank, count = plan_device(kw, n_old)
        assert count == int(keep.sum()), name
        moved.fill_(7)
        compact_rows_device(nbd, moved, n_old, kw, word_rank)
        G.graph_remap(moved, count, kw, word_rank, n_old)
        sample = C.remap_sample(count, j)
        want = G.remap_host(nb[np.nonzero(keep)[0][sample]], keep)
        got = moved[dev(sample)].cpu().numpy()
        assert np.array_equal(got, want), name
        assert int(moved[:count].max()) < count and int(moved[:count].min()) >= -1 and bool((moved[count:] == 7).all()), name
        assert (want[:, -1] == -1).any() and (count == 1 or (want[:, -1] >= 0).any()), name        # rows with a dropped entry, rows with none


# ---- 9: assembly in slices ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spoiled_lists():
    from arxiv_rag_amd.index import ShardIndex
    knn = G.knn_lists(ShardIndex(dev(C.clustered_rows()), prefilter=None))
    return C.spoil_lists(knn.cpu().numpy())


@pytest.mark.parametrize("degree", [16, 32])
def test_assembly_in_slices(degree, monkeypatch):
    knn = spoiled_lists()
    monkeypatch.setattr(G, "ASSEMBLE_ROWS", 1000)                 # 66 slices, the last of 539 rows
    got = G.assemble_device(dev(knn), degree).cpu().numpy()
    monkeypatch.undo()
    assert knn.shape == (C.N_ASSEMBLE, G.KNN - 1) and C.N_ASSEMBLE > 65 * 1000
    assert np.array_equal(got, G.assemble_host(knn, degree))
    assert np.array_equal(G.assemble_device(dev(knn), degree).cpu().numpy(), got)                  # one slice: the same graph
