"""The cases of tests/test_gpu_graph_large.py (built in tests/graph_cases.py) land on the branches they are meant for: proved here with
the numpy restatements alone (no GPU; INTEGRATION.md "Graph search").  If the visited table's hash in csrc/graph.hip changes, or a
builder is altered so that a case leaves its branch (the table below capacity, no wrapped probe, a cut beside the plateau, a beam that
never turns over), a test of this module fails instead of the GPU case going soft."""
import numpy as np
import pytest

from arxiv_rag_amd import graph as G
from tests import graph_cases as C

SLOTS, MULT, SHIFT = C.table_constants()


def trace(c, q, ef=None):
    return C.walk_trace(c.X, c.nb, c.Q[q], c.ent[q], c.ef if ef is None else ef, c.iters, c.n_rows)


def test_the_table_constants_and_the_colliding_rows_are_what_the_cases_assume():
    assert (SLOTS, MULT, SHIFT) == (16384, 0x9E3779B1, 18) and SLOTS == 1 << (32 - SHIFT) and G.MAX_VISITED == SLOTS // 2
    last64, last128, last1 = (C.home_slot_rows(C.N_BIG, lo, MULT, SHIFT) for lo in (SLOTS - 64, SLOTS - 128, SLOTS - 1))
    assert np.array_equal(last64, C.home_slot_rows(C.N_BIG, SLOTS - 64))                      # the builder's defaults are the kernel's
    assert (len(last64), int(last64[0]), int(last64[-1]), len(last128), len(last1)) == (4097, 144, 1048753, 8193, 63)
    assert C.table_model(last64, SLOTS, MULT, SHIFT) == (4090, 4033, 4097)                    # one chain, wrapped into the slots 0 .. 4032
    assert C.table_model([5, 5, 7, 5], SLOTS, MULT, SHIFT) == (0, 0, 2)                      # a row offered again is found, not inserted
    assert C.table_model([14, 15, 12, 13], 8, 1, 1) == (3, 2, 4)                             # 8 slots, home = row / 2: 15 wraps to slot 0, 13 to slot 1


def test_fresh_tree_gives_every_node_one_parent_and_relabel_moves_it():
    tree, roots = C.fresh_tree(8, 8, 8192)
    kids = tree[tree >= 0]
    assert roots.tolist() == list(range(8)) and np.array_equal(np.sort(kids), np.arange(8, 8192)) and int((tree[1023:] >= 0).sum()) == 0
    rows = np.array([40, 7, 19, 3, 90], np.int64)
    moved = C.relabel(np.array([[1, 2], [3, -1], [4, 0], [-1, -1], [-1, -1]], np.int32), rows, 100)
    assert moved[40].tolist() == [7, 19] and moved[7].tolist() == [3, -1] and moved[19].tolist() == [90, 40] and int((moved >= 0).sum()) == 5
    order = C.walk_order(8, 8, 1023)
    assert np.array_equal(np.sort(order), np.arange(8192)) and np.array_equal(order[1023:], np.arange(1023, 8192))


@pytest.mark.parametrize("degree,n_entries,iters", C.CAPACITY_SHAPES)
def test_capacity_shapes_fill_the_table_to_its_limit(degree, n_entries, iters):
    c = C.capacity_case(degree)
    assert n_entries + iters * degree == G.MAX_VISITED == 8192 and c.iters == iters and c.ent.shape == (3, n_entries)
    for want in (c.want, c.want_allow):
        assert want[2].tolist() == [8192] * 3 and want[3].tolist() == [iters] * 3
    assert (c.want_allow[1] >= 0).all() and c.mask[c.want_allow[1]].all() and not np.array_equal(c.want[1], c.want_allow[1])
    G.check_search_args(c.k, c.ef, iters, degree, n_entries)
    with pytest.raises(ValueError, match="visited table|max_iters"):
        G.check_search_args(c.k, c.ef, iters + 1, degree, n_entries)
    for q in range(3):                                           # every query walks rows of its own
        assert set(c.want[1][q].tolist()) <= set(range(8192 * q, 8192 * (q + 1)))


def test_collision_shapes_build_one_long_chain_that_wraps():
    c = C.collision_case("chain")
    c.nb = C.collision_graph(c)
    t = trace(c, 0)
    assert c.want[2].tolist() == [4096, 4096] and c.want[3].tolist() == [63, 63] and len(t.visited) == 4096 and len(t.expanded) == 63
    assert (C.home_slots(t.visited, MULT, SHIFT) >= SLOTS - 64).all()
    longest, wrapped, held = C.table_model(t.visited, SLOTS, MULT, SHIFT)
    assert longest >= 4000 and wrapped >= 4000 and held == 4096
    assert np.array_equal(c.want[1][0], c.want[1][1]) and np.array_equal(c.want[0][1], 2 * c.want[0][0])      # the doubled query: the same walk
    del c.nb
    c = C.collision_case("half")
    c.nb = C.collision_graph(c)
    t = trace(c, 0)
    assert c.want[2].tolist() == [8192, 8192] and c.want[3].tolist() == [127, 127] and len(t.visited) == 8192
    longest, wrapped, held = C.table_model(t.visited, SLOTS, MULT, SHIFT)
    assert held == 8192 == G.MAX_VISITED and wrapped > 8000 and longest > 8000
    del c.nb
    c = C.collision_case("last")
    c.nb = C.collision_graph(c)
    t = trace(c, 1)
    assert c.want[2].tolist() == [63] * 3 and c.want[3].tolist() == [63] * 3 and sorted(t.visited) == c.rows.tolist()
    assert (C.home_slots(c.rows, MULT, SHIFT) == SLOTS - 1).all() and C.table_model(t.visited, SLOTS, MULT, SHIFT) == (62, 62, 63)
    del c.nb


def test_high_rows_are_reached_and_answer_their_queries():
    c = C.high_rows_case()
    assert c.want[1][:, 0].tolist() == C.HIGH_ROWS.tolist() and (C.HIGH_ROWS >= (1 << 20) - 1).all() and C.HIGH_ROWS[-1] == C.N_BIG - 1
    only_high, none, every = c.want_masks
    assert (only_high[1][:, :3] >= 1 << 20).all() and (only_high[1][:, 3:] == -1).all()       # three of the four planted rows pass
    assert (none[1] == -1).all() and np.isneginf(none[0]).all()
    assert all(np.array_equal(a, b) for a, b in zip(every, c.want))


@pytest.mark.parametrize("ef,degree,n_entries,iters", C.EF_SHAPES)
def test_beam_widths_walk_long_and_take_parents_from_the_last_chunk(ef, degree, n_entries, iters):
    c = C.ef_case(ef)
    assert ef % 64 in (1, 63) and iters <= G.max_iters_for(degree, n_entries) and (ef != 511 or iters == G.max_iters_for(8, 8) == 1023)
    assert (c.want[3] > ef // 2).all() and (c.want[2] > ef).all()
    last_chunk = 0
    for q in range(3):
        t = trace(c, q)
        assert len(t.visited) == c.want[2][q] and len(t.expanded) == c.want[3][q] and t.beam[:32] == c.want[1][q].tolist()
        last_chunk += sum(p >= ef // 64 * 64 for p in t.parent_pos)
    assert last_chunk > 0                                        # a parent the ballot finds only in the beam's last, partial chunk of 64 marks
    assert (c.want_allow[1] >= 0).all() and c.mask[c.want_allow[1]].all()


@pytest.mark.parametrize("ef", [64, 512])
def test_the_beam_turns_over(ef):
    c = C.turnover_case(ef)
    assert c.degree == 8 and c.iters == 1023 >= 600
    assert (c.want[3] > ef).any()
    gone = 0
    for q in range(3):
        t = trace(c, q)
        assert len(t.expanded) == c.want[3][q] and len(t.visited) == c.want[2][q]
        gone += len(set(t.expanded) - set(t.beam))
    assert gone > 0                                              # expanded rows, pushed past the cut by better ones


def test_the_cuts_fall_inside_the_plateau():
    c = C.plateau_case()
    X, rows = c.X, set(C.PLATEAU_ROWS.tolist())
    assert all(np.array_equal(X[r], X[5]) for r in rows) and len(rows) == 200 and min(rows) == 5 and max(rows) == (1 << 20) + 100
    t = trace(c, 0)
    seen = sorted(r for r in t.visited if r in rows)
    word = t.words[5] if 5 in t.words else t.words[seen[0]]
    assert all(t.words[r] == word for r in seen) and max(t.words.values()) == word            # one score word, and the best there is
    assert len(seen) > c.ef and t.beam == seen[:c.ef]                                         # the cut at ef: inside the run, the lowest rows stay
    assert c.want[1][0].tolist() == seen[:32] and len(set(G.order_words(c.want[0][0]).tolist())) == 1
    ok = [r for r in seen if c.mask[r]]
    assert len(ok) > 10 and c.want_allow[1][0].tolist() == ok[:10] and len(ok) < len(seen)    # the cut at k under allow
    assert max(seen) >= 1 << 20 or max(rows - set(seen)) >= 1 << 20                           # (the plateau reaches past 2^20 either way)


@pytest.mark.parametrize("degree", [24, 40, 56])
def test_odd_degrees_walk(degree):
    c = C.degree_case(degree)
    assert c.nb.shape[1] == degree and (c.want[3] > 64).all() and (c.want[2] > 64 * degree // 2).all()


@pytest.mark.parametrize("dim", C.DIMS)
def test_dims_walk(dim):
    c = C.dim_case(dim)
    assert c.X.shape[1] == dim and dim // 64 in (3, 7, 17, 64) and (c.want[3] == c.iters).all() and (c.want[2] > c.ef).all()
    assert c.want[1][0, :3].tolist() == [10, 1000, 1001]         # query 0 is row 10, and so are its two copies


def test_link_plan_has_the_slots_the_docstring_names():
    p = C.link_plan()
    t = p.targets.astype(np.int64)
    n = C.N_BIG
    valid = np.where(t < n, t, -1)
    before = np.concatenate([[-1], np.maximum.accumulate(valid)[:-1]])
    live = (t >= 0) & (t < n) & (t > before)
    assert len(t) >= 3000 and np.array_equal(t[live], p.live) and int(live.sum()) == 3 + (n - C.LINK_SHADOW - 1) - len(p.left_out) == 602
    assert t[2] == C.LINK_SHADOW and C.LINK_SHADOW > n - 1500
    shadowed = (t >= 0) & (t < C.LINK_SHADOW) & (np.arange(len(t)) > 2)
    assert int(shadowed.sum()) == p.n_shadowed + 3 * 2 and not live[shadowed].any()           # the run of 2500, and a repeat and a descent three times
    assert np.all(np.diff(t[3:][(shadowed & ~np.isin(np.arange(len(t)), p.kinds))[3:]]) > 0)  # ascending over the whole range, yet skipped
    for lo in (256, 512, 1024, 2048, 2560, 3072):                # the skipped kinds past every stride of the scan over the earlier targets
        five = [s for s in p.kinds if lo < s][:5]
        assert len(five) == 5 and five[-1] - five[0] == 4 and not live[five].any()
        assert t[five[0]] == t[five[0] - 1] and 0 <= t[five[1]] < t[five[0]] <= before[five[1]] and t[five[2:]].tolist() == [-1, n, C.I32_MAX]
        assert t[five[1]] not in set(t[live].tolist())           # a descent names a row that is no live target
    counts = np.diff(p.start)
    assert p.most_offers == 5000 == counts.max() and len(p.offers) == p.start[-1]
    hub = p.offers[p.start[np.nonzero(t == C.LINK_HUB)[0][0]]:][:5000]
    assert np.array_equal(hub[:2500], hub[2500:]) and len(set(hub.tolist())) == 2500
    s = int(np.nonzero(t == C.LINK_HIGH_ONLY)[0][0])
    assert live[s] and (p.offers[p.start[s]:p.start[s + 1]] >= 1 << 20).all() and counts[s] == 90


def test_link_plateau_straddles_the_tail_cut():
    p, X = C.link_plan(), C.big_corpus()
    t = C.LINK_PLATEAU
    s = int(np.nonzero(p.targets == t)[0][0])
    offers = p.offers[p.start[s]:p.start[s + 1]]
    run = sorted(set(offers.tolist()) & set(C.PLATEAU_ROWS.tolist()) - {t})
    assert len(run) == 100 and t in offers and np.array_equal(X[t], X[5])
    for degree in (32, 64):
        H = degree // 2
        nb = np.full((C.N_BIG, degree), -1, np.int32)
        nb[t, :H] = np.arange(100000, 100000 + H)
        got = G.link_host(X, nb, p.targets[s:s + 1], np.array([0, len(offers)]), offers, n_rows=C.N_BIG)
        assert got[t, H:].tolist() == run[:H] and H < len(run)   # a run of one score across the cut: the lowest rows stay


def test_remap_masks_leave_the_counts_and_the_holes_they_name():
    masks = C.remap_masks()
    assert [int(m.sum()) % 4 for _, m in masks[:3]] == [1, 2, 3] and int(masks[3][1].sum()) == 1 and masks[3][1][(1 << 20) + 1]
    for _, m in masks[:3]:
        assert m.shape == (C.N_BIG,) and not m[[63, 64, (1 << 20) - 1, 1 << 20]].any() and m[[62, (1 << 20) - 2, (1 << 20) + 1, C.N_BIG - 1]].all()
        assert all(not m[64 * w:64 * (w + 1)].any() for w in (1, 2, 77, C.N_BIG // 64 - 1))
        assert int(m.sum()) > (1 << 20) - 40000
    assert C.N_BIG % 64 != 0 and len(C.remap_sample(1 << 20, 0)) == 3 * 4096 and C.remap_sample(1, 0).tolist() == [0]
