"""CPU companion of tests/test_gpu_search_large.py: the shapes that suite relies on (tests/search_cases.py `regime`, the restated dispatch of
csrc/search.hip) and the planter's promise that every sixteenth of a shard decides some planted query's answer."""
import numpy as np

from tests.search_cases import (GRADES, LINE, N_GRADED, N_SPANS, PLANT_K, batch_indices, last_list_first_row, near_copies, plant_rows,
                                plant_values, regime, span_of, tie_rows, GRADED0, TIED_Q)

# name -> (n, dim, n_groups, n_super, nsplit, per): the table of the large-shard suite (None: the shard's own searches select in-block)
TABLE = {
    "A": (625000, 768, 9766, 611, None, None),
    "B1": (1047581, 128, 16369, 1024, None, None),
    "B2": (1048576, 128, 16384, 1024, None, None),
    "B3": (1048577, 128, 16385, 1025, 129, 2),
    "C1": (2088989, 128, 32641, 2041, 256, 2),
    "C2": (2097181, 128, 32769, 2049, 256, 3),
    "D": (2162717, 1024, 33793, 2113, 256, 3),
}
DIM_SHARDS = {d: [v[0] for v in TABLE.values() if v[1] == d] for d in (768, 128, 1024)}


def test_regime_returns_the_figures_of_the_table():
    for name, (n, d, groups, sup, nsplit, per) in TABLE.items():
        for int8 in (False, True):
            r = regime(n, 40, 10, int8)
            assert (r.n_groups, r.n_super) == (groups, sup), name
            if nsplit is None:
                assert r.tail == ("i8-inblock" if int8 else "f16-inblock") and r.sel == 0, name
                assert regime(n, 40, 10, int8, no_single=True).sel == 1, name
            else:
                assert (r.nsplit, r.per) == (nsplit, per), name
                assert r.tail == ("i8-collect" if int8 else "select-rescore-NT1024") and r.sel == 1, name
    assert 625000 - 9765 * 64 == 40 and 1047581 - 16368 * 64 == 29 and 16369 - 1023 * 16 == 1      # the ragged groups; thread 1023's one group
    assert (regime(TABLE["B3"][0], 1, 10, False).slices, regime(TABLE["B3"][0], 1, 10, False).lists) == (513, 129)
    assert (regime(TABLE["C1"][0], 1, 10, False).slices, regime(TABLE["C1"][0], 1, 10, False).lists) == (1021, 256)
    assert (regime(TABLE["C2"][0], 1, 10, False).slices, regime(TABLE["C2"][0], 1, 10, False).lists) == (683, 171)      # lists 171 ... 255 empty
    assert (regime(TABLE["D"][0], 1, 10, False).slices, regime(TABLE["D"][0], 1, 10, False).lists) == (705, 177)
    n_d = TABLE["D"][0]
    assert n_d * 1024 * 2 > 4.4e9 and (1 << 21) * 1024 * 2 == 1 << 32 and (1 << 20) * 1024 * 2 == 1 << 31 and n_d > 1 << 21
    # the tails by k and batch size, the select launches by internal passes
    n = TABLE["B3"][0]
    assert regime(n, 130, 2, False).tail == "select-rescore-NT256" and regime(n, 128, 2, False).tail == "select-rescore-NT1024"
    assert regime(n, 300, 32, False).tail == "select-rescore-NT1024"
    assert regime(n, 1100, 10, False).sel == 2 and regime(n, 1100, 10, False).tail == "select-rescore-NT256"
    assert regime(TABLE["A"][0], 16, 32, True).tail == "i8-collect" and regime(TABLE["A"][0], 16, 32, True).sel == 1
    assert regime(TABLE["A"][0], 16, 32, False).tail == "select-rescore-NT1024"
    assert regime(TABLE["B2"][0], 257, 10, False).sel == 1 and regime(TABLE["B2"][0], 256, 1, False).sel == 0


def test_regime_flips_at_2_20_rows_and_reaches_256_lists_at_2041_super_groups():
    assert regime(LINE, 40, 10, False).tail == "f16-inblock" and regime(LINE + 1, 40, 10, False).tail == "select-rescore-NT1024"
    assert regime(LINE, 33, 10, True).tail == "i8-inblock" and regime(LINE + 1, 33, 10, True).tail == "i8-collect"
    first = min(s for s in range(1, 4000) if regime(s * 1024, 1, 10, False).nsplit == 256)
    assert first == 2041 and regime(2040 * 1024, 1, 10, False).nsplit == 255
    assert regime(2041 * 1024 - 1023, 1, 10, False).n_super == 2041 and regime(2040 * 1024 + 1, 1, 10, False).lists == 256
    # beyond the cap a slice takes more than two super-groups and trailing lists stay empty
    r = regime(2049 * 1024, 1, 10, False)
    assert r.per == 3 and r.lists < r.nsplit == 256


def test_the_planter_covers_every_span_and_the_last_select_list():
    for d, prefixes in DIM_SHARDS.items():
        graded, ties = plant_rows(prefixes)
        every = np.concatenate([graded[n].reshape(-1) for n in prefixes] + [np.asarray(ties)])
        assert np.unique(every).shape[0] == every.shape[0], (d, "a row planted twice")
        for n in prefixes:
            rows = graded[n]
            assert rows.shape == (N_GRADED, PLANT_K + 3) and rows.min() > 0 and rows.max() < n - 1
            assert sorted(span_of(r, n) for r in rows[:, 0]) == list(range(N_SPANS)), (n, "a span without a rank-1 row")
            for j in range(N_GRADED):
                assert len({span_of(r, n) for r in rows[j]}) == PLANT_K + 3, (n, j, "two ranks of one query in one span")
            mine = tie_rows(n)
            assert mine <= set(ties) and {0, n - 1, last_list_first_row(n)} <= mine
            assert {span_of(r, n) for r in mine} == set(range(N_SPANS))
            assert all((r in mine) == (r < n) for r in (LINE - 1, LINE))
            # the last non-empty select list holds a rank-1 row: a graded query's best where the list has room, the tied vector always
            first = last_list_first_row(n)
            assert first < n and first in mine
            if first + 2 < n:
                assert (rows[:, 0] > first).any(), n
            assert len(rows[:, 0]) == len(set(rows[:, 0] // 64)), (n, "two best rows in one group")
    # batches are nested, keep the zero query first and hold every planted query from 18 queries on
    for nq in (1, 8, 16, 18, 33, 40, 130, 300, 1100):
        b = batch_indices(nq)
        assert len(b) == nq == len(set(b)) and b[0] == 0 and set(b) <= set(batch_indices(1100))
        if nq >= 18:
            assert set(range(GRADED0, TIED_Q + 1)) <= set(b)
    assert set(batch_indices(40)) <= set(batch_indices(130)) <= set(batch_indices(300))


def test_clearing_any_span_changes_a_planted_answer_in_float64():
    """A scaled-down shard (dim 64) planted by the same functions: by a float64 numpy product the k + 3 best rows of every graded query
    are its planted rows in rank order, the tied query's best rows are the tied rows, and with any one span's rows removed the top-k of
    at least one planted query changes: a tail that loses any one wave's share cannot pass."""
    d, k = 64, PLANT_K
    for n in (16 * 300 + 37, 16 * 1024 + 1):
        rs = np.random.RandomState(n)
        unit = lambda m: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16))(rs.randn(m, d))
        C = unit(n)
        q16, v16 = unit(N_GRADED), unit(1)[0]
        graded, ties = plant_rows([n])
        rows, vals = plant_values(graded[n], ties, q16, v16)
        C[rows] = vals
        Q = np.concatenate([q16, v16[None]]).astype(np.float64)
        e = Q @ C.astype(np.float64).T                                           # [17, n]
        order = np.argsort(-e, axis=1, kind="stable")
        for j in range(N_GRADED):
            planted = e[j, graded[n][j]]
            assert (np.diff(planted) <= 0).all() and planted[-1] > 0.9, (n, j, "the near-copies are not graded")
            assert set(order[j, :k + 3]) == set(graded[n][j]), (n, j, "chance rows among the planted ranks")
            assert order[j, 0] == graded[n][j, 0] or e[j, order[j, 0]] == planted[0]
        assert set(order[N_GRADED, :len(ties)]) == set(ties) and len(set(e[N_GRADED, ties])) == 1
        top = [set(order[j, :k]) for j in range(N_GRADED + 1)]
        span = -(-n // N_SPANS)
        for s in range(N_SPANS):
            e2 = e.copy()
            e2[:, s * span:min(n, (s + 1) * span)] = -np.inf
            changed = [j for j in range(N_GRADED + 1) if set(np.argsort(-e2[j], kind="stable")[:k]) != top[j]]
            assert s in changed or (s > 0 and changed), (n, s, "no planted answer depends on this span")
            assert any(j < N_GRADED for j in changed), (n, s)


def test_near_copies_move_towards_zero_one_ulp_at_a_time():
    q = np.array([0.5, -0.25, 2.0 ** -14, -2.0 ** -24, 0.0, 1.0], np.float16)
    c = near_copies(q)
    assert c.shape == (len(GRADES), 6) and (c[0] == q).all()
    assert (np.abs(c.astype(np.float64)) <= np.abs(q.astype(np.float64))).all() and (np.sign(c) * np.sign(q) >= 0).all()
    assert c[1, 0] == np.nextafter(np.float16(0.5), np.float16(0)) and (c[1, 1:] == q[1:]).all()
    assert (c[-1, 3:5] == 0).all()                                               # the smallest subnormal and zero stay at zero
    moved = (q.view(np.uint16).astype(np.int64) & 0x7FFF) - (c[7].view(np.uint16).astype(np.int64) & 0x7FFF)
    assert GRADES[7] == 64 and moved.tolist() == [11, 11, 11, 1, 0, 10]          # 64 moves dealt round 6 components; none below zero
