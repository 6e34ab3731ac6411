"""Graphs and cases the graph tests share.  Pure numpy, importable without a GPU.

`ring` serves tests/test_graph_host.py and tests/test_gpu_graph.py.  Everything below it builds the cases of the large suite: the CPU
module tests/test_graph_cases_host.py proves with the restatements alone that every case lands on the branch it is meant for, the GPU
module tests/test_gpu_graph_large.py runs the same cases on the device.  A case is computed once a process (`functools.lru_cache`) and
never written to afterwards.

The corpus (`big_corpus`) is a function of the row number (a counter hash), so a row has the same bits whatever else is generated; it
has 2^20 + 197 unit rows at dim 64 and carries every plant of every case:
  PLATEAU_ROWS            200 copies of row 5 between row 5 and row 2^20 + 100
  HIGH_ROWS               copies of the four queries `high_queries()` at rows 2^20 - 1, 2^20, 2^20 + 1 and the last row
Cases that need an order of rows take it from the planted corpus, so a plant cannot move a case off its branch unseen.
"""
import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

I32_MAX = np.iinfo(np.int32).max
N_BIG = (1 << 20) + 197
DIM = 64
N_WORLD = 20000                                                  # the rows of the random-graph world: the first of the big corpus
PLATEAU_ROWS = 5 + np.arange(200, dtype=np.int64) * 5269
PLATEAU_ROWS[-2:] = [(1 << 20) + 37, (1 << 20) + 100]
HIGH_ROWS = np.array([(1 << 20) - 1, 1 << 20, (1 << 20) + 1, N_BIG - 1], np.int64)
CAPACITY_SHAPES = ((64, 64, 127), (32, 32, 255), (8, 8, 1023))  # (degree, n_entries, max_iters): n_entries + max_iters * degree = 8192
EF_SHAPES = ((63, 8, 4, 300), (65, 64, 64, 127), (127, 32, 8, 255), (129, 16, 8, 511), (511, 8, 8, 1023))     # (ef, degree, n_entries, max_iters)


def ring(lo, hi, n):
    """neighbors int32 [n, 8]: inside [lo, hi) row i -> i +- 1 .. 4 around the ring; the other rows have no edge."""
    nb = np.full((n, 8), -1, np.int32)
    m = hi - lo
    for i in range(lo, hi):
        nb[i] = [lo + (i - lo + d) % m for d in (1, -1, 2, -2, 3, -3, 4, -4)]
    return nb


# ---- the visited table ----------------------------------------------------------------------------------------------------------------
def table_constants():
    """(slots, multiplier, shift) of the search kernel's visited table, read from csrc/graph.hip."""
    src = (Path(__file__).resolve().parents[1] / "arxiv_rag_amd" / "csrc" / "graph.hip").read_text()
    slots = re.search(r"\bconstexpr\s+int\s+GRAPH_SLOTS\s*=\s*(\d+)\s*;", src)
    hashed = re.search(r"\(\(uint32_t\)r\s*\*\s*(0x[0-9A-Fa-f]+)u\)\s*>>\s*(\d+)\s*;", src)
    assert slots and hashed, "graph.hip no longer has GRAPH_SLOTS or the hash of the visited table in the form the tests read"
    return int(slots.group(1)), int(hashed.group(1), 16), int(hashed.group(2))


def home_slots(rows, mult, shift):
    """The slot a row's probe starts at: (uint32(row) * mult) >> shift."""
    return ((np.asarray(rows, dtype=np.uint64) * np.uint64(mult)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


def home_slot_rows(n_rows, lo_slot, mult=0x9E3779B1, shift=18):
    """The rows of [0, n_rows) whose home slot is >= lo_slot, ascending."""
    rows = np.arange(n_rows, dtype=np.int64)
    return rows[home_slots(rows, mult, shift) >= lo_slot]


def table_model(rows, slots, mult, shift):
    """(longest probe in steps, inserts that wrapped past the last slot, final occupancy) of an open-addressing table with the kernel's
    hash and probe rule, the rows offered one after the other: a probe walks from the home slot to the first slot that is empty or
    holds the row, and `(s + 1) & (slots - 1)` takes it from the last slot to slot 0.  Plain Python; `list.index` is the walk."""
    tab, where = [-1] * slots, {}
    longest = wrapped = 0
    for r in (int(v) for v in rows):
        home = ((r * mult) & 0xFFFFFFFF) >> shift
        if r in where:                                           # the slots between stayed full: the probe stops at the row itself
            s = where[r]
        else:
            try:
                s = tab.index(-1, home)
            except ValueError:
                s = tab.index(-1)                                # past the last slot (ValueError: the table is full)
            tab[s], where[r] = r, s
            wrapped += s < home
        longest = max(longest, (s - home) % slots)
    return longest, wrapped, len(where)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
def fresh_tree(n_entries, degree, n_nodes):
    """(neighbors int32 [n_nodes, degree], entries int32 [n_entries]): node v's neighbours are n_entries + v * degree + j (no edge where
    that is no node), the roots are 0 .. n_entries - 1.  Every node has exactly one parent, so every expansion of a node whose
    children exist, in any order, offers `degree` rows never seen before."""
    nb = n_entries + np.arange(n_nodes, dtype=np.int64)[:, None] * degree + np.arange(degree, dtype=np.int64)[None, :]
    return np.where(nb < n_nodes, nb, -1).astype(np.int32), np.arange(n_entries, dtype=np.int32)


def relabel(graph, rows, n_rows):
    """int32 [n_rows, degree]: `graph` with node i at row rows[i]; the rows outside `rows` get no edges."""
    graph, rows = np.asarray(graph), np.asarray(rows, dtype=np.int64)
    out = np.full((n_rows, graph.shape[1]), -1, np.int32)
    out[rows[:graph.shape[0]]] = np.where(graph >= 0, rows[np.clip(graph, 0, None)], -1).astype(np.int32)
    return out


def walk_order(n_entries, degree, max_iters):
    """The nodes of `fresh_tree(n_entries, degree, n_entries + max_iters * degree)`, best first, for a walk that expands exactly the
    max_iters nodes that have children (0 .. max_iters - 1) and so visits every node.  The walk takes the best unexpanded row of the
    beam, and a row stays in a beam of `ef` only while fewer than ef visited rows are better: in index order (breadth first) node
    512 would have 512 better rows above it.  So the order is last in, first out: the children of the node just expanded are better
    than everything seen before, a higher index is better among them, and a node waits only for the subtrees of its later siblings
    (at most 511 nodes at degree 8 with 1023 iterations, the largest shape the table admits).  The nodes without children are worst."""
    n_inner, batch = max_iters, {}
    stack, t = list(range(min(n_entries, n_inner))), 0
    for v in stack:
        batch[v] = -1
    while stack:
        v = stack.pop()
        kids = [c for c in range(n_entries + v * degree, n_entries + (v + 1) * degree) if c < n_inner]
        for c in kids:
            batch[c] = t
        stack += kids
        t += 1
    assert len(batch) == n_inner
    inner = sorted(range(n_inner), key=lambda v: (batch[v], v), reverse=True)
    return np.array(inner + list(range(n_inner, n_entries + max_iters * degree)), np.int64)


def rows_by_key(X, rows, q):
    """`rows` sorted by the kernel's key against the query q (fp16 [dim]): score word descending, row ascending."""
    from arxiv_rag_amd.graph import order_words
    from arxiv_rag_amd.topics import exact_scores_host
    rows = np.asarray(rows, dtype=np.int64)
    w = order_words(exact_scores_host(X[rows], q[None, :])[:, 0]).astype(np.int64)
    return rows[np.lexsort((rows, -w))]


def tree_rows(X, rows, q, n_entries, degree, max_iters):
    """int64 [len(rows)]: the row of every node of the fresh tree, so that query q walks it in `walk_order`: the best row is the best node."""
    out = np.empty(len(rows), np.int64)
    out[walk_order(n_entries, degree, max_iters)] = rows_by_key(X, rows, q)
    return out


def plateau(X, rows, src):
    """X with row `src` copied into `rows` (in place; returns X)."""
    X[np.asarray(rows, dtype=np.int64)] = X[src]
    return X


def bad_edge_graph(n, degree, seed):
    """tests/test_gpu_graph.py's random_graph: random edges, about 5 % of them bad: -1, n, INT32_MAX, a self-loop or a repeat of the
    row's first edge."""
    rs = np.random.RandomState(seed)
    nb = rs.randint(0, n, (n, degree)).astype(np.int32)
    kind = rs.randint(0, 100, (n, degree))
    nb[kind == 0], nb[kind == 1], nb[kind == 2] = -1, min(n, I32_MAX), I32_MAX
    nb = np.where(kind == 3, np.arange(n, dtype=np.int32)[:, None], nb)
    nb[:, 1:] = np.where(kind[:, 1:] == 4, nb[:, :1], nb[:, 1:])
    return nb


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def _mix(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def unit_rows_at(rows, dim, seed):
    """fp16 [len(rows), dim]: unit rows that depend on (row, column, seed) alone."""
    rows = np.asarray(rows, dtype=np.uint64)
    out = np.empty((rows.shape[0], dim), np.float16)
    step = max(1, (1 << 22) // dim)
    for a in range(0, rows.shape[0], step):
        idx = rows[a:a + step, None] * np.uint64(dim) + np.arange(dim, dtype=np.uint64)[None, :]
        u = (_mix(idx + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)) >> np.uint64(11)).astype(np.float64) / float(1 << 53) - 0.5
        out[a:a + step] = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float16)
    return out


def high_queries():
    return unit_rows_at(np.arange(4), DIM, 7003)


@functools.lru_cache(maxsize=None)
def big_corpus():
    """fp16 [N_BIG, DIM] with every plant (the module's docstring).  Read-only."""
    X = unit_rows_at(np.arange(N_BIG), DIM, 7001)
    plateau(X, PLATEAU_ROWS, 5)
    X[HIGH_ROWS] = high_queries()
    X.setflags(write=False)
    return X


def walk_trace(X, nb, q, entries, ef, max_iters, n_rows):
    """The walk of one query (q fp16 [dim], entries int [E]) written a second time, keeping what `search_host` does not return:
    SimpleNamespace(visited: rows in the order scored, expanded: rows in the order expanded, parent_pos: the beam position of every
    parent when it was taken, beam: the final beam's rows best first, words: row -> score word)."""
    from arxiv_rag_amd.graph import order_words
    from arxiv_rag_amd.topics import exact_scores_host
    n = n_rows
    visited, words, beam, done, expanded, parent_pos = [], {}, [], set(), [], []

    def offer(rows):
        new = []
        for r in (int(v) for v in rows):
            if 0 <= r < n and r not in words and r not in new:
                new.append(r)
        if new:
            for r, w in zip(new, order_words(exact_scores_host(X[new], q[None, :])[:, 0])):
                words[r] = int(w)
                beam.append((int(w) << 32) | (0xFFFFFFFF - r))
            visited.extend(new)
            beam[:] = sorted(beam, reverse=True)[:ef]

    offer(entries)
    for _ in range(max_iters):
        pos = next((i for i, key in enumerate(beam) if key not in done), None)
        if pos is None:
            break
        done.add(beam[pos])
        parent_pos.append(pos)
        expanded.append(0xFFFFFFFF - (beam[pos] & 0xFFFFFFFF))
        offer(nb[expanded[-1]])
    return SimpleNamespace(visited=visited, expanded=expanded, parent_pos=parent_pos, beam=[0xFFFFFFFF - (key & 0xFFFFFFFF) for key in beam], words=words)


# ---- the search cases -----------------------------------------------------------------------------------------------------------------
def _search(c, allow=None, k=None, ef=None):
    from arxiv_rag_amd.graph import search_host
    return search_host(c.X[:c.n_rows], c.nb, c.Q, c.ent, c.k if k is None else k, c.ef if ef is None else ef, c.iters, allow=allow,
                       pair_scores=getattr(c, "S", None))


@functools.lru_cache(maxsize=None)
def capacity_case(degree):
    """The fresh tree at the table's capacity: three queries, query j on the tree over the rows [8192 j, 8192 (j + 1)) laid out by its
    own keys, so each walks its own tree in `walk_order` and inserts 8192 rows.  n_rows = 3 * 8192 + 5."""
    n_entries, iters = next((e, t) for d, e, t in CAPACITY_SHAPES if d == degree)
    X, Q = big_corpus(), unit_rows_at(np.arange(3), DIM, 7100 + degree)
    n_rows = 3 * 8192 + 5
    tree, roots = fresh_tree(n_entries, degree, 8192)
    nb = np.full((n_rows, degree), -1, np.int32)
    ent = np.empty((3, n_entries), np.int32)
    for j in range(3):
        rows = tree_rows(X, np.arange(8192 * j, 8192 * (j + 1)), Q[j], n_entries, degree, iters)
        nb[rows] = relabel(tree, rows, n_rows)[rows]
        ent[j] = rows[roots]
    c = SimpleNamespace(X=X, Q=Q, nb=nb, ent=ent, n_rows=n_rows, k=32, ef=512, iters=iters, degree=degree,
                        mask=np.random.RandomState(degree).rand(n_rows) < 0.3)
    c.want, c.want_allow = _search(c), _search(c, allow=c.mask)
    return c


def collision_rows(which):
    slots, mult, shift = table_constants()
    if which == "chain":                                         # 4096 rows whose home is one of the last 64 slots: one chain, and it wraps
        return home_slot_rows(N_BIG, slots - 64, mult, shift)[:4096]
    if which == "half":                                          # 8192 rows in the last 128 slots: the table half full, in one run
        return home_slot_rows(N_BIG, slots - 128, mult, shift)[:8192]
    return home_slot_rows(N_BIG, slots - 1, mult, shift)          # "last": the rows of the last slot alone


@functools.lru_cache(maxsize=None)
def collision_case(which):
    """The table under collision (`collision_rows`).  "chain" and "half": the fresh tree (degree 64, 64 entries, 63 / 127 iterations)
    over the rows, laid out by query 0's keys; query 1 is query 0 doubled (exact in fp16: every score doubles, the order stays), so
    both walk the whole tree.  "last": a ring (degree 8) over the rows of the last slot, one entry, ef 64, three queries.  `nb` is
    built by `collision_graph` (a quarter of a GiB at degree 64: not kept)."""
    X, rows = big_corpus(), collision_rows(which)
    if which == "last":
        Q = unit_rows_at(np.arange(3), DIM, 7203)
        c = SimpleNamespace(X=X, Q=Q, rows=rows, tree=ring(0, len(rows), len(rows)), ent=np.full((3, 1), rows[5], np.int32), n_rows=N_BIG, k=32,
                            ef=64, iters=len(rows), degree=8)
    else:
        iters = len(rows) // 64 - 1
        q = unit_rows_at(np.arange(1), DIM, 7201 if which == "chain" else 7202)[0]
        Q = np.stack([q, q * np.float16(2)])
        assert np.array_equal(Q[1].astype(np.float64), 2 * Q[0].astype(np.float64))
        tree, roots = fresh_tree(64, 64, len(rows))
        rows = tree_rows(X, rows, q, 64, 64, iters)
        c = SimpleNamespace(X=X, Q=Q, rows=rows, tree=tree, ent=np.stack([rows[roots]] * 2).astype(np.int32), n_rows=N_BIG, k=32, ef=512, iters=iters,
                            degree=64)
    c.nb = collision_graph(c)
    c.want = _search(c)
    del c.nb
    return c


def collision_graph(c):
    return relabel(c.tree, c.rows, N_BIG)


@functools.lru_cache(maxsize=None)
def high_rows_case():
    """Rows around 2^20: a ring (degree 8) over the rows [0, 400), the entry row 7 with shortcuts to HIGH_ROWS, which hold copies of the
    four queries and point at each other.  `masks`: only rows >= 2^20 allowed, none, all."""
    X, Q = big_corpus(), high_queries()
    nb = np.full((N_BIG, 8), -1, np.int32)
    nb[:400] = ring(0, 400, 400)
    nb[7, :4] = HIGH_ROWS
    nb[HIGH_ROWS] = np.concatenate([HIGH_ROWS, HIGH_ROWS[::-1]])[None, :]
    rows = np.arange(N_BIG)
    c = SimpleNamespace(X=X, Q=Q, nb=nb, ent=np.full((4, 1), 7, np.int32), n_rows=N_BIG, k=10, ef=64, iters=200, degree=8,
                        masks=(rows >= 1 << 20, np.zeros(N_BIG, bool), np.ones(N_BIG, bool)))
    c.want = _search(c)
    c.want_masks = [_search(c, allow=m) for m in c.masks]
    return c


@functools.lru_cache(maxsize=None)
def world():
    """(X fp16 [N_WORLD, DIM], Q fp16 [3, DIM], S: every pair's exact score): the first rows of the big corpus and three queries."""
    from arxiv_rag_amd.topics import exact_scores_host
    X, Q = big_corpus()[:N_WORLD], unit_rows_at(np.arange(3), DIM, 7300)
    return X, Q, exact_scores_host(X, Q)


def _world_case(degree, n_entries, k, ef, iters, seed):
    X, Q, S = world()
    ent = np.random.RandomState(seed).randint(-2, N_WORLD + 2, (3, n_entries)).astype(np.int32)
    ent[:, 0] = np.clip(ent[:, 0], 0, N_WORLD - 1)               # entries with repeats and values outside the rows, one valid at least
    if n_entries > 1:
        ent[:, -1] = ent[:, 0]
    c = SimpleNamespace(X=X, Q=Q, S=S, nb=bad_edge_graph(N_WORLD, degree, seed), ent=ent, n_rows=N_WORLD, k=k, ef=ef, iters=iters, degree=degree,
                        mask=np.random.RandomState(seed + 1).rand(N_WORLD) < 0.3)
    c.want, c.want_allow = _search(c), _search(c, allow=c.mask)
    return c


@functools.lru_cache(maxsize=None)
def ef_case(ef):
    """Beam widths next to a multiple of 64, walks as long as `max_iters_for` admits, over the random graph with bad edges; k = 32
    (the answer at a smaller k is its prefix: neither the walk nor the allowed list's order depends on k)."""
    degree, n_entries, iters = next(s[1:] for s in EF_SHAPES if s[0] == ef)
    return _world_case(degree, n_entries, 32, ef, iters, {129: 7533}.get(ef, 7400 + ef))      # (seeds at which every width takes a parent from its last chunk)


@functools.lru_cache(maxsize=None)
def turnover_case(ef):
    """The beam turning over: degree 8, 8 entries, 1023 iterations over the random graph, ef 64 or 512."""
    return _world_case(8, 8, 32, ef, 1023, 7500 + ef)


@functools.lru_cache(maxsize=None)
def degree_case(degree):
    """Degrees 24, 40, 56 over the random graph: ef 100, as many iterations as the table admits up to 150."""
    from arxiv_rag_amd.graph import max_iters_for
    return _world_case(degree, 8, 10, 100, min(150, max_iters_for(degree, 8)), 7600 + degree)


@functools.lru_cache(maxsize=None)
def plateau_case():
    """200 identical rows (PLATEAU_ROWS) and a query equal to them: a ring over the 200 in a shuffled order (degree 16: the ring's 8
    and 8 random other rows), the entry in the middle.  The walk always takes the lowest unexpanded plateau row, so the beam (ef 64)
    ends as the 64 lowest plateau rows visited, the answer (k 32) as the lowest 32, and under `mask` (every third plateau row, every
    other row) the answer at k 10 as the lowest 10 allowed ones."""
    X = big_corpus()
    rs = np.random.RandomState(7700)
    order = PLATEAU_ROWS[rs.permutation(200)]
    nb = np.full((N_BIG, 16), -1, np.int32)
    nb[:, :8] = relabel(ring(0, 200, 200), order, N_BIG)
    nb[order, 8:] = rs.randint(0, N_BIG, (200, 8))
    mask = np.ones(N_BIG, bool)
    mask[PLATEAU_ROWS] = np.arange(200) % 3 == 0
    Q = np.stack([X[5], unit_rows_at(np.arange(1), DIM, 7701)[0]])
    c = SimpleNamespace(X=X, Q=Q, nb=nb, ent=np.full((2, 1), order[100], np.int32), n_rows=N_BIG, k=32, ef=64, iters=127, degree=16, mask=mask)
    c.want, c.want_allow = _search(c), _search(c, allow=mask, k=10)
    return c


DIMS = (192, 448, 1088, 4096)                                    # 3, 7, 17 and 64 rounds of eight 16-byte chunks a row
N_DIM_ROWS = 2000


@functools.lru_cache(maxsize=None)
def dim_rows(dim):
    """fp16 [N_DIM_ROWS + 8, dim] unit rows (the last 8: guard rows for the link), rows 1000 and 1001 copies of row 10, and 3 queries."""
    X = unit_rows_at(np.arange(N_DIM_ROWS + 8), dim, 7800 + dim)
    X[1000] = X[1001] = X[10]
    Q = unit_rows_at(np.arange(3), dim, 7900 + dim)
    Q[0] = X[10]
    return X, Q


@functools.lru_cache(maxsize=None)
def dim_case(dim):
    X, Q = dim_rows(dim)
    n = N_DIM_ROWS
    ent = np.random.RandomState(dim).randint(0, n, (3, 4)).astype(np.int32)
    ent[0, 0] = 10
    nb = bad_edge_graph(n, 16, dim)
    nb[10, 0], nb[10, 1] = 1000, 1001
    c = SimpleNamespace(X=X, Q=Q, nb=nb, ent=ent, n_rows=n, k=10, ef=48, iters=40, degree=16)
    c.want = _search(c)
    return c


# ---- the link cases -------------------------------------------------------------------------------------------------------------------
def _csr(lists):
    start = np.zeros(len(lists) + 1, np.int64)
    start[1:] = np.cumsum([len(o) for o in lists])
    return start.astype(np.int32), np.array([r for o in lists for r in o], np.int32)


def _dirty(nb, rows, n, rs):
    """about 6 % bad entries in the given rows of nb: -1, n, INT32_MAX, INT32_MIN, the row itself, a repeat of the first entry"""
    rows = np.asarray(rows, dtype=np.int64)
    part = nb[rows]
    kind = rs.randint(0, 100, part.shape)
    part[kind == 0], part[kind == 1], part[kind == 2], part[kind == 5] = -1, min(n, I32_MAX), I32_MAX, np.iinfo(np.int32).min
    part = np.where(kind == 3, rows[:, None].astype(np.int32), part)
    part[:, 1:] = np.where(kind[:, 1:] == 4, part[:, :1], part[:, 1:])
    nb[rows] = part


@functools.lru_cache(maxsize=None)
def link_dim_case(dim):
    """A small link call at one dim (degree 16, N_DIM_ROWS rows and 8 guard rows): 24 ascending live targets with 0 .. 130 offers
    (the copies of row 10, the target itself and repeats among them) and skipped slots between them."""
    X, _ = dim_rows(dim)
    n, rs = N_DIM_ROWS, np.random.RandomState(dim + 1)
    nb = rs.randint(0, n, (n + 8, 16)).astype(np.int32)
    _dirty(nb, np.arange(n + 8), n, rs)
    live = sorted(set(rs.choice(np.arange(20, n - 1), 21, replace=False).tolist()) | {10, 1000, n - 1})
    targets, lists = [], []
    for j, t in enumerate(live):
        c = (0, 1, 63, 64, 65, 130)[j % 6]
        o = rs.randint(-3, n + 3, c).astype(np.int64)
        if c >= 63:
            o[:5] = [t, 10, 1000, 1001, I32_MAX]
            o[c // 2:] = o[:c - c // 2]
        targets.append(t), lists.append(o.tolist())
        if j % 4 == 1:
            for bad in (t, live[0], -1, n):
                targets.append(bad), lists.append(rs.randint(0, n, 5).tolist())
    start, offers = _csr(lists)
    c = SimpleNamespace(X=X, nb=nb, targets=np.array(targets, np.int32), start=start, offers=offers, n_rows=n, live=live, degree=16)
    from arxiv_rag_amd.graph import link_host
    c.want = link_host(X, nb, c.targets, start, offers, n_rows=n)
    return c


LINK_SHADOW = (1 << 20) - 1000                                   # the early large target: every later slot at or below it is skipped
LINK_HUB, LINK_HIGH_ONLY, LINK_PLATEAU = LINK_SHADOW + 400, LINK_SHADOW + 401, int(PLATEAU_ROWS[-1])


@functools.lru_cache(maxsize=None)
def link_plan():
    """The slots of the large link call over the big corpus, the same for every degree.  -> SimpleNamespace(targets, start, offers and
    the counts the host test checks):
      slots 0, 1      live: rows 3 and 11
      slot 2          live: LINK_SHADOW = 2^20 - 1000, near the top of the range
      2500 slots      targets ascending over [12, LINK_SHADOW), each with 5 offers: all shadowed by slot 2
      then            every other row of (LINK_SHADOW, N_BIG), ascending: live.  Among them LINK_HUB (5000 offers, 2500 rows
                      each twice, 2500 offers apart), LINK_HIGH_ONLY (offers from rows >= 2^20 alone) and LINK_PLATEAU (a copy of the
                      plateau row: its offers hold itself and 100 plateau rows, all of one score: the cut at H falls inside them)
      skipped kinds   (a repeat of the slot before, a descent to a row left out, -1, N_BIG, INT32_MAX; 5 offers each) after the
                      slots 300, 600, 1100 (inside the shadowed run) and 2600, 2800, 3100 (inside the live run): a descent there goes
                      to a row no slot targets, so a slot that wrongly runs changes a row of its own."""
    rs = np.random.RandomState(7950)
    n = N_BIG
    targets, lists, kinds = [3, 11, LINK_SHADOW], [rs.randint(0, n, 70).tolist(), rs.randint(0, n, 3).tolist(), rs.randint(-3, n + 3, 64).tolist()], []
    shadowed = np.sort(rs.choice(np.arange(12, LINK_SHADOW), 2500, replace=False))
    above = np.arange(LINK_SHADOW + 1, n)
    left_out = np.setdiff1d(above[(above - LINK_SHADOW) % 2 == 1], [LINK_HIGH_ONLY])        # every other row is no target: the descents go to three of them
    live_hi = np.setdiff1d(above, left_out)
    descents = iter((LINK_SHADOW + np.array([7, 19, 43])).tolist())
    counts = (0, 1, 5, 63, 64, 65, 130)

    def skipped(last_valid):
        down = next(descents) if last_valid > LINK_SHADOW else int(rs.randint(12, last_valid))
        assert down < last_valid
        for bad in (last_valid, down, -1, n, I32_MAX):
            targets.append(bad), lists.append(rs.randint(0, n, 5).tolist()), kinds.append(len(targets) - 1)

    for t in shadowed.tolist():
        targets.append(t), lists.append(rs.randint(0, n, 5).tolist())
        if len(targets) in (301, 601, 1101):
            skipped(t)
    hub_rows = rs.choice(n, 2500, replace=False)
    for j, t in enumerate(live_hi.tolist()):
        if t == LINK_HUB:
            o = np.concatenate([hub_rows, hub_rows])
        elif t == LINK_HIGH_ONLY:
            o = rs.randint(1 << 20, n, 90)
        elif t == LINK_PLATEAU:
            o = np.concatenate([PLATEAU_ROWS[40:140], [t], rs.randint(0, n, 20)])[rs.permutation(121)]
        else:
            o = rs.randint(-3, n + 3, counts[j % len(counts)])
            if o.shape[0] >= 63:
                o[:3] = [t, I32_MAX, 5]
                o[o.shape[0] // 2:] = o[:o.shape[0] - o.shape[0] // 2]
        targets.append(t), lists.append(np.asarray(o, dtype=np.int64).tolist())
        if len(targets) in (2601, 2801, 3101):
            skipped(t)
    start, offers = _csr(lists)
    live = np.array([3, 11, LINK_SHADOW] + live_hi.tolist(), np.int64)
    return SimpleNamespace(targets=np.array(targets, np.int32), start=start, offers=offers, live=live, n_shadowed=2500, kinds=kinds,
                           most_offers=max(len(o) for o in lists), left_out=left_out)


def link_graph(degree):
    """int32 [N_BIG + 8, degree]: random edges (8 guard rows at the end), the rows the plan names made dirty.  Not kept: up to a quarter GiB."""
    p = link_plan()
    rs = np.random.RandomState(7960 + degree)
    nb = np.random.default_rng(7960 + degree).integers(0, N_BIG, (N_BIG + 8, degree), dtype=np.int32)
    named = np.unique(p.targets[(p.targets >= 0) & (p.targets < N_BIG)])
    _dirty(nb, named, N_BIG, rs)
    return nb


def link_want(degree, nb):
    from arxiv_rag_amd.graph import link_host
    p = link_plan()
    return link_host(big_corpus(), nb, p.targets, p.start, p.offers, n_rows=N_BIG)


# ---- the remap cases ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def remap_masks():
    """Keep-masks over N_BIG rows -> [(name, mask)]: about 3 % of the rows deleted at random, the whole words 1, 2, 77 and the last
    full one deleted, the rows 63, 64, 2^20 - 1 and 2^20 deleted; then rows kept or dropped at the front until the count is 1, 2 and 3
    mod 4; and a mask that keeps the single row 2^20 + 1."""
    rs = np.random.RandomState(7970)
    base = rs.rand(N_BIG) >= 0.03
    for w in (1, 2, 77, N_BIG // 64 - 1):
        base[64 * w:64 * (w + 1)] = False
    base[[63, 64, (1 << 20) - 1, 1 << 20]] = False
    base[[0, 62, (1 << 20) - 2, (1 << 20) + 1, N_BIG - 1]] = True
    out = []
    for want in (1, 2, 3):
        m = base.copy()
        flip = iter(range(3, 62))
        while int(m.sum()) % 4 != want:
            m[next(flip)] ^= True
        out.append((f"count % 4 == {want}", m))
    out.append(("count == 1", np.arange(N_BIG) == (1 << 20) + 1))
    return out


def remap_graph(degree):
    """int32 [N_BIG, degree]: random edges, 2 % of them any bit pattern, 2 % -1."""
    rs = np.random.RandomState(7980 + degree)
    nb = np.random.default_rng(7980 + degree).integers(0, N_BIG, (N_BIG, degree), dtype=np.int32)
    flat = nb.reshape(-1)
    flat[rs.randint(0, flat.shape[0], flat.shape[0] // 50)] = rs.randint(-1 << 31, (1 << 31) - 1, flat.shape[0] // 50, dtype=np.int64).astype(np.int32)
    flat[rs.randint(0, flat.shape[0], flat.shape[0] // 50)] = -1
    return nb


def remap_sample(count, seed):
    """The moved rows compared with `remap_host`: the first and the last 4096 and a random 4096 between them (all of them up to 12288)."""
    if count <= 3 * 4096:
        return np.arange(count)
    mid = np.random.RandomState(seed).choice(np.arange(4096, count - 4096), 4096, replace=False)
    return np.concatenate([np.arange(4096), np.sort(mid), np.arange(count - 4096, count)])


# ---- the assembly case ----------------------------------------------------------------------------------------------------------------
N_ASSEMBLE = (1 << 16) + 3


@functools.lru_cache(maxsize=None)
def clustered_rows():
    """fp16 [N_ASSEMBLE, DIM]: 256 centres, every row a centre plus noise, normalised: k-NN lists with many mutual edges."""
    centres = unit_rows_at(np.arange(256), DIM, 7990).astype(np.float64)
    noise = unit_rows_at(np.arange(N_ASSEMBLE), DIM, 7991).astype(np.float64)
    X = centres[np.arange(N_ASSEMBLE) % 256] + 0.5 * noise
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)


def spoil_lists(knn):
    """The k-NN lists with a few rows emptied and a few entries made invalid (-1, the row count, the row itself): in place, returns knn."""
    n = knn.shape[0]
    rs = np.random.RandomState(7992)
    knn[rs.choice(n, 40, replace=False)] = -1
    for bad in (-1, n, None):
        r, c = rs.randint(0, n, 300), rs.randint(0, knn.shape[1], 300)
        knn[r, c] = r if bad is None else bad
    return knn
