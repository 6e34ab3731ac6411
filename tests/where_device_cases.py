"""The metadata fixture and the filters shared by tests/test_where_device_host.py and tests/test_gpu_where_device.py (no tests in here).

Keys of the fixture:
  num     ints, floats, -0.0, 0.0, NaN, an int above 2^53; missing from some rows
  s       strings: empty, non-ASCII, prefixes of each other ("a" / "ab" / "abc"); missing from some rows
  t       strings without the empty one, so an operand can lie below the whole dictionary ("b", "bb", "d", "dé")
  flag    bools; missing from some rows
  mix     numbers, strings, bools, None and a list within one key
  sparse  a number in every 37th row only
  nokey   in no row
"""
import numpy as np

NUMS = [0, 1, 2, 3, -1, 2.5, -0.0, 0.0, float("nan"), 2 ** 53 + 1, 2 ** 53, 1e300, -7, 3.0, 10]
STRS = ["", "a", "ab", "abc", "b", "é", "日本", "z", "ab́", "A"]
TSTRS = ["b", "bb", "d", "dé"]
MIX = [1, "1", True, None, [1], 2.0, "a", False, 0, ""]
KEYS = ("num", "s", "t", "flag", "mix", "sparse", "nokey")


def make_metadata(n: int, seed: int = 0):
    rs = np.random.RandomState(seed)
    out = []
    for r in range(n):
        m = {"chunk_id": f"c{r}"}
        if rs.rand() < 0.85:
            m["num"] = NUMS[rs.randint(len(NUMS))]
        if rs.rand() < 0.85:
            m["s"] = STRS[rs.randint(len(STRS))]
        if rs.rand() < 0.9:
            m["t"] = TSTRS[rs.randint(len(TSTRS))]
        if rs.rand() < 0.8:
            m["flag"] = bool(rs.randint(2))
        if rs.rand() < 0.9:
            m["mix"] = MIX[rs.randint(len(MIX))]
        if r % 37 == 5:
            m["sparse"] = r
        out.append(m)
    return out


_CMP = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte")
NUM_OPERANDS = [3, 2.5, -0.0, 0, float("nan"), 2 ** 53 + 1, 2 ** 53, -100, 1e301, np.int64(2), np.float32(2.5), 3.0]
STR_OPERANDS = ["", "a", "ab", "abc", "aa", "abd", "é", "日本", "zz", "\U0001d53d", "B"]       # present, between, above the dictionary of `s`
T_OPERANDS = ["a", "b", "c", "bb", "d", "dé", "e", ""]                                        # "a" and "" lie below the dictionary of `t`


def fixed_filters():
    """Every operator on every kind it accepts, on every key (a key of another kind included), the set cases and some trees."""
    fs = []
    for key in ("num", "mix", "sparse", "nokey", "s"):
        for x in NUM_OPERANDS:
            fs += [{key: {op: x}} for op in _CMP]
        fs.append({key: 3})
    for key, operands in (("s", STR_OPERANDS), ("t", T_OPERANDS), ("mix", ["1", "a", "", "0"]), ("nokey", ["a"]), ("num", ["a"])):
        for x in operands:
            fs += [{key: {op: x}} for op in _CMP]
        fs.append({key: operands[0]})
    for key in ("flag", "mix", "num", "nokey"):
        for x in (True, False):
            fs += [{key: {"$eq": x}}, {key: {"$ne": x}}, {key: x}, {key: {"$in": [x]}}, {key: {"$nin": [x]}}]
        fs += [{key: {"$in": [True, False]}}, {key: {"$nin": [False, True, True]}}]
    for op in ("$in", "$nin"):
        fs += [{"num": {op: [1, 2.5, 3]}}, {"num": {op: [0]}}, {"num": {op: [-0.0, float("nan")]}}, {"num": {op: [float("nan")]}},
               {"num": {op: [2 ** 53]}}, {"num": {op: [77, 78]}}, {"num": {op: list(range(-20, 20))}}, {"mix": {op: [1, 2, 0]}},
               {"s": {op: ["a", "nope", "日本"]}}, {"s": {op: ["nope", "never"]}}, {"s": {op: [""]}}, {"s": {op: STRS + ["q"]}},
               {"t": {op: ["a", "c", "e"]}}, {"t": {op: ["dé", "b"]}}, {"mix": {op: ["1", "", "x"]}}, {"nokey": {op: ["a"]}}, {"nokey": {op: [1]}},
               {"sparse": {op: [5, 42, 79]}}]
    fs += [
        {"num": {"$gte": 1, "$lt": 3}},
        {"num": {"$gte": 1}, "s": {"$lt": "b"}, "flag": True},
        {"$and": [{"s": "ab"}, {"num": {"$ne": 2}}]},
        {"$or": [{"s": {"$gt": "abc"}}, {"flag": False}, {"nokey": {"$ne": 1}}]},
        {"$and": [{"$or": [{"t": {"$lte": "bb"}}, {"num": {"$in": [0, 1]}}]}, {"$or": [{"flag": {"$ne": True}}, {"$and": [{"mix": "a"}, {"s": {"$nin": ["a"]}}]}]}]},
        {"$or": [{"$and": [{"num": {"$lt": 0}}]}, {"$or": [{"$or": [{"s": ""}]}]}]},
        {"$and": [{"sparse": {"$gt": 100}}], "t": {"$ne": "d"}},
    ]
    return fs


def _random_leaf(rs):
    kind = rs.randint(4)
    if kind == 0:
        key = ("num", "mix", "sparse", "nokey")[rs.randint(4)]
        pool = NUM_OPERANDS
    elif kind == 1:
        key = ("s", "mix")[rs.randint(2)]
        pool = STR_OPERANDS
    elif kind == 2:
        key, pool = "t", T_OPERANDS
    else:
        key = ("flag", "mix")[rs.randint(2)]
        x = bool(rs.randint(2))
        return {key: {("$eq", "$ne")[rs.randint(2)]: x}} if rs.rand() < 0.7 else {key: {("$in", "$nin")[rs.randint(2)]: [x]}}
    if rs.rand() < 0.25:
        vals = [pool[i] for i in rs.randint(len(pool), size=rs.randint(1, 6))]
        if key == "num" and rs.rand() < 0.3:
            vals += list(range(int(rs.randint(12))))
        return {key: {("$in", "$nin")[rs.randint(2)]: vals}}
    return {key: {_CMP[rs.randint(6)]: pool[rs.randint(len(pool))]}}


def _random_tree(rs, depth):
    if depth == 0 or rs.rand() < 0.3:
        return _random_leaf(rs)
    if rs.rand() < 0.2:                                       # several keys in one dict
        out = {}
        for _ in range(rs.randint(2, 4)):
            out.update(_random_leaf(rs))
        return out
    return {("$and", "$or")[rs.randint(2)]: [_random_tree(rs, depth - 1) for _ in range(rs.randint(1, 5))]}


def count_leaves(f) -> int:
    """Leaves of the compiled tree of filter dict `f`: one per (key, operator)."""
    n = 0
    for key, val in f.items():
        if key in ("$and", "$or"):
            n += sum(count_leaves(c) for c in val)
        else:
            n += len(val) if isinstance(val, dict) else 1
    return n


def random_filters(count: int = 300, seed: int = 11, max_leaves: int = 32):
    """Seeded random trees of up to 4 levels with at most `max_leaves` leaves each (larger draws are skipped)."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        f = _random_tree(rs, rs.randint(1, 5))
        if count_leaves(f) <= max_leaves:
            out.append(f)
    return out


def right_leaning(n_leaves: int, key: str = "num"):
    """and(l1, or(l2, and(l3, ...))) with `n_leaves` leaves: n_leaves - 1 nested levels, postfix stack depth n_leaves."""
    node = {key: {"$gte": n_leaves % 5 - 1}}
    for j in range(n_leaves - 1, 0, -1):
        leaf = {key: {("$gte", "$lt", "$ne")[j % 3]: j % 4}} if j % 2 else {"s": {("$gte", "$lt")[j % 4 // 2]: STRS[j % len(STRS)]}}
        node = {("$and", "$or")[j % 2]: [leaf, node]}
    return node


def chain(levels: int, leaf=None):
    """`levels` nested single-child `$and` / `$or` nodes over one leaf."""
    node = leaf or {"num": {"$gt": 0}}
    for j in range(levels):
        node = {("$and", "$or")[j % 2]: [node]}
    return node
