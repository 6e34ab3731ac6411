"""The refusals of the five row-selecting modes (`graph_ef`, `pq_candidates`, `boost_weight`, `binary_candidates`, `nprobe`) through the
three front ends (`retrieval.retrieve`, `HipCollection.query`, `search_queries`), message by message (no GPU).  Every expected string
below was written out by hand from the five `check_query_with_*` functions; a whole message is compared with `==`.  Nothing is
launched: the index, the queries' model and the shard are None or stubs without a device.

Which refusal wins when two modes are given together follows the order a front end checks them in: `retrieve` and `query` graph, PQ,
boost, binary, nprobe; `search_queries` boost, graph, PQ, binary, nprobe (so `boost_weight` with `pq_candidates` is worded by the
boost there and by the PQ elsewhere).  `search_queries` builds its own indexes, so it has no "no index built" case; `retrieve` and
`search_queries` let `nprobe` through with `min_score` and per-query filter lists, which shows as the NEXT refusal of that mode."""
import types

import numpy as np
import pytest

MODES = ("graph_ef", "pq_candidates", "boost_weight", "binary_candidates", "nprobe")
VALUE = {"graph_ef": 64, "pq_candidates": 64, "boost_weight": 0.1, "binary_candidates": 64, "nprobe": 4}

# two modes together, by the pair (unordered): what `retrieve` and `query` raise
PAIR = {
    frozenset(("graph_ef", "pq_candidates")): "graph_ef cannot be combined with pq_candidates: both choose which rows get scored",
    frozenset(("graph_ef", "boost_weight")): "graph_ef cannot be combined with boost_weight: the boosted search reads every row",
    frozenset(("graph_ef", "binary_candidates")): "graph_ef cannot be combined with binary_candidates: both choose which rows get scored",
    frozenset(("graph_ef", "nprobe")): "graph_ef cannot be combined with nprobe: both choose which rows get scored",
    frozenset(("pq_candidates", "boost_weight")): "pq_candidates cannot be combined with boost_weight: the boosted search reads every row",
    frozenset(("pq_candidates", "binary_candidates")): "pq_candidates cannot be combined with binary_candidates: both choose which rows get scored",
    frozenset(("pq_candidates", "nprobe")): "pq_candidates cannot be combined with nprobe: both choose which rows get scored",
    frozenset(("boost_weight", "binary_candidates")): "boost_weight cannot be combined with binary_candidates: a boosted binary-code search is out of scope",
    frozenset(("boost_weight", "nprobe")): "boost_weight cannot be combined with nprobe: a boosted IVF search is out of scope",
    frozenset(("binary_candidates", "nprobe")): "binary_candidates cannot be combined with nprobe: both choose which rows get scored",
}
# ... and what `search_queries` raises, which checks the boost first
PAIR_CLI = {**PAIR, frozenset(("pq_candidates", "boost_weight")):
            "boost_weight cannot be combined with pq_candidates: a boosted product-quantised search is out of scope"}

HYBRID = {
    "graph_ef": "graph_ef cannot be combined with hybrid_alpha: the BM25 keyword search has no graph",
    "pq_candidates": "pq_candidates cannot be combined with hybrid_alpha: the BM25 keyword search has no PQ codes",
    "boost_weight": "boost_weight cannot be combined with hybrid_alpha: the fusion ranks by its own score",
    "binary_candidates": "binary_candidates cannot be combined with hybrid_alpha: the BM25 keyword search has no binary codes",
    "nprobe": "nprobe cannot be combined with hybrid_alpha: the BM25 keyword search has no inverted lists of topics",
}
GROUP_BY = {
    "graph_ef": "graph_ef cannot be combined with group_by: the grouped search reads every row",
    "pq_candidates": "pq_candidates cannot be combined with group_by: the grouped search reads every row",
    "boost_weight": "boost_weight cannot be combined with group_by: a boosted grouped search is out of scope",
    "binary_candidates": "binary_candidates cannot be combined with group_by: the grouped search reads every row",
    "nprobe": "nprobe cannot be combined with group_by: the grouped search reads every row",
}
MIN_SCORE = {
    "graph_ef": "graph_ef cannot be combined with min_score: the range search reads every row",
    "pq_candidates": "pq_candidates cannot be combined with min_score: the range search reads every row",
    "boost_weight": "boost_weight cannot be combined with min_score: a boosted range search is out of scope",
    "binary_candidates": "binary_candidates cannot be combined with min_score: the range search reads every row",
    "nprobe": "nprobe cannot be combined with min_score: the range search reads every row",
}
PER_QUERY = {
    "graph_ef": "graph_ef cannot be combined with per-query filter lists: the graph search takes one bitmap per call",
    "pq_candidates": "pq_candidates cannot be combined with per-query filter lists: the code scan takes one bitmap per call",
    "boost_weight": "boost_weight cannot be combined with per-query filter lists: the boosted search takes one bitmap per call",
    "binary_candidates": "binary_candidates cannot be combined with per-query filter lists: the Hamming scan takes one bitmap per call",
    "nprobe": "nprobe cannot be combined with per-query filter lists: the IVF search takes one bitmap per call",
}
WORLD = {
    "graph_ef": "graph_ef needs world == 1: more than one rank is out of scope",
    "pq_candidates": "pq_candidates needs world == 1: more than one rank is out of scope",
    "boost_weight": "boost_weight needs world == 1: more than one rank is out of scope",
    "binary_candidates": "binary_candidates needs world == 1: more than one rank is out of scope",
    "nprobe": "nprobe needs world == 1: more than one rank is out of scope",
}
NO_INDEX = {
    "graph_ef": "graph_ef needs a graph index: call build_graph() first",
    "pq_candidates": "pq_candidates needs a PQ index: call build_pq() first",
    "boost_weight": "boost_weight needs a prior: call set_boost() first",
    "binary_candidates": "binary_candidates needs a binary index: call build_binary() first",
    "nprobe": "nprobe needs an IVF index: call build_ivf(n_lists) first",
}
NPROBE_TOO_LARGE = "nprobe=200 must be an integer in [1, 128]"       # the refusal behind the two that `nprobe` is let through


class Untouchable:
    """An index nothing may read: any attribute but the few the refusals ask for with a default is an error."""
    def __getattr__(self, name):
        if name in ("stale", "n_entry_lists", "degree", "n_lists"):
            raise AttributeError(name)                           # (`getattr(index, name, default)` gives the default)
        raise AssertionError(f"the index was touched: .{name}")


def _message(call):
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


# ---- retrieve ------------------------------------------------------------------------------------------------------------------------
RETRIEVE_INDEX = {"graph_ef": "graph", "pq_candidates": "pq", "boost_weight": "prior", "binary_candidates": "binary", "nprobe": "ivf"}


def _retrieve(modes, built=True, **kw):
    import torch
    from arxiv_rag_amd.retrieval import retrieve
    given = {m: VALUE[m] for m in modes}
    if built:
        given.update({RETRIEVE_INDEX[m]: Untouchable() for m in modes})
    return _message(lambda: retrieve(None, torch.zeros((2, 64), dtype=torch.float16), None, 10, **given, **kw))


@pytest.mark.parametrize("a", MODES)
@pytest.mark.parametrize("b", MODES)
def test_retrieve_two_modes_together(a, b):
    if a != b:
        assert _retrieve((a, b)) == PAIR[frozenset((a, b))]


@pytest.mark.parametrize("mode", MODES)
def test_retrieve_a_mode_with_the_shared_context(mode):
    assert _retrieve((mode,), hybrid_alpha=0.5) == HYBRID[mode]
    assert _retrieve((mode,), grouped=True) == GROUP_BY[mode]
    assert _retrieve((mode,), world=2) == WORLD[mode]
    assert _retrieve((mode,), built=False) == NO_INDEX[mode]
    if mode == "nprobe":                                         # let through: the next refusal of the mode is the one raised
        assert _retrieve((mode,), built=False, min_score=0.2) == NO_INDEX[mode]
        assert _retrieve((mode,), built=False, where=[None, None]) == NO_INDEX[mode]
        assert _retrieve((mode,), built=False, where_document=[None, None]) == NO_INDEX[mode]
    else:
        assert _retrieve((mode,), min_score=0.2) == MIN_SCORE[mode]
        assert _retrieve((mode,), where=[None, None]) == PER_QUERY[mode]
        assert _retrieve((mode,), where_document=[None, None]) == PER_QUERY[mode]


# ---- HipCollection.query ---------------------------------------------------------------------------------------------------------------
QUERY_INDEX = {"graph_ef": "graph", "pq_candidates": "pq", "binary_candidates": "binary", "nprobe": "ivf"}


def _query(modes, built=True, world=1, **kw):
    from arxiv_rag_amd.store import HipCollection
    col = HipCollection.__new__(HipCollection)
    col.world, col._keep, col._deleted = world, None, None
    for m in modes if built else ():
        if m == "boost_weight":
            col._boost_buf, col.lo, col.hi = np.zeros(4, np.float32), 0, 4
        else:
            setattr(col, QUERY_INDEX[m], Untouchable())
    return _message(lambda: col.query(query_embeddings=np.zeros((1, 64), np.float32), **{m: VALUE[m] for m in modes}, **kw))


@pytest.mark.parametrize("a", MODES)
@pytest.mark.parametrize("b", MODES)
def test_query_two_modes_together(a, b):
    if a != b:
        assert _query((a, b)) == PAIR[frozenset((a, b))]


@pytest.mark.parametrize("mode", MODES)
def test_query_a_mode_with_the_shared_context(mode):
    assert _query((mode,), hybrid_alpha=0.5) == HYBRID[mode]
    assert _query((mode,), group_by=True) == GROUP_BY[mode]
    assert _query((mode,), min_score=0.5) == MIN_SCORE[mode]
    assert _query((mode,), where=[None]) == PER_QUERY[mode]
    assert _query((mode,), where_document=[None]) == PER_QUERY[mode]
    assert _query((mode,), world=2) == WORLD[mode]
    assert _query((mode,), built=False) == NO_INDEX[mode]


# ---- search_queries --------------------------------------------------------------------------------------------------------------------
CLI_ALSO = {"boost_weight": {"boost_spec": {"key": "quality_score", "missing": 0.0}}, "nprobe": {"ivf_lists": 8}}
SHARD = types.SimpleNamespace(rows=np.zeros((100, 64), np.float16))     # (its shape is all the refusals read)


def _search_queries(modes, **kw):
    from arxiv_rag_amd import generate_embeddings_parallel as G
    given = {}
    for m in modes:
        given.update({m: VALUE[m], **CLI_ALSO.get(m, {})})
    given.update(kw)
    return _message(lambda: G.search_queries(None, [], SHARD, ["q"], **given))


@pytest.mark.parametrize("a", MODES)
@pytest.mark.parametrize("b", MODES)
def test_search_queries_two_modes_together(a, b, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if a != b:
        assert _search_queries((a, b)) == PAIR_CLI[frozenset((a, b))]


@pytest.mark.parametrize("mode", MODES)
def test_search_queries_a_mode_with_the_shared_context(mode, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert _search_queries((mode,), hybrid_alpha=0.5) == HYBRID[mode]
    assert _search_queries((mode,), group_by_paper=True) == GROUP_BY[mode]
    if mode == "nprobe":                                         # let through: the next refusal of the mode is the one raised
        assert _search_queries((mode,), min_score=0.3, nprobe=200) == NPROBE_TOO_LARGE
        assert _search_queries((mode,), where=[None], nprobe=200) == NPROBE_TOO_LARGE
    else:
        assert _search_queries((mode,), min_score=0.3) == MIN_SCORE[mode]
        assert _search_queries((mode,), where=[None]) == PER_QUERY[mode]
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert _search_queries((mode,)) == WORLD[mode]
