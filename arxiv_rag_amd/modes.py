"""The modes that decide which rows a query scores (`graph_ef`, `pq_candidates`, `boost_weight`, `binary_candidates`, `nprobe`), each
described once, and the one function that refuses from the descriptions.

`check_mode` is what `graph.check_query_with_graph`, `pq.check_query_with_pq`, `boost.check_query_with_boost`,
`binary.check_query_with_binary` and `ivf.check_query_with_nprobe` call; `check_modes` is what `HipCollection.query` and
`retrieval.retrieve` call with every mode's argument at once.  A mode refuses the parts its `order` names, in that order, then more
than one rank, then a missing index, then its own arguments (`check`, a function of the mode's module, imported when the mode is
asked for).  A part a mode does not name it does not refuse: such a pair is either refused by the other mode, which a front end asks
first (`ORDER`), or allowed.
"""
from __future__ import annotations

from dataclasses import dataclass
from importlib import import_module
from typing import Dict, Optional, Tuple

PARTS = {"per_query": "per-query filter lists"}     # how a part is named in a refusal, where that is not its own name


@dataclass(frozen=True)
class Mode:
    name: str                       # the query argument
    order: Tuple[str, ...]          # the parts it refuses, first refusal first: other modes, hybrid_alpha, group_by, min_score, per_query
    needs: str                      # "<an index>: call <its build> first"
    hybrid: str                     # why not with hybrid_alpha
    scan: str                       # its search, as the per-query refusal names it
    check: str                      # "module.function" (width, value, **own): the refusals about its own arguments; imported when asked
    boosted: str = ""               # "a boosted <this> search"
    reads_every_row: bool = False   # the boost; the others choose rows
    counter: Optional[str] = None   # the field of `retrieval.Retrieved` (and key of a result) that counts the rows it scored

    def why(self, part: str) -> str:
        if part == "hybrid_alpha":
            return self.hybrid
        if part == "per_query":
            return f"{self.scan} takes one bitmap per call"
        if self.reads_every_row:
            return f"a boosted {MODES[part].boosted if part in MODES else EVERY_ROW[part]} search is out of scope"
        if part in MODES:
            return "the boosted search reads every row" if MODES[part].reads_every_row else "both choose which rows get scored"
        return f"the {EVERY_ROW[part]} search reads every row"


EVERY_ROW = {"group_by": "grouped", "min_score": "range"}
MODES: Dict[str, Mode] = {m.name: m for m in (
    Mode("graph_ef", ("nprobe", "binary_candidates", "pq_candidates", "hybrid_alpha", "group_by", "min_score", "boost_weight", "per_query"),
         "a graph index: call build_graph() first", "the BM25 keyword search has no graph", "the graph search",
         "graph.check_query_args", counter="graph_scored"),
    Mode("pq_candidates", ("nprobe", "binary_candidates", "hybrid_alpha", "group_by", "min_score", "boost_weight", "per_query"),
         "a PQ index: call build_pq() first", "the BM25 keyword search has no PQ codes", "the code scan",
         "pq.check_args", boosted="product-quantised", counter="pq_count"),
    Mode("boost_weight", ("hybrid_alpha", "group_by", "min_score", "nprobe", "binary_candidates", "pq_candidates", "per_query"),
         "a prior: call set_boost() first", "the fusion ranks by its own score", "the boosted search",
         "boost.check_args", reads_every_row=True),
    Mode("binary_candidates", ("nprobe", "pq_candidates", "hybrid_alpha", "group_by", "min_score", "per_query"),
         "a binary index: call build_binary() first", "the BM25 keyword search has no binary codes", "the Hamming scan",
         "binary.check_args", boosted="binary-code", counter="binary_count"),
    Mode("nprobe", ("per_query", "hybrid_alpha", "group_by", "min_score"),
         "an IVF index: call build_ivf(n_lists) first", "the BM25 keyword search has no inverted lists of topics", "the IVF search",
         "ivf.check_probe_args", boosted="IVF", counter="ivf_scanned"),
)}
ORDER = tuple(MODES)                # the order `query` and `retrieve` ask the modes in


def check_mode(name: str, value, *, has_index: bool, others=None, per_query: bool = False, hybrid_alpha=None, group_by=None, min_score=None,
               world: int = 1, n_width: int = 1, let_through=(), **own):
    """The refusals of the mode `name` given `value`, each a ValueError naming the part, before any launch -> what its `check`
    returns.  `others`: {mode name: its argument or None}; `n_width`: the rows the search returns per query (the reranker's or MMR's
    candidates, else n_results); `let_through`: parts not refused here although `order` names them; `own`: further arguments of
    the mode's `check`."""
    mode = MODES[name]
    module, function = mode.check.split(".")
    check = getattr(import_module(f"{__package__}.{module}"), function)      # (a query without the mode never imports its module)
    on = {**{m: v is not None for m, v in (others or {}).items()}, "per_query": per_query, "hybrid_alpha": hybrid_alpha is not None,
          "group_by": bool(group_by), "min_score": min_score is not None}
    for part in mode.order:
        if on.get(part) and part not in let_through:
            raise ValueError(f"{name} cannot be combined with {PARTS.get(part, part)}: {mode.why(part)}")
    if world > 1:
        raise ValueError(f"{name} needs world == 1: more than one rank is out of scope")
    if not has_index:
        raise ValueError(f"{name} needs {mode.needs}")
    return check(n_width, value, **own)


def check_modes(given: Dict, own: Dict[str, Dict], **context):
    """Every mode of `given` ({mode name: its argument or None}) that is on, in `ORDER`, through `check_mode` -> the boost's weights as
    float32 [n_queries], or None without `boost_weight`.  `context`: the arguments of `check_mode` every mode shares; `own[name]`: the
    mode's own (`has_index` among them), which win over `context`."""
    checked = {name: check_mode(name, given[name], others=given, **{**context, **own[name]}) for name in ORDER if given.get(name) is not None}
    return checked.get("boost_weight")
