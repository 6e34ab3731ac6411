"""Whole lifecycles of a mutable `HipCollection` (`capacity=...`; INTEGRATION.md "Adding and deleting rows") and a host model of them:
the world the rows come from, `Model` (plain Python and numpy: an ordered list of rows with a tombstone flag each), a scripted
sequence of operations that reaches every state the collection's structures could fall out of step in, and seeded random ones.
No tests in here: tests/test_mutation_cases_host.py checks the model and what the sequences reach on the CPU,
tests/test_gpu_collection_lifecycle.py replays them on the device.  The model's filters are the host references (`where.evaluate`,
Python's `in`), never the collection under test."""
import dataclasses
import itertools

import numpy as np

from arxiv_rag_amd import config as C
from tests.helpers import synthetic_vocab

SECTIONS = ("abstract", "Introduction", "Methods", "Results")
NQ = 8
N_POOL, CAPACITY = 1300, 1100                                   # rows a world offers over a collection's life; the collection's capacity
RUN_LENGTHS = (1, 2, 3, 5, 8, 13, 21, 34)                       # rows per paper, drawn; and, fixed, the first papers:
FIRST_RUNS = (5, 70, 3, 1, 9)                                   # paper 1 is the one run longer than a 64-row word; paper 4 has no texts
LONG_FROM = 1000                                                # pool rows from here on hold long texts: they outgrow the text blob
SEEDS = (32, 50)                                                # of `random_lifecycle`, chosen so that the conditions of
                                                                # test_mutation_cases_host.py::test_random_lifecycles_reach_the_states hold


def world(seed, n=N_POOL, dim=128):
    """The rows a lifecycle draws from, in order (`emb` f32 [n, dim] of fp16 values, `meta` dicts with `chunk_id`, `text`, `paper_id`
    in runs, `section`, `year`, `quality_score`), the papers' first rows (`starts`, with n at the end) and a few queries."""
    from oracle import search_oracle as SO
    cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(cfg)
    words = [t for t in vocab if t.isalpha() and len(t) > 1][:120]
    rs = np.random.RandomState(seed)
    lens = list(FIRST_RUNS)
    while sum(lens) < n:
        lens.append(int(rs.choice(RUN_LENGTHS, p=(.1, .1, .15, .2, .2, .12, .08, .05))))
    lens[-1] -= sum(lens) - n
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    paper_of = np.repeat(np.arange(len(lens)), lens)
    texts = []
    for j in range(n):
        size = rs.randint(100, 160) if j >= LONG_FROM else rs.randint(5, 30)
        texts.append(" ".join(rs.choice(words, size=size)))
        if paper_of[j] == 4 or rs.rand() < 0.03:
            texts[j] = ""
    emb = SO.unit_rows_f16(n, dim, seed + 100).astype(np.float32)
    meta = [{"chunk_id": f"c{j}", "text": t, "paper_id": f"p{paper_of[j]:04d}", "section": SECTIONS[int(rs.randint(4))],
             "quality_score": float(rs.rand()), "year": int(1950 + rs.randint(75))} for j, t in enumerate(texts)]
    qs = [" ".join(rs.choice(words, size=4)) for _ in range(NQ)]
    Q = SO.unit_rows_f16(NQ, dim, seed + 200).astype(np.float32)
    return dict(seed=seed, n=n, dim=dim, cfg=cfg, vocab=vocab, words=words, emb=emb, meta=meta, starts=starts, paper_of=paper_of, qs=qs, Q=Q,
                capacity=CAPACITY)


def tokenizer(w):
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    if "tok" not in w:
        w["tok"] = WordPieceTokenizer.from_vocab(w["vocab"], w["cfg"])
    return w["tok"]


def cut(w, row):
    """The first paper boundary of the pool at or after `row`."""
    return int(w["starts"][np.searchsorted(w["starts"], min(row, w["n"]), side="left")])


class Model:
    """The rows in HBM in order, each `(embedding row, metadata)` with a tombstone flag.  `add`, `delete_ids`, `delete_mask` and
    `compact` return what `HipCollection`'s methods return.  `version` counts the operations that changed the survivors or their
    rows, `blob_capacity` follows the rule `DocumentStore.append` documents (at least twice the size once the capacity is used up)."""

    def __init__(self, emb, meta):
        self.emb = [np.asarray(e, np.float32) for e in emb]
        self.meta = [dict(m) for m in meta]
        self.dead = [False] * len(self.meta)
        self.version, self.compactions, self.reallocations = 0, 0, 0
        self.blob_capacity = max(16, self.n_bytes())

    # ---- what the collection is asked for ----
    def add(self, emb, meta):
        assert len(emb) == len(meta)
        live = {m["chunk_id"] for m, d in zip(self.meta, self.dead) if not d}
        assert not live & {m["chunk_id"] for m in meta}, "the model is only given ids the collection accepts"
        self.emb += [np.asarray(e, np.float32) for e in emb]
        self.meta += [dict(m) for m in meta]
        self.dead += [False] * len(meta)
        if len(meta):
            self.version += 1
            if self.n_bytes() > self.blob_capacity:
                self.blob_capacity, self.reallocations = max(self.n_bytes(), 2 * self.blob_capacity), self.reallocations + 1

    def delete_mask(self, mask):
        hit = [bool(x) and not d for x, d in zip(mask, self.dead)]
        assert len(mask) == len(self.dead)
        self.dead = [d or h for d, h in zip(self.dead, hit)]
        self.version += 1 if any(hit) else 0
        return sum(hit)

    def delete_ids(self, ids):
        rows = self.rows_of(ids)
        return self.delete_mask([r in set(rows) for r in range(len(self.dead))])

    def compact(self):
        keep = [not d for d in self.dead]
        mapping = np.full(len(keep), -1, np.int64)
        mapping[np.nonzero(keep)[0]] = np.arange(sum(keep))
        if not all(keep):
            self.emb = [e for e, k in zip(self.emb, keep) if k]
            self.meta = [m for m, k in zip(self.meta, keep) if k]
            self.dead = [False] * len(self.meta)
            self.version, self.compactions = self.version + 1, self.compactions + 1
        return mapping

    # ---- the host reference filters ----
    def where_mask(self, where):
        from arxiv_rag_amd.where import compile_where, evaluate
        return evaluate(compile_where(where), list(self.meta), cache={}) if self.meta else np.zeros(0, bool)

    def contains_mask(self, s):
        return np.array([s in m["text"] for m in self.meta], bool)

    # ---- what the states are compared with ----
    def rows_of(self, ids):
        at = {m["chunk_id"]: r for r, (m, d) in enumerate(zip(self.meta, self.dead)) if not d}
        return [at[i] for i in ids]                              # (KeyError: an id the collection has forgotten)

    def n_hbm(self):
        return len(self.meta)

    def n_dead(self):
        return sum(self.dead)

    def count(self):
        return len(self.meta) - sum(self.dead)

    def n_bytes(self):
        return sum(len(m["text"].encode("utf-8")) for m in self.meta)

    def survivors(self):
        """-> (emb f32 [count, dim], meta, index_map): the rows a fresh collection is built from, and their current rows."""
        rows = [r for r, d in enumerate(self.dead) if not d]
        dim = self.emb[0].shape[0] if self.emb else 0
        emb = np.stack([self.emb[r] for r in rows]) if rows else np.zeros((0, dim), np.float32)
        return emb, [self.meta[r] for r in rows], np.asarray(rows, np.int64)

    def all_rows(self, alive_key):
        """-> (emb, meta) of every row in HBM in order, each dict copied with a bool `alive_key`."""
        return np.stack(self.emb), [dict(m, **{alive_key: not d}) for m, d in zip(self.meta, self.dead)]

    def runs(self):
        """(paper key, rows, tombstoned rows) of every run of consecutive equal keys in HBM."""
        out, r = [], 0
        for key, grp in itertools.groupby(m["paper_id"] for m in self.meta):
            k = len(list(grp))
            out.append((key, k, sum(self.dead[r:r + k])))
            r += k
        return out

    def max_run_rows(self):
        """What `ShardIndex.set_groups` measures: the longest run in HBM, tombstoned rows included; 1 for an empty shard."""
        return max([k for _, k, _ in self.runs()] + [1])

    def dead_papers(self):
        """The keys of the papers in HBM whose rows are all tombstoned."""
        gone = {key for key, k, d in self.runs() if d == k}
        return gone - {key for key, k, d in self.runs() if d < k}

    def zero_words(self):
        """The 64-row keep-words without a surviving row."""
        return sum(1 for a in range(0, len(self.dead), 64) if all(self.dead[a:a + 64]))

    def zero_run(self):
        """The most such words in a row."""
        flags = [all(self.dead[a:a + 64]) for a in range(0, len(self.dead), 64)]
        return max([len(list(g)) for z, g in itertools.groupby(flags) if z] + [0])

    def live_ids(self, positions):
        return [self.meta[r]["chunk_id"] for r in positions if not self.dead[r]]


# ---- operations ----------------------------------------------------------------------------------------------------------------------
# {"op": "build" | "add", "emb": f32 [m, dim], "meta": [...], "raises": None or a regex of the ValueError (nothing is added then)}
# {"op": "delete", "args": the keywords of `HipCollection.delete`};  {"op": "compact"};  "note": the state the step is there for
def _rows(w, a, b, op="add", note=""):
    return {"op": op, "emb": w["emb"][a:b], "meta": w["meta"][a:b], "raises": None, "note": note}


def _delete(note="", **args):
    return {"op": "delete", "args": args, "note": note}


def selection(model, args):
    """bool [rows in HBM]: the rows a delete's arguments select, tombstoned ones included."""
    mask = np.ones(model.n_hbm(), bool)
    if "ids" in args:
        mask &= np.isin(np.arange(model.n_hbm()), model.rows_of(args["ids"]))
    if "where" in args:
        mask &= model.where_mask(args["where"])
    if "where_document" in args:
        mask &= model.contains_mask(args["where_document"]["$contains"])
    return mask


def apply(model, step):
    """One step on the model -> what the collection's method must return (None for add; for a refused add nothing changes)."""
    if step["op"] == "add":
        if step["raises"] is None:
            model.add(step["emb"], step["meta"])
        return None
    if step["op"] == "compact":
        return model.compact()
    return model.delete_mask(selection(model, step["args"]).tolist())


def replay(steps):
    """The steps one by one on a fresh model -> (step, model after it, what the step returns, facts about the state it met).  `facts`:
    before the step `pending` (tombstoned rows), `dead_ids` (their ids), `zero_words` and `zero_run` (64-row keep-words without a
    survivor, and the most of them in a row), `dead_papers`, `max_run`, `compactions`, `n_before`; of the step `noop`, `selected` (rows
    a delete's arguments select, tombstoned ones included), `hit` (the rows it tombstoned), `reallocated` (the text blob grew by
    reallocation); after it `max_run_after`, `count_after`."""
    assert steps[0]["op"] == "build"
    model = Model(steps[0]["emb"], steps[0]["meta"])
    yield steps[0], model, None, dict(pending=0, dead_ids=set(), noop=False, zero_words=0, zero_run=0, dead_papers=set(), max_run=0,
                                      max_run_after=model.max_run_rows(), reallocated=False, compactions=0, n_before=0, selected=0, hit=[],
                                      count_after=model.count())
    for step in steps[1:]:
        facts = dict(pending=model.n_dead(), dead_ids={m["chunk_id"] for m, d in zip(model.meta, model.dead) if d},
                     zero_words=model.zero_words(), zero_run=model.zero_run(), dead_papers=model.dead_papers(), max_run=model.max_run_rows(),
                     compactions=model.compactions, n_before=model.n_hbm(),
                     selected=int(selection(model, step["args"]).sum()) if step["op"] == "delete" else 0)
        version, grown, dead = model.version, model.reallocations, list(model.dead)
        ret = apply(model, step)
        facts.update(noop=model.version == version, reallocated=model.reallocations > grown, max_run_after=model.max_run_rows(),
                     count_after=model.count(),
                     hit=[r for r, (a, b) in enumerate(zip(dead, model.dead)) if b and not a] if step["op"] == "delete" else [])
        yield step, model, ret, facts


def scripted_lifecycle(w):
    """A fixed sequence that reaches, in an order that makes each reachable: an add between delete and compact; a second (and third)
    compaction into the spare buffer and an add on top of its stale rows; structured deletions (a whole paper, two aligned 64-row
    words, the first rows, the last rows, the rows without text, every row but one); a withdrawn paper's key refused while its run
    is tombstoned and accepted after the compaction; an id deleted and added again before and after a compaction; the text blob
    reallocated after a compaction swapped it; deletes that select nothing; a compaction with nothing to do; zero rows, and an add
    into them."""
    meta, emb = w["meta"], w["emb"]
    paper1 = [m["chunk_id"] for m in meta if m["paper_id"] == "p0001"]
    a = next(int(s) + 1 for s, e in zip(w["starts"][:-1], w["starts"][1:]) if s >= 300 and e - s >= 2)     # inside a paper
    b, c, d = cut(w, 800), cut(w, LONG_FROM), cut(w, 1170)
    steps = [_rows(w, 0, a, "build"), _rows(w, a, b, note="the first new row continues the last run")]
    m = Model(emb[:b], meta[:b])

    def then(step):
        steps.append(step)
        return apply(m, step)
    then(_delete("a whole paper, longer than a 64-row word", ids=paper1))
    then(_delete("two aligned 64-row words", ids=m.live_ids(range(256, 384))))
    then(_delete("the first rows", ids=m.live_ids(range(3))))
    then(_rows(w, b, c, note="add between delete and compact"))
    then(_delete("the last rows", ids=m.live_ids(range(m.n_hbm() - 30, m.n_hbm()))))
    then(_delete("by where", where={"year": {"$lt": 1958}}))
    then(_delete("by where_document", where_document={"$contains": w["words"][5]}))
    then(_delete("the rows without text", ids=[x["chunk_id"] for x, dead in zip(m.meta, m.dead) if not dead and x["text"] == ""]))
    steps.append({"op": "add", "emb": emb[5:6], "meta": [dict(meta[5], chunk_id="refused")], "note": "the key of a tombstoned run",
                  "raises": "group key 'p0001' appears at row 74 and again at row %d after its run ended" % m.n_hbm()})
    then(_delete("only rows that are deleted already", where={"year": {"$lt": 1958}}))
    then({"op": "compact", "note": "first compaction"})
    back = [dict(meta[r], chunk_id=f"again{r}") for r in range(5, 10)]
    then({"op": "add", "emb": emb[5:10], "meta": back, "raises": None, "note": "the withdrawn paper's key comes back"})
    then({"op": "compact", "note": "right after add, nothing tombstoned"})
    x = m.live_ids(range(7, 8))[0]
    then(_delete("an id ...", ids=[x]))
    then({"op": "add", "emb": emb[20:21], "meta": [dict(meta[20], chunk_id=x, paper_id="p-re0")], "raises": None,
          "note": "... added again in the generation of its tombstoned row"})
    then(_delete("by where_document", where_document={"$contains": w["words"][17]}))
    then({"op": "compact", "note": "second compaction: into the spare buffer"})
    then(_rows(w, c, d, note="on top of the spare buffer's stale rows; the text blob reallocates"))
    y = m.live_ids(range(100, 101))[0]
    then(_delete("an id ...", ids=[y]))
    then({"op": "compact", "note": "third compaction"})
    then({"op": "add", "emb": emb[21:22], "meta": [dict(meta[21], chunk_id=y, paper_id="p-re1")], "raises": None,
          "note": "... added again after the compaction"})
    then(_delete("selects nothing", where={"year": {"$lt": 0}}))
    then(_delete("every row but one", ids=m.live_ids(range(m.n_hbm()))[:-1]))
    then({"op": "compact", "note": "one row stays"})
    then(_delete("the last row", ids=m.live_ids(range(m.n_hbm()))))
    then({"op": "compact", "note": "zero rows"})
    then(_rows(w, d, d + 130, note="an empty collection filled by add"))
    return steps


def random_lifecycle(w, seed, steps=15):
    """A seeded sequence of `steps` operations after the build, drawn from add / delete by ids (some rows, a whole paper, an aligned
    64-row word) / delete by `where` / delete by `where_document` / compact, never beyond the capacity."""
    rs = np.random.RandomState(seed)
    pos = cut(w, 250 + int(rs.randint(100)))
    out = [_rows(w, 0, pos, "build")]
    m = Model(w["emb"][:pos], w["meta"][:pos])
    for _ in range(steps):
        kind = rs.choice(["add", "ids", "paper", "word", "where", "contains", "compact"], p=[.22, .08, .15, .12, .13, .1, .2])
        if kind == "add":
            end = min(cut(w, pos + int(rs.randint(40, 200))), w["n"])
            if end == pos or m.n_hbm() + end - pos > w["capacity"]:
                kind = "compact"
            else:
                step, pos = _rows(w, pos, end), end
        if m.n_hbm() == 0 and kind != "add":
            kind = "compact"
        if kind == "ids":
            step = _delete(ids=m.live_ids(sorted(rs.choice(m.n_hbm(), size=min(20, m.n_hbm()), replace=False).tolist())))
        elif kind == "paper":
            alive = sorted({x["paper_id"] for x, dead in zip(m.meta, m.dead) if not dead})
            key = alive[int(rs.randint(len(alive)))] if alive else None
            step = _delete(ids=[x["chunk_id"] for x, dead in zip(m.meta, m.dead) if not dead and x["paper_id"] == key])
        elif kind == "word":
            g = int(rs.randint(max(1, m.n_hbm() // 64)))
            step = _delete(ids=m.live_ids(range(64 * g, min(64 * g + 64, m.n_hbm()))))
        elif kind == "where":
            step = _delete(where={"$and": [{"year": {"$lt": int(1955 + rs.randint(25))}}, {"section": {"$ne": SECTIONS[int(rs.randint(4))]}}]})
        elif kind == "contains":
            step = _delete(where_document={"$contains": w["words"][int(rs.randint(len(w["words"])))]})
        elif kind == "compact":
            step = {"op": "compact", "note": ""}
        out.append(step)
        apply(m, step)
    return out
