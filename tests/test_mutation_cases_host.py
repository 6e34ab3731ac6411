"""The lifecycles of tests/mutation_cases.py on the CPU: the host model against the collection's own host bookkeeping
(`mutation.old_to_new`, `compact_pieces`, `word_rank_host`, `grouping.continue_runs` / `runs_from_keys`) at every step, and the states
each sequence must reach, asserted as conditions: an edit of a generator that stops reaching one fails here, without a GPU.

The numbered states (tests/test_gpu_collection_lifecycle.py replays the same sequences on the device):
 1 add between delete and compact            2 a second compaction, and an add on top of the spare buffer's stale rows
 3 hybrid search under pending tombstones    4 where_on_device / hybrid_on_device on a mutable collection   (3, 4: the GPU test's parameters)
 5 structured deletions: a whole paper, aligned 64-row words, the first rows, the last rows, every row but one, rows without text
 6 a withdrawn paper's key: refused while tombstoned, free after compact         7 an id deleted and added again, before and after compact
 8 zero rows, and an add into them           9 the text blob reallocated after a compaction swapped it
10 a delete that selects nothing, or only deleted rows                           11 compact right after add, nothing tombstoned"""
import numpy as np
import pytest

from tests import mutation_cases as MC

_WORLDS = {}


def _world(seed=1, dim=128):
    if (seed, dim) not in _WORLDS:
        _WORLDS[(seed, dim)] = MC.world(seed, dim=dim)
    return _WORLDS[(seed, dim)]


def _steps(name):
    w = _world()
    return w, (MC.scripted_lifecycle(w) if name == "scripted" else MC.random_lifecycle(w, name))


def test_the_world_has_the_shapes_the_lifecycles_need():
    w = _world()
    lens = np.diff(w["starts"])
    assert w["n"] == MC.N_POOL == len(w["meta"]) == int(lens.sum()) and lens.min() >= 1
    assert lens[1] == 70 and lens.max() == 70 and (lens == 70).sum() == 1          # one run longer than a 64-row word, and only one
    assert w["starts"][1] < 64 < w["starts"][2]                                    # ... which crosses a word boundary
    texts = [m["text"] for m in w["meta"]]
    assert all(t == "" for t, p in zip(texts, w["paper_of"]) if p == 4) and 20 < sum(t == "" for t in texts) < 100
    assert w["emb"].shape == (MC.N_POOL, 128) and np.array_equal(w["emb"], w["emb"].astype(np.float16).astype(np.float32))
    assert len({m["chunk_id"] for m in w["meta"]}) == w["n"] and _world(1, 64)["emb"].shape[1] == 64
    assert [m["text"] for m in _world(1, 64)["meta"]] == texts                     # the dim changes the embeddings only


@pytest.mark.parametrize("name", ("scripted",) + MC.SEEDS)
def test_the_model_agrees_with_the_host_bookkeeping_at_every_step(name):
    from arxiv_rag_amd.grouping import continue_runs, runs_from_keys
    from arxiv_rag_amd.keyword import flatten_pieces
    from arxiv_rag_amd.mutation import append_pieces, compact_pieces, old_to_new, piece_lists, word_rank_host
    from arxiv_rag_amd.where import pack_bitmap
    w, steps = _steps(name)
    number = {t: i for i, t in enumerate(w["words"])}

    def pieces_of(metas):
        return [[number[t] for t in m["text"].split()] for m in metas]
    group_of, run_keys = runs_from_keys([m["paper_id"] for m in steps[0]["meta"]])
    flat, ptr = flatten_pieces(pieces_of(steps[0]["meta"]))
    deleted = np.zeros(len(steps[0]["meta"]), bool)
    for step, model, ret, facts in MC.replay(steps):
        keys = [m["paper_id"] for m in step.get("meta", [])]
        if step["op"] == "add" and step["raises"] is not None:
            with pytest.raises(ValueError, match=step["raises"]):
                continue_runs(group_of, run_keys, keys)
        elif step["op"] == "add":
            more, run_keys = continue_runs(group_of, run_keys, keys)
            group_of = np.concatenate([group_of, more])
            flat, ptr = append_pieces(flat, ptr, *flatten_pieces(pieces_of(step["meta"])))
            deleted = np.concatenate([deleted, np.zeros(len(keys), bool)])
        elif step["op"] == "delete":
            assert ret == len(facts["hit"]) == facts["pending"] + len(facts["hit"]) - int(deleted.sum())
            deleted[facts["hit"]] = True
        elif step["op"] == "compact":
            keep = ~deleted
            assert ret.dtype == np.int64 and np.array_equal(ret, old_to_new(keep))
            rank = word_rank_host(pack_bitmap(keep), len(keep))
            assert rank.tolist() == [int((ret[:a] >= 0).sum()) for a in range(0, len(keep), 64)] + [int(keep.sum())]
            assert facts["zero_words"] == int((np.diff(rank) == 0).sum())
            group_of, (flat, ptr), deleted = group_of[keep], compact_pieces(flat, ptr, keep), np.zeros(int(keep.sum()), bool)
        assert len(deleted) == model.n_hbm() <= w["capacity"] and deleted.tolist() == model.dead and model.count() == int((~deleted).sum())
        # the continued runs are `runs_from_keys` of the rows there are, up to renumbering, and every value still names its key
        in_hbm = [m["paper_id"] for m in model.meta]
        fresh, fresh_keys = runs_from_keys(in_hbm)
        assert np.array_equal(np.unique(group_of, return_inverse=True)[1] if len(group_of) else group_of, fresh)
        assert [run_keys[g] for g in group_of.tolist()] == in_hbm == [fresh_keys[g] for g in fresh.tolist()]
        assert model.max_run_rows() == max(np.bincount(fresh).tolist() + [1])
        assert piece_lists(flat, ptr) == pieces_of(model.meta)
        emb, meta, index_map = model.survivors()
        assert len(meta) == model.count() == len(emb) and [model.meta[r] for r in index_map] == meta
        runs_from_keys([m["paper_id"] for m in meta])              # a fresh collection over the survivors accepts their keys
        if model.n_hbm():
            rows, every = model.all_rows("alive")
            assert len(rows) == model.n_hbm() and [m["alive"] for m in every] == (~deleted).tolist() and "alive" not in model.meta[0]


def test_the_scripted_lifecycle_contains_every_state():
    w, steps = _steps("scripted")
    seen, prev, withdrawn, forgotten = set(), None, set(), set()
    for step, model, ret, facts in MC.replay(steps):
        op, accepted = step["op"], step["op"] == "add" and step["raises"] is None
        new_ids, new_keys = {m["chunk_id"] for m in step.get("meta", [])}, {m["paper_id"] for m in step.get("meta", [])}
        if accepted and facts["pending"]:
            seen.add("1 add between delete and compact")
        if op == "compact" and not facts["noop"] and facts["compactions"] >= 1:
            seen.add("2 a second compaction")
        if accepted and facts["compactions"] >= 2 and facts["n_before"] > 0:
            seen.add("2 an add on top of the spare buffer's stale rows")
        if op == "delete" and model.dead_papers() - facts["dead_papers"] and max(k for _, k, d in model.runs() if k == d) > 64:
            seen.add("5 a whole paper")
        if op == "compact" and facts["dead_papers"] and facts["max_run_after"] < facts["max_run"]:
            seen.add("5 max_run_rows shrinks at the compaction")
        if op == "compact" and facts["zero_run"] >= 2:
            seen.add("5 aligned 64-row words, several in a row")
        if op == "delete" and 0 in facts["hit"]:
            seen.add("5 the first rows")
        if op == "delete" and facts["n_before"] - 1 in facts["hit"] and len(facts["hit"]) > 1 and facts["count_after"] > 1:
            seen.add("5 the last rows")
        if op == "delete" and facts["hit"] and facts["count_after"] == 1:
            seen.add("5 every row but one")
        if op == "delete" and len(facts["hit"]) > 9 and all(model.meta[r]["text"] == "" for r in facts["hit"]):
            seen.add("5 rows without text")
        if op == "add" and not accepted and new_keys <= facts["dead_papers"]:
            seen.add("6 a tombstoned run's key is refused")
        if accepted and new_keys & withdrawn:
            seen.add("6 a withdrawn key comes back after compact")
        if accepted and new_ids & facts["dead_ids"]:
            seen.add("7 an id added again beside its tombstoned row")
        if accepted and new_ids & forgotten and not new_ids & facts["dead_ids"]:
            seen.add("7 an id added again after compact")
        if op == "compact" and facts["pending"] and facts["count_after"] == 0:
            seen.add("8 compact leaves zero rows")
        if accepted and facts["n_before"] == 0 and facts["compactions"]:
            seen.add("8 an add into zero rows")
        if accepted and facts["reallocated"] and facts["compactions"]:
            seen.add("9 the blob reallocates after a compaction")
        if op == "delete" and ret == 0 and facts["selected"] == 0:
            seen.add("10 a delete that selects nothing")
        if op == "delete" and ret == 0 and facts["selected"] > 0:
            seen.add("10 a delete that selects deleted rows only")
        if op == "compact" and facts["noop"] and prev == "add" and facts["n_before"] > 0:
            seen.add("11 compact right after add")
        if op == "compact" and not facts["noop"]:
            withdrawn |= facts["dead_papers"]
            forgotten |= facts["dead_ids"]
        prev = "add" if accepted else op
    assert sorted(seen) == sorted([
        "1 add between delete and compact", "2 a second compaction", "2 an add on top of the spare buffer's stale rows", "5 a whole paper",
        "5 max_run_rows shrinks at the compaction", "5 aligned 64-row words, several in a row", "5 the first rows", "5 the last rows",
        "5 every row but one", "5 rows without text", "6 a tombstoned run's key is refused", "6 a withdrawn key comes back after compact",
        "7 an id added again beside its tombstoned row", "7 an id added again after compact", "8 compact leaves zero rows",
        "8 an add into zero rows", "9 the blob reallocates after a compaction", "10 a delete that selects nothing",
        "10 a delete that selects deleted rows only", "11 compact right after add"])


@pytest.mark.parametrize("seed", MC.SEEDS)
def test_random_lifecycles_reach_the_states(seed):
    w, steps = _steps(seed)
    again = MC.random_lifecycle(w, seed)                          # the same seed, the same sequence
    assert [(s["op"], s.get("args"), [m["chunk_id"] for m in s.get("meta", [])]) for s in steps] == \
           [(s["op"], s.get("args"), [m["chunk_id"] for m in s.get("meta", [])]) for s in again]
    facts = [(s, f) for s, _, _, f in MC.replay(steps)][1:]
    assert len(facts) == 15
    assert sum(1 for s, f in facts if s["op"] == "compact" and f["pending"]) >= 2
    assert any(s["op"] == "add" and f["pending"] for s, f in facts)
    assert any(s["op"] == "compact" and f["zero_words"] for s, f in facts)
    assert any(s["op"] == "compact" and f["dead_papers"] for s, f in facts)
    assert sum(1 for s, f in facts if f["noop"]) <= len(facts) // 2
    assert {s["op"] for s, f in facts} == {"add", "delete", "compact"}
    assert {k for s, f in facts if s["op"] == "delete" for k in s["args"]} == {"ids", "where", "where_document"}


def test_the_gpu_cases_give_every_lifecycle_both_values_of_every_flag():
    """States 3 and 4: every lifecycle has pending tombstones at some step (above), where the GPU test runs the hybrid queries; here:
    each lifecycle meets dim 128 and 64 and both values of where_on_device, hybrid_on_device and keyword_build_on_device."""
    from tests.test_gpu_collection_lifecycle import CASES
    assert {c[0] for c in CASES} == {"scripted", *MC.SEEDS}
    for name in {c[0] for c in CASES}:
        mine = [c[1:] for c in CASES if c[0] == name]
        assert {c[0] for c in mine} == {128, 64} and all({c[j] for c in mine} == {False, True} for j in (1, 2, 3)), name
    for name in ("scripted",) + MC.SEEDS:
        assert any(f["pending"] and s["op"] != "compact" for s, _, _, f in MC.replay(_steps(name)[1]))


def test_a_withdrawn_key_is_refused_while_tombstoned_and_free_after_compact():
    from arxiv_rag_amd.grouping import continue_runs, runs_from_keys
    keys = ["a", "a", "b", "b", "b", "c"]
    group_of, run_keys = runs_from_keys(keys)
    # b's rows are tombstoned only: they are still in `group_of`, and its key is `runs_from_keys`' ValueError naming both rows
    with pytest.raises(ValueError) as e:
        continue_runs(group_of, run_keys, ["d", "b"])
    with pytest.raises(ValueError) as ref:
        runs_from_keys(keys + ["d", "b"])
    assert str(e.value) == str(ref.value) and "'b'" in str(e.value) and "row 4" in str(e.value) and "row 7" in str(e.value)
    keep = np.array([1, 1, 0, 0, 0, 1], bool)                     # the compaction removes b's run: the key is free, under a new value
    more, run_keys2 = continue_runs(group_of[keep], run_keys, ["d", "b", "b"])
    assert more.tolist() == [3, 4, 4] and run_keys == ["a", "b", "c"]
    now = np.concatenate([group_of[keep], more])
    assert [run_keys2[g] for g in now.tolist()] == ["a", "a", "c", "d", "b", "b"]
    assert run_keys2[1] == "b" and 1 not in now                   # (the old value names no row any more)
    with pytest.raises(ValueError, match="'a' appears at row 1 and again at row 6"):
        continue_runs(now, run_keys2, ["a"])
    last, _ = continue_runs(now, run_keys2, ["b", "e"])           # the last run, tombstoned or not, is continued
    assert last.tolist() == [4, 5]
