"""Whole add / delete / compact lifecycles of a mutable `HipCollection` (tests/mutation_cases.py; the states they reach are asserted on
the CPU in tests/test_mutation_cases_host.py), every structure switched on.  After EVERY operation the collection M is compared with
the host model and with collections built fresh: F over the survivors (every query kind and `facets`, bit for bit, through the
survivors' index map while tombstones are pending) and, for the hybrid query under pending tombstones, R over every row still in HBM
with an `alive` flag each (INTEGRATION.md "BM25 statistics": the corpus statistics count the tombstoned rows, the lists never hold
one).  The fp16 shard, `group_of` and the text blob are read back and compared with the model directly.  No tolerances anywhere."""
import numpy as np
import pytest
import torch          # (before anything loads libarx_hip.so: the library then binds to the HIP runtime torch brought)

from tests import mutation_cases as MC
from tests.test_gpu_collection_mutation import _queries, _same

pytestmark = pytest.mark.gpu
FACET_KEYS = ["section", "year"]
FACET_WHERE = {"year": {"$gte": 1990}}
HYBRID_WHERE = {"section": {"$in": ["Methods", "Results", "abstract"]}}
_WORLDS = {}


def _world(dim):
    if dim not in _WORLDS:
        _WORLDS[dim] = MC.world(1, dim=dim)
        MC.tokenizer(_WORLDS[dim])
    return _WORLDS[dim]


def _kw(w, where_on_device=False, hybrid_on_device=False, build_on_device=False):
    return dict(device="cuda:0", keyword=True, tokenizer=w["tok"], documents=True, document_regex=True, group_key="paper_id",
                hybrid_filters=True, where_on_device=where_on_device, hybrid_on_device=hybrid_on_device,
                keyword_build_on_device=build_on_device)


def _answers(col, w):
    """Every query kind of the existing mutation test, plus `facets` on two keys with and without a `where`."""
    out = {name: col.query(query_embeddings=w["Q"], **q) for name, q in _queries(w).items()}
    out["facets"] = {"facets": [col.facets(FACET_KEYS, top=None), col.facets(FACET_KEYS, top=None, where=FACET_WHERE)]}
    return out


def _hybrids(w, on_device):
    return [dict(query_embeddings=w["Q"], query_texts=w["qs"], n_results=10, n_candidates=n, hybrid_alpha=0.7)
            for n in ((20, 100) if on_device else (20,))]


def _empty(got, what):
    """One empty list per query under every key."""
    assert got and all(v == [[] for _ in range(MC.NQ)] for v in got.values()), (what, {k: v for k, v in got.items() if any(v)})


def _check_empty(M, w, what):
    assert M.count() == 0 and M.index.n_rows == 0 and len(M.metadata) == 0 and M._keep is None and M.index._i8 is None
    for name, q in _queries(w).items():
        got = M.query(query_embeddings=w["Q"], **q)
        extra = {"min_score": {"truncated"}, "mmr": {"mmr_scores"}, "group_by": {"group_keys", "group_sizes"}}.get(name, set())
        assert set(got) == {"ids", "distances", "scores", "documents", "metadatas", "indices"} | extra, (what, name)
        if name == "min_score":
            assert got.pop("truncated") == [False] * MC.NQ       # (one bool per query, not a list)
        _empty(got, (what, name))
    for kw in (dict(), dict(where=FACET_WHERE), dict(where_document={"$contains": w["words"][7]})):
        for res in M.facets(FACET_KEYS, top=None, **kw):
            assert res == {"key": res["key"], "values": [], "counts": [], "distinct": 0, "missing": 0, "unbinned": 0, "total": 0}, (what, kw)
    for hybrid in _hybrids(w, M.hybrid_on_device):
        for kw in (dict(), dict(where=HYBRID_WHERE)):
            got = M.query(**hybrid, **kw)
            assert {"hybrid_scores", "keyword_scores"} <= set(got)
            _empty(got, (what, "hybrid", kw))
    assert M.keyword.n_rows == 0 and M.keyword.n_postings == 0 and M.documents.n_rows == 0 and M.documents.n_bytes == 0


def _check_device_state(M, model, what):
    """The structures in HBM against the model, read back whole: nothing stale below `count`, whatever the buffers held before."""
    from arxiv_rag_amd.mutation import unpack_rows
    from arxiv_rag_amd.where_document import pack_documents
    n = model.n_hbm()
    want = np.stack(model.emb).astype(np.float16) if n else np.zeros((0, M.dim), np.float16)
    assert np.array_equal(M._buf[:n].cpu().numpy().view(np.uint16), want.view(np.uint16)), (what, "the fp16 shard")
    assert M.index.corpus.shape[0] == n and (n == 0 or M.index.corpus.data_ptr() == M._buf.data_ptr())      # (torch: an empty view points nowhere)
    assert np.array_equal(M._group_buf[:n].cpu().numpy(), M._group_host) and len(M._group_host) == n, (what, "group_of")
    assert [M.group_keys[g] for g in M._group_host.tolist()] == [m["paper_id"] for m in model.meta], (what, "group_keys")
    blob, off = pack_documents([m["text"] for m in model.meta])
    assert M.documents.n_rows == n and M.documents.n_bytes == len(blob) and M.documents.blob.numel() == model.blob_capacity, (what, "texts")
    assert np.array_equal(M.documents.row_off.cpu().numpy(), off), (what, "row_off")
    assert np.array_equal(M.documents.blob[:len(blob)].cpu().numpy(), blob), (what, "the text blob")
    if model.n_dead():
        assert unpack_rows(M._keep.cpu().numpy(), n).tolist() == [not d for d in model.dead] == M._keep_mask.tolist(), (what, "the keep-bitmap")
    else:
        assert M._keep is None or unpack_rows(M._keep.cpu().numpy(), n).all(), (what, "the keep-bitmap")


def _check_counts(M, model, what):
    n = model.n_hbm()
    assert (M.count(), len(M.metadata), M.index.n_rows, M.n_total) == (model.count(), n, n, n), what
    # `ShardIndex.set_groups` measures the runs of the rows in HBM: tombstoned rows count until `compact`
    assert M.index.max_run_rows == model.max_run_rows(), what
    assert M.metadata == model.meta, what
    alive = [m["chunk_id"] for m, d in zip(model.meta, model.dead) if not d]
    ids = [alive[j] for j in sorted({0, len(alive) // 3, len(alive) - 1})] if alive else []
    rows = model.rows_of(ids)
    assert M.get(ids) == {"ids": ids, "documents": [model.meta[r]["text"] for r in rows],
                          "metadatas": [{k: model.meta[r][k] for k in ("paper_id", "section", "quality_score")} for r in rows]}, what
    gone = sorted({m["chunk_id"] for m, d in zip(model.meta, model.dead) if d} - set(alive))
    for cid in gone[:1] + ["no such id"]:
        with pytest.raises(ValueError, match=f"unknown id '{cid}'"):
            M.get([cid])
        with pytest.raises(ValueError, match=f"unknown id '{cid}'"):
            M.delete(ids=[cid])
    assert M.count() == model.count()                            # (the refused delete deleted nothing)


def _replay_on_device(w, steps, flags):
    from arxiv_rag_amd.store import HipCollection
    kw = _kw(w, **flags)
    M, fresh = None, {}                                          # `fresh`: F and R of the model's last version, and F's answers
    for at, (step, model, ret, facts) in enumerate(MC.replay(steps)):
        what = (at, step["op"], step.get("note", ""))
        if step["op"] == "build":
            M = HipCollection(step["emb"], list(step["meta"]), capacity=w["capacity"], **kw)
        elif step["op"] == "add" and step["raises"] is not None:
            with pytest.raises(ValueError, match=step["raises"]):
                M.add(step["emb"], step["meta"])
        elif step["op"] == "add":
            assert M.add(step["emb"], step["meta"]) is None
        elif step["op"] == "delete":
            assert M.delete(**step["args"]) == ret, what
        else:
            got = M.compact()
            assert got.dtype == np.int64 and np.array_equal(got, ret), what
            assert M._keep is None and M._deleted is None
        _check_counts(M, model, what)
        _check_device_state(M, model, what)
        if model.n_hbm() == 0:
            _check_empty(M, w, what)
            continue
        pending = model.n_dead() > 0
        emb, meta, index_map = model.survivors()
        if fresh.get("version") != model.version:                # a step that changed nothing meets the same F
            fresh = {"version": model.version}
            if len(meta):
                fresh["F"] = HipCollection(emb, meta, **kw)
                fresh["answers"] = _answers(fresh["F"], w)
        if len(meta):
            F = fresh["F"]
            assert F.count() == M.count()
            for name, got in _answers(M, w).items():
                _same(got, fresh["answers"][name], (what, name), index_map=index_map if pending else None)
        else:                                                    # every row tombstoned, none compacted away yet
            for name, got in _answers(M, w).items():
                if name != "facets":
                    got.pop("truncated", None)
                    _empty(got, (what, name))
        # a paper whose rows are all tombstoned is not a group any more
        grouped = M.query(query_embeddings=w["Q"], **_queries(w)["group_by"])
        named = {k for row in grouped["group_keys"] for k in row}
        assert not named & model.dead_papers(), (what, "a fully deleted paper's key in group_keys", sorted(named & model.dead_papers()))
        assert all(sum(sizes) == len(ids) for sizes, ids in zip(grouped["group_sizes"], grouped["ids"]))
        # hybrid search
        if pending:
            if "R" not in fresh:
                fresh["R"] = HipCollection(*model.all_rows("alive"), **kw)
            R = fresh["R"]
            assert R.keyword.n_rows == model.n_hbm() == M.index.n_rows
            for hybrid in _hybrids(w, flags["hybrid_on_device"]):
                got = M.query(**hybrid)
                _same(got, R.query(**hybrid, where={"alive": True}), (what, "hybrid under tombstones", hybrid["n_candidates"]))
                dead = {r for r, d in enumerate(model.dead) if d}
                assert not dead & {r for row in got["indices"] for r in row}, (what, "hybrid returned a deleted row")
                _same(M.query(**hybrid, where=HYBRID_WHERE), R.query(**hybrid, where={"$and": [HYBRID_WHERE, {"alive": True}]}),
                      (what, "hybrid under tombstones and a where", hybrid["n_candidates"]))
            assert torch.equal(M.keyword.post_w.view(torch.int32), R.keyword.post_w.view(torch.int32)), (what, "the statistics count deleted rows")
        else:
            F = fresh["F"]
            for hybrid in _hybrids(w, flags["hybrid_on_device"]):
                got = M.query(**hybrid)
                _same(got, F.query(**hybrid), (what, "hybrid", hybrid["n_candidates"]))
                assert "hybrid_scores" in got and "keyword_scores" in got
                _same(M.query(**hybrid, where=HYBRID_WHERE), F.query(**hybrid, where=HYBRID_WHERE), (what, "hybrid and a where"))
            assert torch.equal(M.keyword.post_w.view(torch.int32), F.keyword.post_w.view(torch.int32)), what     # the rebuilt index is the fresh one
            assert torch.equal(M.keyword.term_ptr, F.keyword.term_ptr) and torch.equal(M.keyword.post_row, F.keyword.post_row), what
            assert (M.index._i8 is not None) == (w["dim"] == 128), (what, "the int8 pre-filter is on for dim 128")
    return M


# each lifecycle meets both values of dim, where_on_device, hybrid_on_device and keyword_build_on_device
CASES = [("scripted", 128, False, False, False), ("scripted", 64, True, True, True),
         (MC.SEEDS[0], 128, True, False, True), (MC.SEEDS[0], 64, False, True, False),
         (MC.SEEDS[1], 128, False, True, True), (MC.SEEDS[1], 64, True, False, False)]


@pytest.mark.parametrize("lifecycle, dim, where_on_device, hybrid_on_device, build_on_device", CASES)
def test_every_step_of_a_lifecycle_answers_as_collections_built_fresh(lifecycle, dim, where_on_device, hybrid_on_device, build_on_device):
    w = _world(dim)
    steps = MC.scripted_lifecycle(w) if lifecycle == "scripted" else MC.random_lifecycle(w, lifecycle)
    _replay_on_device(w, steps, dict(where_on_device=where_on_device, hybrid_on_device=hybrid_on_device, build_on_device=build_on_device))


@pytest.mark.parametrize("start", ("deleted_and_compacted", "built_empty"))
@pytest.mark.parametrize("on_device", (False, True))
def test_the_empty_states_answer_with_empty_lists_and_can_be_filled(start, on_device):
    from arxiv_rag_amd.store import HipCollection
    w = _world(128)
    kw = _kw(w, where_on_device=on_device, hybrid_on_device=on_device, build_on_device=on_device)
    if start == "built_empty":
        M = HipCollection(np.zeros((0, 128), np.float32), [], capacity=200, **kw)
    else:
        M = HipCollection(w["emb"][:200], w["meta"][:200], capacity=200, **kw)
        assert M.delete(where={"year": {"$gte": 0}}) == 200 and M.count() == 0 and M.index.n_rows == 200
        assert M.compact().tolist() == [-1] * 200
    _check_empty(M, w, start)
    assert M.delete(where={"year": {"$gte": 0}}) == 0 and M.delete(where_document={"$contains": "a"}) == 0 and M.compact().tolist() == []
    a = MC.cut(w, 400)
    rows = slice(a, a + 130)
    M.add(w["emb"][rows], w["meta"][rows])
    F = HipCollection(w["emb"][rows], w["meta"][rows], **kw)
    assert M.count() == 130 and M.index._i8 is not None and F.index._i8 is not None and M.index.max_run_rows == F.index.max_run_rows
    want = _answers(F, w)
    for name, got in _answers(M, w).items():
        _same(got, want[name], (start, "after add", name))
    for hybrid in _hybrids(w, on_device):
        _same(M.query(**hybrid), F.query(**hybrid), (start, "hybrid after add"))
        _same(M.query(**hybrid, where=HYBRID_WHERE), F.query(**hybrid, where=HYBRID_WHERE), (start, "hybrid after add, with a where"))
    assert torch.equal(M.keyword.post_w.view(torch.int32), F.keyword.post_w.view(torch.int32)) and torch.equal(M.keyword.post_row, F.keyword.post_row)


def test_an_id_comes_back_at_once_and_a_tombstoned_papers_key_does_not():
    from arxiv_rag_amd.store import HipCollection
    w = _world(128)
    kw = _kw(w)
    n = MC.cut(w, 300)
    M = HipCollection(w["emb"][:n], w["meta"][:n], capacity=n + 10, **kw)
    old, new = w["meta"][7], dict(w["meta"][n], chunk_id="c7", paper_id="p-new", text="a text of its own")
    assert old["text"] and M.delete(ids=["c7"]) == 1
    with pytest.raises(ValueError, match="unknown id 'c7'"):
        M.get(["c7"])
    M.add(w["emb"][n:n + 1], [new])                              # accepted while the old row is only tombstoned
    assert M.count() == n and M.index.n_rows == n + 1
    assert M.get(["c7"]) == {"ids": ["c7"], "documents": [new["text"]], "metadatas": [{k: new[k] for k in ("paper_id", "section", "quality_score")}]}
    model = MC.Model(w["emb"][:n], w["meta"][:n])
    model.delete_ids(["c7"])
    model.add(w["emb"][n:n + 1], [new])
    emb, meta, index_map = model.survivors()
    F = HipCollection(emb, meta, **kw)
    want = _answers(F, w)
    for name, got in _answers(M, w).items():
        _same(got, want[name], ("c7 again", name), index_map=index_map)
        if name != "facets":
            assert all(7 not in rows for rows in got["indices"]) and all(old["text"] not in docs for docs in got["documents"])
    everything = M.query(query_embeddings=w["Q"][:1], n_results=1024, min_score=float("-inf"))
    assert everything["ids"][0].count("c7") == 1 and sorted(everything["indices"][0]) == index_map.tolist()

    # the key of a run that is tombstoned but still in HBM: refused, and nothing is added
    paper1 = [m["chunk_id"] for m in w["meta"][:n] if m["paper_id"] == "p0001" and m["chunk_id"] != "c7"]     # (c7 names the new row now)
    assert M.delete(ids=paper1) == 69 == model.delete_ids(paper1) and "p0001" in model.dead_papers()
    before = _answers(M, w)
    with pytest.raises(ValueError, match=f"group key 'p0001' appears at row 74 and again at row {n + 2} after its run ended"):
        M.add(w["emb"][n + 1:n + 3], [dict(w["meta"][n + 1], paper_id="p-other"), dict(w["meta"][n + 2], paper_id="p0001")])
    assert M.count() == n - 69 and M.index.n_rows == n + 1 and len(M.metadata) == n + 1
    for name, got in _answers(M, w).items():
        _same(got, before[name], ("after the refused add", name))
    with pytest.raises(ValueError, match=f"unknown id '{w['meta'][n + 1]['chunk_id']}'"):
        M.get([w["meta"][n + 1]["chunk_id"]])

    mapping = M.compact()
    assert np.array_equal(mapping, model.compact()) and M.count() == n - 69 == M.index.n_rows
    assert [m["chunk_id"] for m in M.metadata].count("c7") == 1 and M.get(["c7"])["documents"] == [new["text"]]
    emb, meta, _ = model.survivors()
    F = HipCollection(emb, meta, **kw)
    want = _answers(F, w)
    for name, got in _answers(M, w).items():
        _same(got, want[name], ("after compact", name))
    M.add(w["emb"][n + 2:n + 3], [dict(w["meta"][n + 2], paper_id="p0001")])      # and now the key is free again
    assert M.group_keys[int(M._group_host[-1])] == "p0001" and M.count() == n - 68
