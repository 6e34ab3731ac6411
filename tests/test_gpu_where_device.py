"""Chroma `where` on the device (-m gpu): `arx_where_eval` against `pack_bitmap(where.evaluate(...))`, word for word, the `and_with`
bitmaps, long sets, the limits, batch independence, `HipCollection(where_on_device=True)` against the default collection, and the
refusals.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd import where_device as WD
from arxiv_rag_amd.where import compile_where, evaluate, pack_bitmap
from tests.where_device_cases import fixed_filters, make_metadata, random_filters, right_leaning

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 64 * 4 * 3 + 1, 100_003)         # one row, the word edge, the block edge (4 words), many blocks + a ragged tail
_CASES = {}


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _case(n):
    """(metadata, device columns, 64 filters, their host masks) for n rows: built once per n."""
    if n not in _CASES:
        meta = make_metadata(n, seed=100 + n % 97)
        fixed = fixed_filters()
        filters = random_filters(40, seed=n % 1000) + fixed[::len(fixed) // 23][:23] + [right_leaning(32)]
        assert len(filters) == 64
        cache = {}
        masks = np.stack([evaluate(compile_where(f), meta, cache=cache) for f in filters])
        _CASES[n] = (meta, WD.MetadataColumns(meta, 0, n, "cuda:0"), filters, masks)
    return _CASES[n]


def _prefilled(shape, byte=0xFF):
    return torch.full(tuple(shape) + (8,), byte, dtype=torch.uint8, device="cuda:0").view(torch.int64).reshape(shape)


def _run(cols, filters, and_with=None, stride=0):
    """One arx_where_eval over `filters` into buffers that held 0xFF bytes -> (uint64 [F, W], int64 [F]) on the host."""
    prog = cols.lower([compile_where(f) for f in filters])
    out, counts = _prefilled((len(filters), cols.n_words)), _prefilled((len(filters),))
    assert int(out[0, 0]) == -1 and int(counts[0]) == -1
    cols.run_program(prog, out, counts, and_with, stride)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), counts.cpu().numpy()


def _popcounts(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).sum(axis=-1)


def _assert_words(got, want, filters, n):
    if not np.array_equal(got, want):
        f, w = np.argwhere(got != want)[0]
        diff = int(got[f, w] ^ want[f, w])
        raise AssertionError(f"n={n}: filter {f} {filters[f]!r} word {w} row {int(w) * 64 + (diff & -diff).bit_length() - 1}: device "
                             f"{int(got[f, w]):#018x}, host {int(want[f, w]):#018x}; {int((got != want).sum())} words differ")


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_kernel_against_the_host_evaluator_word_for_word(hip, n):
    meta, cols, filters, masks = _case(n)
    want = np.stack([pack_bitmap(m) for m in masks])
    for picks in ([5], [63], [2, 41], list(range(64))):        # F = 1, 1, 2, 64
        got, counts = _run(cols, [filters[j] for j in picks])
        assert got.shape == (len(picks), (n + 63) // 64)
        _assert_words(got, want[picks], [filters[j] for j in picks], n)
        if n % 64:
            assert not (got[:, -1] >> np.uint64(n % 64)).any()    # the tail bits are written as zero
        assert counts.tolist() == masks[picks].sum(axis=1).tolist() == _popcounts(got).tolist()
    assert 0 < masks.sum() < masks.size


@pytest.mark.parametrize("n", (65, 64 * 4 * 3 + 1, 100_003))
def test_and_with_null_shared_and_per_filter(hip, n):
    meta, cols, filters, masks = _case(n)
    rs = np.random.RandomState(n)
    fs, ms = filters[10:17], masks[10:17]
    shared = rs.rand(n) < 0.6
    each = rs.rand(len(fs), n) < 0.5
    d_shared = torch.from_numpy(pack_bitmap(shared).view(np.int64)).cuda()
    d_each = torch.from_numpy(np.stack([pack_bitmap(m) for m in each]).view(np.int64)).cuda()
    d_shared[-1] |= -1 << (n % 64)                              # bits beyond n set in and_with (a folded `$not_contains`): still zero in the result
    for aw, stride, keep in ((None, 0, np.ones((len(fs), n), bool)), (d_shared, 0, np.broadcast_to(shared, (len(fs), n))), (d_each, cols.n_words, each)):
        got, counts = _run(cols, fs, aw, stride)
        want = ms & keep
        _assert_words(got, np.stack([pack_bitmap(m) for m in want]), fs, n)
        assert counts.tolist() == want.sum(axis=1).tolist()
    bits, counts = cols.allow_many([compile_where(f) for f in fs], d_each)      # the same through the public method
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), np.stack([pack_bitmap(m) for m in ms & each])) and counts == (ms & each).sum(axis=1).tolist()
    assert cols.paths == {"device": len(fs), "host": 0} and all(type(c) is int for c in counts)
    with pytest.raises(ValueError, match="and_with"):
        cols.allow_many([compile_where(fs[0])], d_each)         # 7 bitmaps for one filter


def test_long_sets_32_leaves_and_stack_depth_32(hip):
    n = 6_007
    rs = np.random.RandomState(5)
    meta = [{"v": int(rs.randint(20_000)), "p": f"p{int(rs.randint(9000)):05d}", "x": float(rs.randint(8))} if r % 11 else {"v": "str"} for r in range(n)]
    cols = WD.MetadataColumns(meta, 0, n, "cuda:0")
    ids = [int(v) for v in rs.choice(40_000, size=5000, replace=False)]
    papers = [f"p{int(v):05d}" for v in rs.choice(12_000, size=5000, replace=False)]
    wide = {"$or": [{"x": {"$eq": j % 8}} if j % 3 else {"v": {"$in": ids[j * 9:j * 9 + 9]}} for j in range(32)]}      # exactly 32 leaves, sets of 9
    deep = right_leaning(32, key="x")                           # stack depth exactly 32
    filters = [{"v": {"$in": ids}}, {"v": {"$nin": ids}}, {"p": {"$in": papers}}, {"$and": [{"p": {"$nin": papers}}, {"v": {"$in": ids[:9]}}]},
               {"v": {"$in": ids[:8]}}, {"v": {"$in": ids[:9] + [float("nan"), -0.0]}}, wide, deep, {"s": {"$gte": ""}}]
    prog = cols.lower([compile_where(f) for f in filters])
    assert prog.leaves["set_len"].max() == 5000 and (prog.leaf_off[7] - prog.leaf_off[6], prog.leaf_off[8] - prog.leaf_off[7]) == (32, 32)
    got, counts = _run(cols, filters)
    masks = np.stack([evaluate(compile_where(f), meta) for f in filters])
    _assert_words(got, np.stack([pack_bitmap(m) for m in masks]), filters, n)
    assert counts.tolist() == masks.sum(axis=1).tolist() and 300 < masks[0].sum() < n - 300 and masks[7].any() and not masks[7].all()
    beyond = [right_leaning(33, key="x"), filters[0], {"$or": wide["$or"] + [{"x": 1}]}]       # past the limits: the host route, same bits
    bits, cnt = cols.allow_many([compile_where(f) for f in beyond])
    assert cols.paths == {"device": 1, "host": 2}
    want = np.stack([evaluate(compile_where(f), meta) for f in beyond])
    _assert_words(bits.cpu().numpy().view(np.uint64), np.stack([pack_bitmap(m) for m in want]), beyond, n)
    assert cnt == want.sum(axis=1).tolist()


def test_a_bitmap_does_not_depend_on_the_other_filters_of_the_call_or_their_order(hip):
    n = 64 * 4 * 3 + 1
    meta, cols, filters, masks = _case(n)
    whole, counts = _run(cols, filters)
    order = np.random.RandomState(1).permutation(64)
    shuffled, counts_s = _run(cols, [filters[j] for j in order])
    assert np.array_equal(shuffled, whole[order]) and counts_s.tolist() == counts[order].tolist()
    for j in (0, 17, 40, 63):
        alone, c = _run(cols, [filters[j]])
        assert np.array_equal(alone[0], whole[j]) and c[0] == counts[j]
    bits, cnt = cols.allow_many([compile_where(f) for f in filters + filters[:6]])      # 70 filters: two calls
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), np.concatenate([whole, whole[:6]])) and cnt == counts.tolist() + counts[:6].tolist()
    assert cols.paths == {"device": 70, "host": 0}


# ---- the collection ------------------------------------------------------------------------------------------------------------------------
SECTIONS = ("abstract", "Introduction", "Methods", "Results", "Discussion")


def _corpus(n=3000, dim=128, seed=4):
    from oracle import search_oracle as SO
    rs = np.random.RandomState(seed)
    emb = SO.unit_rows_f16(n, dim, seed).astype(np.float32)
    emb[1500:1540] = emb[100:140]                               # near-duplicates for dedup_threshold
    meta = [{"chunk_id": f"c{r}", "paper_id": f"p{r // 8:05d}", "section": SECTIONS[int(rs.randint(5))], "quality_score": float(rs.rand()),
             "year": int(2000 + rs.randint(25)), "text": ("alpha " if r % 3 == 0 else "beta ") + ("lemma " if r % 5 == 0 else "graph ") + str(r)}
            for r in range(n)]
    return emb, meta


def test_collection_with_where_on_device_returns_what_the_default_collection_returns(hip):
    from arxiv_rag_amd.store import HipCollection
    from oracle import search_oracle as SO
    emb, meta = _corpus()
    kw = dict(documents=True, dedup_threshold=0.999, group_key="paper_id")
    plain, dev = HipCollection(emb, meta, **kw), HipCollection(emb, meta, where_on_device=True, **kw)
    assert plain.duplicates and plain.duplicates == dev.duplicates and dev.where_on_device and not plain.where_on_device
    q = SO.unit_rows_f16(80, 128, 21)
    one = {"$and": [{"section": {"$in": ["abstract", "Methods"]}}, {"quality_score": {"$gte": 0.3}}, {"year": {"$gte": 2005}}]}
    doc = {"$and": [{"$contains": "alpha"}, {"$not_contains": "lemma"}]}
    wheres = [None if j % 10 == 4 else ({"quality_score": {"$gte": j / 100.0}} if j % 2 else {"paper_id": {"$gte": f"p{j:05d}"}, "year": {"$ne": 2000 + j % 25}})
              for j in range(80)]
    wheres[79], wheres[78] = wheres[1], dict(reversed(list(wheres[2].items())))
    docs = [doc if j % 4 == 0 else (None if j % 4 < 3 else {"$contains": "beta"}) for j in range(80)]
    from arxiv_rag_amd.filter_sets import distinct_filters
    assert len([w for w, _ in distinct_filters(wheres, [None] * 80)[0] if w is not None]) == 70
    for kwargs in (dict(where=one), dict(where=one, where_document=doc), dict(where={"paper_id": "nope"}), dict(where=wheres),
                   dict(where=wheres, where_document=docs), dict(where=wheres, where_document=doc, n_results=5, n_candidates=20, mmr_lambda=0.5),
                   dict(where=one, group_by=True, chunks_per_group=2, n_results=6), dict(where=one, where_document=doc, group_by=True),
                   dict(where_document=doc), dict()):
        want, got = plain.query(query_embeddings=q, **kwargs), dev.query(query_embeddings=q, **kwargs)
        assert got == want, kwargs
    assert want["indices"][0] and dev._device_columns.paths["device"] >= 1 and set(dev._device_columns._dev) == {"section", "quality_score", "year", "paper_id"}
    dropped = {d["index"] for d in plain.duplicates}
    assert not dropped & {r for rows in dev.query(query_embeddings=q, where=one)["indices"] for r in rows}
    bare_p, bare_d = HipCollection(emb, meta), HipCollection(emb, meta, where_on_device=True)      # no keep-bitmap, no documents: and_with is NULL
    for kwargs in (dict(where=one), dict(where=wheres), dict(where={"section": {"$nin": list(SECTIONS)}})):
        assert bare_d.query(query_embeddings=q, **kwargs) == bare_p.query(query_embeddings=q, **kwargs), kwargs
    refusal = "where cannot be combined with hybrid_alpha: the BM25 keyword search has no row filter"
    for a, b in ((plain, dev), (bare_p, bare_d)):                 # the same refusals, the same messages
        for kwargs in (dict(where=one, hybrid_alpha=0.5, query_texts=["t"] * 80), dict(where=wheres, hybrid_alpha=0.5, query_texts=["t"] * 80),
                       dict(where={"section": {"$like": "a"}}), dict(where=wheres[:-1]), dict(where=[{"$bad": 1}] + wheres[1:])):
            said = []
            for coll in (a, b):
                with pytest.raises(ValueError) as e:
                    coll.query(query_embeddings=q, **kwargs)
                said.append(str(e.value))
            assert said[0] == said[1], kwargs
            if "hybrid_alpha" in kwargs:
                assert "hybrid_alpha" in said[1] and (a is plain or said[1] == refusal)
    with pytest.raises(ValueError, match="documents=True"):
        bare_d.query(query_embeddings=q, where=wheres, where_document=docs)


def test_each_rank_builds_columns_for_its_own_rows(hip):
    from arxiv_rag_amd.index import shard_bounds
    meta = make_metadata(5000, seed=8)
    f = [compile_where(x) for x in ({"s": {"$gte": "ab"}}, {"t": {"$in": ["b", "dé"]}, "num": {"$lt": 3}})]
    for rank in range(3):
        lo, hi = shard_bounds(5000, 3, rank)
        cols = WD.MetadataColumns(meta, lo, hi, "cuda:0")
        bits, counts = cols.allow_many(f)
        want = [evaluate(t, meta, lo, hi) for t in f]
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), np.stack([pack_bitmap(m) for m in want])) and counts == [int(m.sum()) for m in want]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip):
    n = 65
    meta, cols, filters, masks = _case(n)
    prog = cols.lower([compile_where(filters[0])])
    out, counts = _prefilled((1, cols.n_words)), _prefilled((1,))
    lib = hip.load()
    kd, vd = cols.device_column(prog.keys[0])
    table = torch.tensor([[kd.data_ptr(), vd.data_ptr()]], dtype=torch.int64, device="cuda:0")
    dummy = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    ok = dict(col_table=table.data_ptr(), n_cols=1, n_rows=n, leaves=dummy.data_ptr(), leaf_off=dummy.data_ptr(), tokens=dummy.data_ptr(),
              token_off=dummy.data_ptr(), set_vals=dummy.data_ptr(), n_set_vals=0, n_filters=1, and_with=None, and_stride=0,
              out_bits=out.data_ptr(), out_counts=counts.data_ptr(), stream=None)
    for change, part in ((dict(n_filters=0), b"n_filters=0"), (dict(n_filters=65), b"n_filters=65"), (dict(n_rows=0), b"n_rows=0"),
                         (dict(n_cols=0), b"n_cols=0"), (dict(leaves=None), b"leaves"), (dict(out_counts=None), b"out_counts"),
                         (dict(and_stride=-2), b"and_stride=-2")):
        assert lib.arx_where_eval(*{**ok, **change}.values()) == -1, change
        assert part in lib.arx_last_error(), (change, lib.arx_last_error())
    bad = WD.Program(prog.keys, prog.leaves.copy(), prog.leaf_off, prog.tokens, prog.token_off, prog.set_vals)
    bad.leaves["column"][0] = len(prog.keys)
    with pytest.raises(ValueError, match=r"leaves\[0\]\.column"):
        cols.run_program(bad, out, counts)
    torch.cuda.synchronize()
    assert (out == -1).all() and (counts == -1).all()           # nothing ran
    cols.run_program(prog, out, counts)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64)[0], pack_bitmap(masks[0])) and int(counts[0]) == int(masks[0].sum())


def test_cli_where_on_device_end_to_end(hip, tmp_path, monkeypatch):
    """The drop-in script writes the same search_results.json with and without --where-on-device, for --where-file and for --where with
    --where-document."""
    import json
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    chunks = make_chunk_tree(tmp_path / "in", n_files=30, chunks_per_file=10, seed=2, words=words)
    from collections import Counter
    common_word = Counter(w for c in chunks for w in set(c["text"].split())).most_common(1)[0][0]
    qs = [" ".join(words[i:i + 6]) for i in range(0, 24, 6)]
    (tmp_path / "queries.txt").write_text("\n".join(qs) + "\n")
    filters = [{"section": "Methods"}, None, {"quality_score": {"$gte": 0.93}}, {"section": {"$in": ["Methods", "Results"]}}]
    (tmp_path / "filters.jsonl").write_text("\n".join(json.dumps(f) for f in filters) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
              "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    results = tmp_path / "embeddings_saved" / "search_results.json"
    for extra in (["--where-file", str(tmp_path / "filters.jsonl")],
                  ["--where", json.dumps({"quality_score": {"$gte": 0.92}}), "--where-document", json.dumps({"$contains": common_word})]):
        got = []
        for flag in ([], ["--where-on-device"]):
            GEN._model, GEN._model_name = None, None
            assert GEN.main(common + extra + flag) == 0
            got.append(json.loads(results.read_text()))
        assert got[0] == got[1] and [r["query"] for r in got[1]] == qs and any(r["results"] for r in got[1]), extra
