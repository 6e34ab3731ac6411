"""The score-threshold search (`ShardIndex.search_range`, csrc/range.hip) held to the repository's own definition: for sampled queries
the reference list is peeled out of `search(q, 32, allow=bitmap)` (the search's own order and score bits), and the range answer must be,
bit for bit, that list's prefix cut at the threshold and at M, with counts = the qualifying rows among its M + 1; for M <= 32 and
threshold -inf the whole batch is `search(Q, M, allow=...)`; every answer is checked against float64 with the bound B(D) of
check_topk_fp64; the scan, the exhaustive path and a candidate capacity of 1 return the same bits."""
import numpy as np
import pytest

from tests.helpers import scores_fp64
from tests.range_cases import KINDS, MASKS, check_range_fp64, expected, make_mask, peel, threshold_of, to_device, visible_rows
from tests.test_gpu_search_fp64 import _case_data, _gen, _unit

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# the smallest shapes at which it can still go wrong: M > n, one group and one row more, two pass-A tiles at BM = 256, M + 1 above the
# number of non-empty groups (t = -inf), `ties` rows (12805 = 64 * 200 + 5: the cut-back sort runs and near-ties straddle the M-th row),
# two internal query slices
CASES = [
    dict(id="range-n1", d=64, n=1, nq=3, M=1, rows="unit"),
    dict(id="range-63-M50", d=320, n=63, nq=17, M=50, rows="mixed"),
    dict(id="range-64-M32", d=768, n=64, nq=64, M=32, rows="mixed"),
    dict(id="range-65-M33", d=1024, n=65, nq=65, M=33, rows="unit", base=1 << 33),
    dict(id="range-257-M256", d=64, n=257, nq=129, M=256, rows="mixed"),
    dict(id="range-1281-M1024", d=128, n=1281, nq=300, M=1024, rows="unit"),
    dict(id="range-ties-320-M10", d=320, n=12805, nq=12, M=10, rows="ties"),
    dict(id="range-ties-320-M1024", d=320, n=12805, nq=12, M=1024, rows="ties"),
    dict(id="range-ties-64-M33", d=64, n=12805, nq=70, M=33, rows="ties", base=7),
    dict(id="range-ties-64-M1024", d=64, n=12805, nq=70, M=1024, rows="ties"),
    dict(id="range-2200-1100q", d=128, n=2200, nq=1100, M=50, rows="unit"),
]


def _same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_range_search_is_the_peeled_prefix_and_fp64_exact_on_every_path(case):
    from arxiv_rag_amd.index import ShardIndex
    c = case
    C_, Q_ = _case_data(c)
    n, nq, M, base = c["n"], c["nq"], c["M"], c.get("base", 0)
    idx = ShardIndex(C_, idx_base=base)
    e = scores_fp64(Q_, C_)
    n_groups = (n + 63) // 64
    sample = sorted({0, 1, 2, 5, nq // 2, nq - 1} & set(range(nq)))
    plain = None
    for mi, kind in enumerate(MASKS):
        what = (c["id"], kind)
        words = make_mask(kind, n, seed=mi + 1)
        allow = to_device(words)
        vis = visible_rows(words, n)
        groups_seen = len(set((np.nonzero(vis)[0] >> 6).tolist()))
        refs = {qi: peel(idx, Q_[qi:qi + 1], words, n, M + 1, base) for qi in sample}
        # two threshold vectors: -inf everywhere, and a mix of every kind across the batch
        mix = np.array([(-np.inf, 0.03125, np.inf, np.nan)[qi % 4] for qi in range(nq)], np.float32)
        for j, qi in enumerate(sample):
            mix[qi] = threshold_of(KINDS[(j + mi) % len(KINDS)], refs[qi][0], M)
        for ms in (np.full(nq, -np.inf, np.float32), mix):
            got = idx.search_range(Q_, ms, M, allow=allow)
            assert idx.range_stats()[0] == 0, (what, "a shard of at most 201 groups overflowed the default cand_cap")
            s, i, cnt = got
            for qi in sample:
                es, ei, ec = expected(refs[qi][0], refs[qi][1], ms[qi], M, base)
                assert int(cnt[qi]) == ec, (what, qi, "count", int(cnt[qi]), ec)
                assert np.array_equal(i[qi].cpu().numpy(), ei), (what, qi, "ids")
                assert np.array_equal(s[qi].cpu().numpy().view(np.int32), es.view(np.int32)), (what, qi, "score bits")
            check_range_fp64(C_, Q_, e, words, ms, M, s, i, cnt, base, what)
            for kw in (dict(path=1), dict(path=2), dict(path=1, cand_cap=1)):
                other = idx.search_range(Q_, torch.from_numpy(ms).cuda(), M, allow=allow, **kw)
                assert _same(other, got), (what, kw, "not the default path's bits")
                if kw.get("cand_cap") == 1:
                    flagged = idx.range_stats()[0]
                    live = int((ms < np.inf).sum())                          # (+inf and NaN never list a candidate)
                    # a query is flagged when it has two or more candidate groups; its answer's rows all lie in candidate groups
                    spread = 0
                    for qi in sample:
                        held = min(M, int((refs[qi][0] >= ms[qi]).sum()))
                        spread += len(set((refs[qi][1][:held] >> 6).tolist())) >= 2
                    assert spread <= flagged <= (live if groups_seen >= 2 else 0), (what, "fallback counter", flagged, spread, live)
                    if groups_seen >= 2 and np.isneginf(ms).all() and kind in ("none", "ones"):
                        assert flagged == nq, (what, "every query has min(groups, M + 1) >= 2 candidate groups", flagged)
            if np.isneginf(ms).all():
                if kind == "none":
                    plain = got
                if kind == "ones":
                    assert _same(got, plain), (what, "an all-ones bitmap is not `allow=None`")
                if M <= 32:
                    ts, ti = idx.search(Q_, M, allow=allow if allow is not None else to_device(make_mask("ones", n, 0)))
                    assert torch.equal(ti, i) and torch.equal(ts.view(torch.int32), s.view(torch.int32)), (what, "not search(Q, M, allow)")
                    assert torch.equal(cnt.long(), torch.full((nq,), min(M + 1, int(vis.sum())), device="cuda")), (what, "counts at -inf")
    assert n_groups <= 201


def test_a_query_answer_does_not_depend_on_the_batch_its_order_or_the_other_thresholds():
    from arxiv_rag_amd.index import ShardIndex
    g = _gen(77)
    n, d, M = 64 * 30 + 9, 192, 100
    C_ = _unit(n, d, g).half().contiguous()
    Q_ = _unit(40, d, g).half().contiguous()
    idx = ShardIndex(C_, idx_base=3)
    ms = torch.linspace(-0.2, 0.2, 40, device="cuda")
    whole = idx.search_range(Q_, ms, M)
    perm = torch.randperm(40, generator=g, device="cuda")
    shuffled = idx.search_range(Q_[perm].contiguous(), ms[perm].contiguous(), M)
    assert _same(tuple(t[perm] for t in whole), shuffled)
    for qi in (0, 17, 39):
        alone = idx.search_range(Q_[qi:qi + 1], float(ms[qi]), M)
        assert _same(alone, tuple(t[qi:qi + 1] for t in whole)), qi
        others = ms.clone(); others[:] = float("-inf"); others[qi] = ms[qi]
        assert _same(tuple(t[qi:qi + 1] for t in idx.search_range(Q_, others, M)), alone), qi
    assert int(whole[2].min()) <= M and int(whole[2].max()) == M + 1          # (the thresholds span complete and truncated lists)


def _golden_reranker():
    """The single-label entry of tests/golden/tiny-cross-encoder.npz as a HipCrossEncoder over a synthetic vocabulary -> (model, words)."""
    import dataclasses
    import json
    from pathlib import Path
    from arxiv_rag_amd import config as C
    from arxiv_rag_amd.rerank import HipCrossEncoder
    from arxiv_rag_amd.tokenizer import WordPieceTokenizer
    from tests.cross_encoder_fp64 import golden_weights
    from tests.helpers import synthetic_vocab
    g = np.load(Path(__file__).resolve().parent / "golden" / "tiny-cross-encoder.npz")
    name = [str(n) for n in g["names"] if int(g[f"{str(n)}:n_labels"]) == 1][0]
    enc = C.EncoderConfig(**json.loads(str(g[f"{name}:cfg"])))
    sd, head = golden_weights(g, name, enc, 1)
    vocab = synthetic_vocab(dataclasses.replace(enc, vocab_size=min(enc.vocab_size, 2000)))
    tok = WordPieceTokenizer.from_vocab(vocab, enc, bert_pair=True)
    cfg = C.CrossEncoderConfig(enc, 1, C.default_activation(1))
    return HipCrossEncoder(cfg, {**sd, **head}, tok, device="cuda:0"), [w for w in vocab if w.isalpha() and len(w) > 1]


class _Spy:
    """A reranker that records what it was given."""
    def __init__(self, model):
        self.model, self.calls = model, []

    def predict(self, pairs, batch_size=32, **kw):
        self.calls.append((len(pairs), batch_size))
        return self.model.predict(pairs, batch_size=batch_size, **kw)


def test_collection_min_score_composes_with_filters_dedup_and_the_reranker():
    from arxiv_rag_amd.store import HipCollection
    rm, words = _golden_reranker()
    rs = np.random.RandomState(5)
    n, d, nq = 3000, 128, 6
    arr = rs.standard_normal((n, d)).astype(np.float32)
    arr /= np.linalg.norm(arr, axis=1, keepdims=True)
    arr[100:110] = arr[0:10]                                                 # ten exact copies of earlier rows: the dedup flags them
    meta = [{"chunk_id": f"c{r}", "paper_id": f"p{r // 7}", "section": ["intro", "method", "result"][r % 3], "quality_score": 0.9,
             "text": " ".join(words[j] for j in rs.randint(len(words), size=6))} for r in range(n)]
    col = HipCollection(arr, meta, device="cuda:0", documents=True, dedup_threshold=0.999)
    dups = set(range(100, 110))
    assert {e["index"] for e in col.duplicates} == dups
    qv = rs.standard_normal((nq, d)).astype(np.float32)
    qv /= np.linalg.norm(qv, axis=1, keepdims=True)
    q16 = torch.from_numpy(qv.astype(np.float16)).cuda()
    e = scores_fp64(q16, col.index.corpus).cpu().numpy()                      # [nq, n] float64
    ms = [float("-inf"), -0.05, 0.1, 0.2, 0.25, 2.0]
    word = words[3]

    def check(out, M, allowed, thresholds):
        assert len(out["truncated"]) == nq and all(isinstance(t, bool) for t in out["truncated"])
        for qi in range(nq):
            rows, x = out["indices"][qi], thresholds[qi]
            assert len(rows) == len(out["scores"][qi]) == len(out["ids"][qi]) == len(out["documents"][qi]) <= M
            assert not set(rows) & dups and all(allowed[r] for r in rows)
            assert all(sc >= x for sc in out["scores"][qi]) and out["scores"][qi] == sorted(out["scores"][qi], reverse=True)
            sure = {r for r in range(n) if allowed[r] and r not in dups and e[qi, r] > x + 1e-3}
            if out["truncated"][qi]:
                assert len(rows) == M and sum(1 for r in range(n) if allowed[r] and r not in dups and e[qi, r] >= x - 1e-3) > M
            else:
                assert sure <= set(rows), (qi, "a row well above the threshold is missing")
    everything = [True] * n
    out = col.query(query_embeddings=qv, min_score=ms, n_results=50)
    check(out, 50, everything, ms)
    assert out["truncated"][0] is True and len(out["indices"][0]) == 50 and out["indices"][5] == [] and out["truncated"][5] is False
    s, i, c = col.index.search_range(q16, ms, 50, allow=col._keep)
    assert out["indices"] == [[int(j) for j in row[row >= 0]] for row in i.cpu().numpy()] and out["truncated"] == (c > 50).cpu().tolist()
    lens = {len(r) for r in out["indices"]}
    assert len(lens) >= 3                                                      # natural, variable lengths
    one = col.query(query_embeddings=qv, min_score=0.1, n_results=1024)        # a single float for every query
    check(one, 1024, everything, [0.1] * nq)
    sect = [m["section"] == "method" for m in meta]
    check(col.query(query_embeddings=qv, min_score=ms, n_results=50, where={"section": "method"}), 50, sect, ms)
    has = [word in m["text"] for m in meta]
    check(col.query(query_embeddings=qv, min_score=ms, n_results=50, where_document={"$contains": word}), 50, has, ms)
    both = [a and b for a, b in zip(sect, has)]
    check(col.query(query_embeddings=qv, min_score=ms, n_results=50, where={"section": "method"}, where_document={"$contains": word}), 50,
          both, ms)
    # "re-rank top 50, return top 10": the cross-encoder receives the range list, in batches of at most 32
    qs = [" ".join(words[j] for j in rs.randint(len(words), size=4)) for _ in range(nq)]
    spy = _Spy(rm)
    cand = col.query(query_embeddings=qv, min_score=float("-inf"), n_results=50)
    rer = col.query(query_embeddings=qv, query_texts=qs, min_score=float("-inf"), n_results=10, reranker=spy, n_candidates=50)
    assert sum(c_[0] for c_ in spy.calls) == nq * 50 and all(c_[1] <= 32 for c_ in spy.calls)
    assert rer["truncated"] == [True] * nq
    for qi in range(nq):
        assert len(rer["indices"][qi]) == 10 and set(rer["indices"][qi]) <= set(cand["indices"][qi])
        sc = rm.predict([(qs[qi], meta[j]["text"]) for j in cand["indices"][qi]])
        assert rer["indices"][qi] == [cand["indices"][qi][t] for t in np.lexsort((np.arange(50), -sc))[:10]]
        assert np.allclose(rer["rerank_scores"][qi], np.sort(sc)[::-1][:10])
    # every refusal, on a real collection
    for kw, text in ((dict(hybrid_alpha=0.5, query_texts=qs), "hybrid_alpha"), (dict(mmr_lambda=0.5), "mmr_lambda"), (dict(group_by=True), "group_by"),
                     (dict(where=[{"section": "intro"}] * nq), "per-query filter lists"), (dict(n_results=1025), "n_results=1025"),
                     (dict(reranker=spy, query_texts=qs, n_candidates=1025), "n_candidates=1025")):
        with pytest.raises(ValueError) as err:
            col.query(query_embeddings=qv, min_score=0.1, **kw)
        assert text in str(err.value) and "min_score" in str(err.value), kw
    plain = col.query(query_embeddings=qv, n_results=10)                       # without min_score nothing changed
    assert "truncated" not in plain and plain["indices"] == [r[:10] for r in cand["indices"]]


def test_cli_run_with_min_score(tmp_path, monkeypatch):
    import dataclasses
    import json
    from arxiv_rag_amd import config as C, generate_embeddings_parallel as GEN
    from arxiv_rag_amd.weights import save_hf_dir, seeded_state_dict
    from tests.helpers import make_chunk_tree, synthetic_vocab
    emb_cfg = dataclasses.replace(C.TINY_BERT_CLS, vocab_size=2000, max_seq_length=64)
    vocab = synthetic_vocab(emb_cfg)
    edir = tmp_path / "emb"
    save_hf_dir(edir, emb_cfg, seeded_state_dict(emb_cfg, seed=1, std=0.05))
    (edir / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n")
    words = [w for w in vocab if w.isalpha() and len(w) > 1][:300]
    make_chunk_tree(tmp_path / "in", n_files=20, chunks_per_file=10, seed=1, words=words)
    (tmp_path / "queries.txt").write_text("\n".join(" ".join(words[i:i + 5]) for i in range(0, 40, 5)) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = [str(tmp_path / "in"), "--model", str(edir), "--min-quality", "0.0", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    results = tmp_path / "embeddings_saved" / "search_results.json"
    GEN._model, GEN._model_name = None, None
    assert GEN.main(base + ["--top-k", "32"]) == 0
    plain = json.loads(results.read_text())
    assert all("truncated" not in p for p in plain)
    GEN._model, GEN._model_name = None, None
    assert GEN.main(base + ["--top-k", "50", "--min-score=-inf"]) == 0
    wide = json.loads(results.read_text())
    for p, w in zip(plain, wide):                                              # 200 chunks: 50 of them, the first 32 the plain search's
        assert w["truncated"] is True and len(w["results"]) == 50
        assert [(h["index"], h["score"]) for h in w["results"][:32]] == [(h["index"], h["score"]) for h in p["results"]]
    cut = plain[0]["results"][4]["score"]                                      # the score of query 0's fifth hit: it is included (>=)
    GEN._model, GEN._model_name = None, None
    assert GEN.main(base + ["--top-k", "50", f"--min-score={cut!r}"]) == 0
    got = json.loads(results.read_text())
    GEN._model, GEN._model_name = None, None
    for w, r in zip(wide, got):
        want = [h for h in w["results"] if np.float32(h["score"]) >= np.float32(cut)]
        assert [(h["index"], h["score"]) for h in r["results"]] == [(h["index"], h["score"]) for h in want]
        assert len(want) == 50 or r["truncated"] is False                       # (50 of the best 50 qualify: more may, or not)
    assert len(got[0]["results"]) >= 5 and [h["index"] for h in got[0]["results"][:5]] == [h["index"] for h in plain[0]["results"][:5]]
