"""Host side of hybrid search, no GPU: postings, impacts, statistics (also over a world-2 gloo group), fusion, query terms, CLI flags.
The reference is tests/bm25_fp64.py (plain float64 dictionaries, written independently of arxiv_rag_amd/keyword.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import config as C
from arxiv_rag_amd import keyword as KW
from arxiv_rag_amd.tokenizer import WordPieceTokenizer
from tests import bm25_fp64 as R
from tests.helpers import synthetic_vocab

ROOT = Path(__file__).resolve().parents[1]
V = 97


def corpus():
    """Random corpus with repeated terms, empty documents, term 3 in every non-empty document and term 5 in none."""
    docs = R.zipf_corpus(211, V, 23, seed=11, empty_every=17)
    docs = [[t if t != 5 else 6 for t in d] + ([3, 3] if d else []) for d in docs]
    assert any(not d for d in docs) and all(5 not in d for d in docs)
    return docs


# ---- postings ---------------------------------------------------------------------------------------------------------------------
def test_build_postings_matches_reference():
    docs = corpus()
    term_ptr, rows, tf, dl = KW.build_postings(docs, V)
    assert term_ptr.dtype == np.int64 and rows.dtype == np.uint32 and term_ptr.shape == (V + 1,)
    assert term_ptr[0] == 0 and term_ptr[-1] == len(rows) == len(tf) and np.all(np.diff(term_ptr) >= 0)
    assert dl.tolist() == [len(d) for d in docs]
    ref = R.postings(docs)
    for t in range(V):
        a, b = term_ptr[t], term_ptr[t + 1]
        assert list(zip(rows[a:b].tolist(), tf[a:b].tolist())) == ref.get(t, []), t
        assert np.all(np.diff(rows[a:b].astype(np.int64)) > 0)                       # rows strictly ascending inside a term
    n_nonempty = sum(1 for d in docs if d)
    assert term_ptr[4] - term_ptr[3] == n_nonempty and term_ptr[6] == term_ptr[5]      # the term in every document / in none
    assert (tf[term_ptr[3]:term_ptr[4]] >= 2).all()
    N, df, total = R.statistics(docs, V)
    st = KW.KeywordStats.from_postings(term_ptr, dl)
    assert (st.N, st.df.tolist(), st.total_len) == (N, df, total)
    with pytest.raises(ValueError):
        KW.build_postings([[0, V]], V)


def test_build_postings_empty_inputs():
    term_ptr, rows, tf, dl = KW.build_postings([], V)
    assert term_ptr.tolist() == [0] * (V + 1) and len(rows) == 0 and len(dl) == 0
    term_ptr, rows, tf, dl = KW.build_postings([[], []], V)
    assert term_ptr[-1] == 0 and dl.tolist() == [0, 0]


def test_impacts_f32_within_half_ulp_of_fp64_formula():
    """The stored impact is the float64 formula rounded once to nearest: relative error <= 2^-24 (half an ulp of f32; derived)."""
    docs = corpus()
    term_ptr, rows, tf, dl = KW.build_postings(docs, V)
    st = KW.KeywordStats.from_postings(term_ptr, dl)
    w64 = KW.impacts_f64(term_ptr, rows, tf, dl, st)
    w32 = w64.astype(np.float32)
    ref = R.impacts(docs, V)
    worst = 0.0
    for t in range(V):
        for p in range(term_ptr[t], term_ptr[t + 1]):
            r = ref[t][int(rows[p])]
            assert r > 0 and w32[p] > 0
            assert abs(w64[p] - r) <= 1e-14 * r                                       # the two float64 formulas agree
            worst = max(worst, abs(float(w32[p]) - r) / r)
    print(f"worst f32 impact error {worst / 2.0 ** -24:.3f} x 2^-24")
    assert worst <= 2.0 ** -24
    # the idf is non-negative, also for the term in every document
    assert (KW.idf_f64(st) >= 0).all() and KW.idf_f64(st)[3] > 0


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def test_stats_of_two_halves_merge_to_the_whole():
    docs = corpus()
    whole = KW.KeywordStats.from_pieces(docs, V)
    a, b = KW.KeywordStats.from_pieces(docs[:90], V), KW.KeywordStats.from_pieces(docs[90:], V)
    m = a.merge(b)
    assert (m.N, m.total_len) == (whole.N, whole.total_len) and np.array_equal(m.df, whole.df) and m.avgdl == whole.avgdl
    assert (whole.N, whole.df.tolist(), whole.total_len) == R.statistics(docs, V)
    assert a.all_reduce() is a                                                         # no process group: the identity
    with pytest.raises(ValueError):
        a.merge(KW.KeywordStats(1, np.zeros(V + 1, np.int64), 1))


_WORKER = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, os.environ["ARX_ROOT"])
import torch.distributed as dist
from arxiv_rag_amd import keyword as KW
from arxiv_rag_amd.index import shard_bounds
from tests import bm25_fp64 as R
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
docs = R.zipf_corpus(211, 97, 23, seed=11, empty_every=17)
lo, hi = shard_bounds(len(docs), world, rank)
st = KW.KeywordStats.from_pieces(docs[lo:hi], 97).all_reduce(KW._host_group())
if rank == world - 1:
    print("RESULT", json.dumps([st.N, st.total_len, st.df.tolist()]))
dist.barrier()
dist.destroy_process_group()
'''


def _run_world(tmp_path, world):
    w = tmp_path / "worker.py"
    w.write_text(_WORKER)
    env = {**os.environ, "ARX_ROOT": str(ROOT), "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", f"--nproc-per-node={world}", "--master-port",
                        str(29740 + world), str(w)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0][len("RESULT "):])


def test_stats_world_size_2_gloo_equals_world_1(tmp_path):
    docs = R.zipf_corpus(211, V, 23, seed=11, empty_every=17)
    N, df, total = R.statistics(docs, V)
    assert _run_world(tmp_path, 2) == [N, total, df] == _run_world(tmp_path, 1)


# ---- fusion -----------------------------------------------------------------------------------------------------------------------
def test_fuse_hand_worked_example():
    """dense  (0.9, r4) (0.7, r1) (0.5, r9)      -> norm 1, 0.5, 0
    keyword (8.0, r1) (6.0, r7) (4.0, r4) (4.0, r2) -> norm 1, 0.5, 0, 0
    alpha = 0.7: r4 = 0.7*1 + 0.3*0 = 0.7; r1 = 0.7*0.5 + 0.3*1 = 0.65; r7 = 0.3*0.5 = 0.15; r9 = 0; r2 = 0 -> r4, r1, r7, r2, r9
    (r2 before r9: equal fused score, lower row first)."""
    ds = np.array([[0.9, 0.7, 0.5, -np.inf]], np.float32); di = np.array([[4, 1, 9, -1]])
    ks = np.array([[8.0, 6.0, 4.0, 4.0]], np.float32); ki = np.array([[1, 7, 4, 2]])
    f, i, d, k = KW.fuse(ds, di, ks, ki, 0.7, 6)
    assert i.tolist() == [[4, 1, 7, 2, 9, -1]]
    np.testing.assert_allclose(f[0, :5], [0.7, 0.65, 0.15, 0.0, 0.0], rtol=0, atol=1e-7)     # (0.9, 0.7, 0.5 are f32 values: (0.7f-0.5f)/(0.9f-0.5f) is 0.5 to 1e-7)
    assert f[0, 5] == -np.inf
    assert d[0, 0] == np.float32(0.9) and d[0, 1] == np.float32(0.7) and np.isnan(d[0, 2]) and np.isnan(d[0, 3]) and d[0, 4] == np.float32(0.5)
    assert k[0].tolist()[:4] == [4.0, 8.0, 6.0, 4.0] and np.isnan(k[0, 4]) and np.isnan(k[0, 5])
    ref = R.fuse([(np.float32(0.9), 4), (np.float32(0.7), 1), (np.float32(0.5), 9)], [(8.0, 1), (6.0, 7), (4.0, 4), (4.0, 2)], 0.7, 6)
    assert [r for _, r in ref] == [4, 1, 7, 2, 9] and [x for x, _ in ref] == f[0, :5].tolist()


def test_fuse_flat_lists_ties_and_extremes():
    # max == min: every member of that list gets 1
    ds = np.array([[0.5, 0.5, 0.5]], np.float32); di = np.array([[7, 3, 5]])
    ks = np.array([[2.0, -np.inf, -np.inf]], np.float32); ki = np.array([[5, -1, -1]])
    f, i, _, _ = KW.fuse(ds, di, ks, ki, 0.6, 3)
    assert i.tolist() == [[5, 3, 7]] and f.tolist() == [[1.0, 0.6, 0.6]]                  # row 5 is in both lists; 3 before 7 on the tie
    # an empty keyword list and an empty dense list
    f, i, _, _ = KW.fuse(ds, di, np.full((1, 3), -np.inf, np.float32), np.full((1, 3), -1), 0.6, 2)
    assert i.tolist() == [[3, 5]] and f.tolist() == [[0.6, 0.6]]
    f, i, d, k = KW.fuse(np.full((1, 2), -np.inf, np.float32), np.full((1, 2), -1), np.full((1, 2), -np.inf, np.float32), np.full((1, 2), -1), 0.6, 2)
    assert i.tolist() == [[-1, -1]] and np.isinf(f).all() and np.isnan(d).all() and np.isnan(k).all()
    # alpha = 1 gives the dense order and alpha = 0 the keyword order for k < n on lists with distinct scores
    rs = np.random.RandomState(3)
    n, k_ = 12, 5
    ds = np.sort(rs.rand(4, n).astype(np.float32))[:, ::-1].copy(); ks = np.sort((rs.rand(4, n) * 9).astype(np.float32))[:, ::-1].copy()
    di = np.stack([rs.choice(40, n, replace=False) for _ in range(4)]); ki = np.stack([rs.choice(40, n, replace=False) for _ in range(4)])
    assert all(len(set(r.tolist())) == n for r in ds) and all(len(set(r.tolist())) == n for r in ks)
    assert KW.fuse(ds, di, ks, ki, 1.0, k_)[1].tolist() == di[:, :k_].tolist()
    assert KW.fuse(ds, di, ks, ki, 0.0, k_)[1].tolist() == ki[:, :k_].tolist()
    # and any alpha equals the reference
    for q in range(4):
        ref = R.fuse(list(zip(ds[q], di[q].tolist())), list(zip(ks[q], ki[q].tolist())), 0.7, n)
        f, i, _, _ = KW.fuse(ds[q], di[q], ks[q], ki[q], 0.7, n)
        assert i[0].tolist() == [r for _, r in ref] and f[0].tolist() == [x for x, _ in ref]
    with pytest.raises(ValueError):
        KW.fuse(ds, di, ks, ki, 1.5, 3)


# ---- query terms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.TINY_MPNET, C.TINY_BERT])
def test_query_term_extraction(cfg):
    vocab = synthetic_vocab(cfg)
    tok = WordPieceTokenizer.from_vocab(vocab, cfg)
    words = [w for w in vocab if w.isalpha() and len(w) > 1]
    sp = KW.special_ids(tok)
    assert sp == {vocab[t] for t in (("<s>", "</s>", "<pad>") if cfg.arch == C.ARCH_MPNET else ("[CLS]", "[SEP]", "[PAD]"))}
    q = f"{words[5]} {words[2]} {words[5]} {words[9]} {words[2]}"
    (terms,) = KW.query_terms(tok, [q])
    assert terms == sorted({vocab[words[5]], vocab[words[2]], vocab[words[9]]})          # duplicates collapse, ascending
    assert terms == R.query_terms(tok._full_pieces([q])[0], exclude=sp)
    long_q = " ".join(words + list("zyxwvutsrqponmlkjihgfedcba") + list(".,;!?-()"))      # late pieces have the LOWEST ids
    (terms,) = KW.query_terms(tok, [long_q])
    pieces = tok._full_pieces([long_q])[0]
    assert len(set(pieces)) > 64 and len(terms) == 64 and terms == sorted(terms)
    assert terms == R.query_terms(pieces, exclude=sp)                                     # the FIRST 64 distinct ones
    assert terms != sorted(set(pieces))[:64] and set(terms) == set(dict.fromkeys(pieces))  - set(list(dict.fromkeys(pieces))[64:])
    specials_text = "<s> </s> <pad> [CLS] [SEP] [PAD] " + words[1]
    (terms,) = KW.query_terms(tok, [specials_text])
    assert not (set(terms) & sp) and vocab[words[1]] in terms
    assert KW.query_terms(tok, [""]) == [[]]
    qt, qn = KW.pack_query_terms([[1, 4, 9], []], cfg.vocab_size)
    assert qt.shape == (2, 64) and qt.dtype == np.int32 and qt[0, :4].tolist() == [1, 4, 9, -1] and qn.tolist() == [3, 0]
    for bad in ([[4, 4]], [[9, 1]], [[-1]], [[cfg.vocab_size]], [list(range(65))]):
        with pytest.raises(ValueError):
            KW.pack_query_terms(bad, max(cfg.vocab_size, 70) if len(bad[0]) == 65 else cfg.vocab_size)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_hybrid_flags(tmp_path, capsys):
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    p = GEN.build_parser()
    a = p.parse_args(["in"])
    assert a.hybrid_alpha is None and GEN.check_hybrid_args(a) is None                    # default: off
    a = p.parse_args(["in", "--hybrid-alpha", "0.7"])
    assert a.hybrid_alpha == 0.7 and GEN.check_hybrid_args(a) is None
    for v in ("0", "1"):
        assert GEN.check_hybrid_args(p.parse_args(["in", "--hybrid-alpha", v])) is None
    for v in ("1.5", "-0.1", "nan"):
        assert "[0, 1]" in GEN.check_hybrid_args(p.parse_args(["in", f"--hybrid-alpha={v}"]))
        assert GEN.main([str(tmp_path), f"--hybrid-alpha={v}"]) == 2
        assert "--hybrid-alpha" in capsys.readouterr().out
    assert "--top-k" in GEN.check_hybrid_args(p.parse_args(["in", "--hybrid-alpha", "0.5", "--top-k", "33"]))
    # composes with the rerank flags, whose own checks still apply
    a = p.parse_args(["in", "--hybrid-alpha", "0.7", "--rerank-model", "m", "--rerank-top-k", "16"])
    assert GEN.check_rerank_args(a) is None and GEN.check_hybrid_args(a) is None
    assert GEN.main([str(tmp_path), "--hybrid-alpha", "0.7", "--rerank-model", "m", "--rerank-top-k", "64"]) == 2
