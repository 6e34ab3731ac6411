"""Near-duplicate detection, host side (no GPU): the float64 definition of "nearest earlier row", the threshold rule and its chain
semantics, the keep-bitmap, and the CLI's argument checks."""
import argparse
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import generate_embeddings_parallel as GEN
from arxiv_rag_amd.dedup import check_threshold, duplicate_entries, duplicates_from_nearest, keep_bitmap, nearest_earlier_f64

ROOT = Path(__file__).resolve().parents[1]


def test_nearest_earlier_f64_on_a_hand_made_matrix():
    rows = np.array([[1.0, 0.0, 0.0],          # 0: nothing before it
                     [0.0, 1.0, 0.0],          # 1: only row 0 (score 0)
                     [1.0, 0.0, 0.0],          # 2: a copy of row 0
                     [0.6, 0.8, 0.0],          # 3: 0.6 with rows 0 and 2, 0.8 with row 1
                     [1.0, 0.0, 0.0],          # 4: ties rows 0 and 2 exactly -> the lower row
                     [0.0, 0.0, 1.0]])         # 5: 0 with every earlier row -> row 0
    s, i = nearest_earlier_f64(rows)
    assert i.dtype == np.int64 and s.dtype == np.float64
    assert i.tolist() == [-1, 0, 0, 1, 0, 0]
    assert s[0] == -np.inf and s[1:].tolist() == [0.0, 1.0, 0.8, 1.0, 0.0]
    # later rows never count, however close: row 1 is the nearest earlier row of row 3, not the identical row 6
    s2, i2 = nearest_earlier_f64(np.vstack([rows, rows[3:4]]))
    assert i2[3] == 1 and i2[6] == 3 and s2[6] == 1.0
    # the blocked evaluation (1 024 rows at a time) equals the plain one; small integers: every product is exact, ties abound
    x = np.random.RandomState(0).randint(-3, 4, size=(2500, 8)).astype(np.float64)
    s3, i3 = nearest_earlier_f64(x)
    full = x @ x.T
    full[np.triu_indices(2500)] = -np.inf
    assert np.array_equal(i3[1:], full[1:].argmax(1)) and np.array_equal(s3[1:], full[1:].max(1)) and i3[0] == -1
    assert (np.diff(np.sort(full[2000][:2000]))[-20:] == 0).any()      # (the ties are real)
    s0, i0 = nearest_earlier_f64(np.zeros((0, 4)))
    assert s0.shape == (0,) and i0.shape == (0,)


def test_duplicates_from_nearest_at_the_threshold():
    t = 0.95
    s = np.array([-np.inf, np.nextafter(t, 0.0), t, np.nextafter(t, 1.0), 0.2, 1.0])
    i = np.array([-1, 0, 1, 2, 3, 0])
    d = duplicates_from_nearest(s, i, t)
    assert d.dtype == np.int64 and d.tolist() == [-1, -1, 1, 2, -1, 0]
    # [n, k] inputs: column 0 is the nearest
    d2 = duplicates_from_nearest(np.stack([s, s - 1], 1), np.stack([i, i], 1), t)
    assert d2.tolist() == d.tolist()
    # float32 scores, as the device returns them
    assert duplicates_from_nearest(np.array([0.5, 0.95], np.float32), np.array([0, 0]), np.float32(0.95)).tolist() == [-1, 0]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_keep_bitmap_words(n):
    dup = np.full(n, -1, np.int64)
    words = keep_bitmap(dup)
    assert words.dtype == np.uint64 and words.shape == ((n + 63) // 64,)
    want = [(1 << min(64, n - 64 * w)) - 1 for w in range((n + 63) // 64)]
    assert [int(x) for x in words] == want
    if n > 1:
        dup[n - 1] = 0                                           # the last row is a duplicate: its bit is cleared, nothing else
        w2 = keep_bitmap(dup)
        want[(n - 1) >> 6] &= ~(1 << ((n - 1) & 63))
        assert [int(x) for x in w2] == want
    dup[0] = -1
    assert int(keep_bitmap(dup)[0]) & 1 == 1                      # row 0 has no earlier row: always kept


def test_chains_collapse_onto_earlier_rows():
    """a ~ b ~ c with a !~ c: b is flagged (onto a) and so is c (onto b, itself a duplicate); only a is kept."""
    ang = np.deg2rad([0.0, 15.0, 30.0])
    rows = np.stack([np.cos(ang), np.sin(ang)], 1)
    t = 0.95                                                      # cos 15 = 0.966 >= t > cos 30 = 0.866
    s, i = nearest_earlier_f64(rows)
    d = duplicates_from_nearest(s, i, t)
    assert d.tolist() == [-1, 0, 1]
    assert rows[0] @ rows[2] < t
    assert [int(x) for x in keep_bitmap(d)] == [1]
    ent = duplicate_entries(d, s, ["a", "b", "c"], base=10)
    assert [(e["index"], e["chunk_id"], e["duplicate_of_index"], e["duplicate_of"]) for e in ent] == [(11, "b", 10, "a"), (12, "c", 11, "b")]
    assert ent[0]["score"] == pytest.approx(np.cos(ang[1]))


def test_check_threshold():
    for ok in (1.0, 0.5, 1e-9):
        assert check_threshold(ok) == ok
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dedup_threshold"):
            check_threshold(bad)


def _args(**kw):
    base = dict(dedup_threshold=None, hybrid_alpha=None, queries=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_dedup_args(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert GEN.check_dedup_args(_args()) is None
    for ok in (1.0, 0.95, 1e-6):
        assert GEN.check_dedup_args(_args(dedup_threshold=ok)) is None
    for bad in (0.0, -0.5, 1.01, float("nan"), float("inf")):
        msg = GEN.check_dedup_args(_args(dedup_threshold=bad))
        assert msg and "--dedup-threshold" in msg, bad
    # the keyword search has no row filter: refused only where a search would run
    assert GEN.check_dedup_args(_args(dedup_threshold=0.9, hybrid_alpha=0.7)) is None
    assert GEN.check_dedup_args(_args(dedup_threshold=0.9, queries="q.txt")) is None
    msg = GEN.check_dedup_args(_args(dedup_threshold=0.9, hybrid_alpha=0.7, queries="q.txt"))
    assert msg and "--dedup-threshold" in msg and "--hybrid-alpha" in msg
    assert GEN.check_dedup_args(_args(hybrid_alpha=0.7, queries="q.txt")) is None      # without the flag nothing is checked
    monkeypatch.setenv("WORLD_SIZE", "2")
    msg = GEN.check_dedup_args(_args(dedup_threshold=0.9))
    assert msg and "--dedup-threshold" in msg and "rank" in msg
    assert GEN.check_dedup_args(_args()) is None


@pytest.mark.parametrize("extra", [["--dedup-threshold", "0"], ["--dedup-threshold", "1.5"], ["--dedup-threshold", "nan"],
                                   ["--dedup-threshold", "0.9", "--hybrid-alpha", "0.7", "--queries", "q.txt"]])
def test_main_refuses_bad_dedup_flags_with_exit_code_2(tmp_path, capsys, monkeypatch, extra):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert GEN.main([str(tmp_path / "missing")] + extra) == 2
    assert "--dedup-threshold" in capsys.readouterr().out


def test_c_abi_declares_the_prefix_search():
    hdr = (ROOT / "include" / "arx.h").read_text()
    from arxiv_rag_amd import _lib
    for name in ("arx_topk_prefix_workspace_bytes", "arx_topk_search_prefix", "arx_topk_search_prefix_tuned", "arx_topk_prefix_stats"):
        assert name + "(" in hdr, f"{name} is not declared in include/arx.h"
        assert name in _lib.EXPORTS, f"{name} has no ctypes prototype"
