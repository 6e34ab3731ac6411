"""The numpy restatement of the nearest-centroid assign (`topics.exact_scores_host`, `assign_exact_host`), the refusals of
`topics.predict` that need no device, and the exports of `arx_cluster_assign` (no GPU; INTEGRATION.md "Topics")."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from arxiv_rag_amd import topics as T
from tests.helpers import pass_b_budget

ROOT = Path(__file__).resolve().parents[1]
NEW = {"arx_cluster_assign_workspace_bytes": 3, "arx_cluster_assign": 12, "arx_cluster_assign_tuned": 14}
DIMS = [64, 128, 768, 8192]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _data(kind, dim, n=6, C=5):
    rs = np.random.RandomState(dim + len(kind))
    if kind == "random":
        X, Cn = rs.randn(n, dim) * rs.uniform(0.25, 4, (n, 1)) / np.sqrt(dim), rs.randn(C, dim) / np.sqrt(dim)
    elif kind == "cancellation":                             # large terms of alternating sign: the sum is far below sum |x c|
        base = rs.uniform(30, 60, (1, dim)) * np.where(np.arange(dim) % 2, -1.0, 1.0)
        X, Cn = base + rs.randn(n, dim) * 1e-2, np.abs(base[:, ::-1]) + rs.randn(C, dim) * 1e-2
    else:                                                    # subnormal halves (below 2^-14) among normal ones
        X, Cn = rs.randn(n, dim) * 2.0 ** -17, rs.randn(C, dim) * 2.0 ** -16
        X[:, ::3] = rs.randn(n, len(range(0, dim, 3)))
    return X.astype(np.float16), Cn.astype(np.float16)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["random", "cancellation", "subnormal"])
def test_exact_scores_host_against_float64(kind, dim):
    """|score - x.c| <= B(D) |x| |c| with the search's pass-B budget B(D) = (D / 16 + 4) 2^-24: two chains of D / 16 rounded adds per
    lane, their sum and the three butterfly steps (the products are exact)."""
    X, Cn = _data(kind, dim)
    if kind == "subnormal":
        assert (np.abs(X[X != 0]) < 2.0 ** -14).any() and (np.abs(Cn[Cn != 0]) < 2.0 ** -14).any()
    got = T.exact_scores_host(X, Cn)
    x64, c64 = X.astype(np.float64), Cn.astype(np.float64)
    ref = x64 @ c64.T
    bound = pass_b_budget(dim) * np.linalg.norm(x64, axis=1)[:, None] * np.linalg.norm(c64, axis=1)[None, :]
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{kind} dim {dim}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert got.dtype == np.float32 and got.shape == (X.shape[0], Cn.shape[0]) and (err <= bound).all()


@pytest.mark.parametrize("dim", [64, 768])
def test_a_pair_has_the_same_bits_alone_and_in_a_batch(dim):
    X, Cn = _data("random", dim, n=9, C=70)
    whole = T.exact_scores_host(X, Cn)
    for i in (0, 4, 8):
        for c in (0, 33, 69):
            assert _bits(T.exact_scores_host(X[i:i + 1], Cn[c:c + 1]))[0, 0] == _bits(whole)[i, c]
    assert np.array_equal(_bits(T.exact_scores_host(X[3:7], Cn)), _bits(whole[3:7]))


def test_ties_go_to_the_lower_centroid():
    X, Cn = _data("random", 64, n=8, C=6)
    Cn[4] = Cn[1]                                            # a duplicate centroid never wins
    Cn[5] = Cn[0]
    labels, scores = T.assign_exact_host(X, Cn)
    sc = T.exact_scores_host(X, Cn)
    assert labels.dtype == np.int32 and scores.dtype == np.float32
    assert not np.isin(labels, [4, 5]).any() and np.array_equal(_bits(scores), _bits(sc.max(axis=1)))
    assert all((sc[i, :labels[i]] < sc[i, labels[i]]).all() for i in range(8))
    same = np.repeat(Cn[2:3], 4, axis=0)                     # all centroids identical: label 0
    assert T.assign_exact_host(X, same)[0].tolist() == [0] * 8
    zl, zs = T.assign_exact_host(np.zeros((3, 64), np.float16), Cn)   # all-zero rows: every score +0.0 (or -0.0 == +0.0): label 0
    assert zl.tolist() == [0, 0, 0] and _bits(zs).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        T.exact_scores_host(X.astype(np.float32), Cn)
    with pytest.raises(ValueError):
        T.exact_scores_host(X, Cn[:, :32])


def test_predict_refusals_that_need_no_device():
    import torch
    X = torch.zeros((4, 128), dtype=torch.float16)
    good = np.ones((3, 128), np.float32)
    with pytest.raises(ValueError, match="dense fp16 device tensor"):
        T.predict(X, good)                                   # (a host tensor: refused after everything else was checked)
    with pytest.raises(ValueError, match="dense fp16 device tensor"):
        T.predict(X.float(), good)
    with pytest.raises(ValueError, match="dim"):
        T.predict(torch.zeros((4, 96), dtype=torch.float16), np.ones((3, 96), np.float32))
    with pytest.raises(ValueError, match="shape"):
        T.predict(X, np.ones((3, 64), np.float32))
    with pytest.raises(ValueError, match="shape"):
        T.predict(X, np.ones(128, np.float32))
    with pytest.raises(ValueError, match="f32 or fp16"):
        T.predict(X, np.ones((3, 128), np.float64))
    with pytest.raises(ValueError, match="f32 or fp16"):
        T.predict(X, torch.ones((3, 128), dtype=torch.int32))
    with pytest.raises(ValueError, match="n_clusters"):
        T.predict(X, np.ones((4097, 128), np.float16))
    with pytest.raises(ValueError, match="n_clusters"):
        T.predict(X, np.ones((0, 128), np.float32))
    bad = good.copy()
    bad[1, 5] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        T.predict(X, bad)
    with pytest.raises(ValueError, match="not finite"):
        T.predict(X, torch.full((2, 128), float("nan")))
    for nb in (0.0, -1.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="norm_bound"):
            T.predict(X, good, norm_bound=nb)
    with pytest.raises(ValueError, match="'kernel' or 'search'"):
        T.assign(X, X, how="eager")


def test_the_exports_are_in_the_header_the_library_and_the_bindings():
    from arxiv_rag_amd import _lib
    hdr = (ROOT / "include" / "arx.h").read_text()
    declared = set(re.findall(r"\b(arx_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert len(_lib.EXPORTS[name][1]) == n_args, name
    ws = lib.arx_cluster_assign_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert ws(0, 1, 64) == 16 and ws(1, 1, 64) == 32 and ws(1000, 4096, 8192) == 16 + 4000
    assert [ws(10, 8, 96), ws(10, 0, 64), ws(10, 4097, 64), ws(-1, 8, 64), ws(1 << 31, 8, 64), ws(10, 8, 8256)] == [-1] * 6
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert "cluster_assign" in build
    # one definition of the score: the kernel file and the search both include it, neither writes a second sum
    csrc = ROOT / "arxiv_rag_amd" / "csrc"
    assert '#include "exact_score.h"' in (csrc / "cluster_assign.hip").read_text() and '#include "exact_score.h"' in (csrc / "search_tail.h").read_text()
    assert sum(len(re.findall(r"float exact_row_score\(", p.read_text())) for p in csrc.iterdir() if p.is_file()) == 1
