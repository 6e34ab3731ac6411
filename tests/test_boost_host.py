"""Boosted search, the host side (no GPU): the exports, the numpy restatement against float64, the prior column, the refusals."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

from arxiv_rag_amd import boost as BO

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"arx_topk_search_boosted": 21, "arx_topk_search_boosted_workspace_bytes": 4, "arx_topk_boosted_stats": 4, "arx_prior_info": 4}


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
        proto = re.search(rf"^int(?:32|64)_t {name}\(([^;]*?)\);", hdr, re.S | re.M).group(1)
        assert len(proto.split(",")) == n_args, name
    ws = lib.arx_topk_search_boosted_workspace_bytes
    ws.restype, ws.argtypes = _lib.EXPORTS["arx_topk_search_boosted_workspace_bytes"]
    assert ws(1000, 70, 64, 10) > 0 and ws(1, 1, 8192, 32) > 0 and ws(1000, 5000, 64, 32) == ws(1000, 1024, 64, 32)
    bad = [ws(1000, 70, 64, 0), ws(1000, 70, 64, 33), ws(1000, 70, 96, 10), ws(1000, 70, 0, 10), ws(1000, 70, 8256, 10), ws(-1, 70, 64, 10),
           ws(0, 70, 64, 10), ws(1000, 0, 64, 10)]
    assert bad == [-1] * len(bad)
    build = (ROOT / "arxiv_rag_amd" / "csrc" / "build.sh").read_text()
    assert " boosted " in build and "$BLD/boosted.o" in build and "$f = boosted" in build      # built, linked, and without FMA contraction


def _separated(seed, n=120, nq=5, dim=64):
    """fp16 rows and queries, a prior and weights such that no two boosted scores of a query lie within 1e-5 of each other (float64)."""
    for s in range(seed, seed + 50):
        rs = np.random.RandomState(s)
        X = (rs.randn(n, dim) / np.sqrt(dim)).astype(np.float16)
        Q = (rs.randn(nq, dim) / np.sqrt(dim)).astype(np.float16)
        prior = rs.rand(n).astype(np.float32)
        w = rs.choice([0.0, 0.02, 0.2, 5.0, -0.2], nq).astype(np.float32)
        S = X.astype(np.float64) @ Q.astype(np.float64).T + prior.astype(np.float64)[:, None] * w.astype(np.float64)[None, :]
        if all(np.diff(np.sort(S[:, q])).min() > 1e-5 for q in range(nq)):
            return X, Q, prior, w, S
    raise AssertionError("no separated data found")


@pytest.mark.parametrize("k", (1, 10, 32))
def test_boosted_host_equals_a_float64_brute_force(k):
    X, Q, prior, w, S = _separated(11)
    mask = np.random.RandomState(2).rand(X.shape[0]) < 0.7
    prior = prior.copy(); prior[[3, 50]] = np.nan; prior[7] = np.inf; prior[8] = -np.inf
    for allow in (None, mask):
        vis = np.isfinite(prior) & (mask if allow is not None else True)
        s, b, i = BO.boosted_host(X, Q, prior, w, k, allow)
        for q in range(Q.shape[0]):
            rows = np.flatnonzero(vis)
            want = rows[np.argsort(-S[rows, q], kind="stable")[:k]]
            assert np.array_equal(i[q], want)
            assert np.allclose(s[q], S[want, q], rtol=0, atol=2e-6 * (1 + abs(float(w[q]))))
            assert np.allclose(b[q], (X.astype(np.float64) @ Q[q].astype(np.float64))[want], rtol=0, atol=2e-6)
            p32 = (np.float32(w[q]) * prior[want]).astype(np.float32)
            assert np.array_equal((b[q] + p32).astype(np.float32).view(np.uint32), s[q].view(np.uint32))      # two rounded operations
    s, b, i = BO.boosted_host(X[:5], Q, prior[:5], w, 10)
    assert (i[:, 4:] == -1).all() and np.isneginf(s[:, 4:]).all() and np.isneginf(b[:, 4:]).all() and (i[:, :4] >= 0).all()      # row 3 is hidden
    s, b, i = BO.boosted_host(X, Q, np.full(X.shape[0], np.nan, np.float32), w, 3)
    assert (i == -1).all() and np.isneginf(s).all() and np.isneginf(b).all()
    # weight 0: the plain order by (base desc, row asc); ties to the lower row
    X2 = X.copy(); X2[100] = X2[20]; Q2 = Q.copy(); Q2[0] = X2[20]
    eq = np.ones(X.shape[0], np.float32)
    s, b, i = BO.boosted_host(X2, Q2, eq, 0.0, 2)
    assert i[0].tolist() == [20, 100] and np.array_equal(s.view(np.uint32), b.view(np.uint32))
    eq[100] = 2.0
    assert BO.boosted_host(X2, Q2, eq, 1.0, 2)[2][0].tolist() == [100, 20]
    with pytest.raises(ValueError, match="prior"):
        BO.boosted_host(X, Q, prior[:-1], w, 3)


def test_prior_from_metadata():
    mds = [{"quality_score": 0.5, "year": 2020}, {"quality_score": 2, "year": 2024.0}, {"year": 2022}, None, {"quality_score": True, "flag": False},
           {"quality_score": None}]
    p = BO.prior_from_metadata(mds, {"key": "quality_score", "missing": -1.0})
    assert p.dtype == np.float32 and p.tolist() == [0.5, 2.0, -1.0, -1.0, 1.0, -1.0]
    assert BO.prior_from_metadata(mds, {"key": "flag"}).tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert BO.prior_from_metadata([], {"key": "x"}).shape == (0,)
    d = BO.prior_from_metadata(mds, {"key": "year", "decay": "exp", "origin": 2024, "half_life": 2.0, "missing": 0.25})
    assert np.array_equal(d, np.array([0.25, 1.0, 0.5, 0.25, 0.25, 0.25], np.float32))
    d = BO.prior_from_metadata([{"year": 2021}, {"year": 2027}], {"key": "year", "decay": "exp", "origin": 2024, "half_life": 1.5})
    assert np.array_equal(d, np.array([np.exp(-np.log(2.0) * 3 / 1.5)] * 2).astype(np.float32))
    assert np.isnan(BO.prior_from_metadata([{"v": float("nan")}], {"key": "v"})[0])
    for mds_, spec in (([{"q": "high"}], {"key": "q"}), ([{"q": "2020"}], {"key": "q", "decay": "exp", "origin": 0, "half_life": 1}),
                       ([{"q": [1]}], {"key": "q"}), (mds, {"key": "year", "decay": "exp", "origin": 2024, "half_life": 0}),
                       (mds, {"key": "year", "decay": "exp", "origin": 2024, "half_life": -1.0}), (mds, {"key": "year", "decay": "exp", "origin": 2024}),
                       (mds, {"key": "year", "decay": "linear", "origin": 2024, "half_life": 1}), (mds, {"missing": 0.0}), (mds, "year"),
                       (mds, {"key": "year", "half_life": 2.0}), (mds, {"key": "year", "scale": 2}), (mds, {"key": "year", "missing": "0"})):
        with pytest.raises(ValueError):
            BO.prior_from_metadata(mds_, spec)


def test_check_args_and_weights():
    assert BO.check_args(10, 0.5, 3).tolist() == [0.5] * 3 and BO.check_args(1, [0.0, -1.0], 2, 7.0, 64).tolist() == [0.0, -1.0]
    for kw in (dict(k=0), dict(k=33), dict(k=1.0), dict(k=True), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=[1.0, 2.0]),
               dict(weight="a"), dict(weight=1e39), dict(max_abs_prior=float("inf")), dict(max_abs_prior=-1.0), dict(max_abs_prior=float("nan")),
               dict(weight=2.0, max_abs_prior=3e38), dict(dim=96), dict(dim=0), dict(dim=8256)):
        args = dict(k=10, weight=0.5, n_queries=3, max_abs_prior=1.0, dim=64); args.update(kw)
        with pytest.raises(ValueError):
            BO.check_args(**args)


def test_every_refusal_of_check_query_with_boost():
    ok = dict(has_prior=True, n_width=10, n_queries=2, max_abs_prior=1.0)
    assert BO.check_query_with_boost(0.1, **ok).tolist() == pytest.approx([0.1, 0.1])
    assert BO.check_query_with_boost([0.1, -2.0], **ok).tolist() == pytest.approx([0.1, -2.0])
    for kw, part in ((dict(hybrid_alpha=0.5), "hybrid_alpha"), (dict(group_by="paper_id"), "group_by"), (dict(min_score=0.3), "min_score"),
                     (dict(nprobe=4), "nprobe"), (dict(binary_candidates=64), "binary_candidates"), (dict(per_query_filters=True), "per-query"),
                     (dict(world=2), "world"), (dict(has_prior=False), "set_boost"), (dict(n_width=33), "k="), (dict(n_width=0), "k=")):
        with pytest.raises(ValueError, match=part):
            BO.check_query_with_boost(0.1, **{**ok, **kw})
    for weight in (float("nan"), float("-inf"), [0.1], "w"):
        with pytest.raises(ValueError, match="weight"):
            BO.check_query_with_boost(weight, **ok)
    with pytest.raises(ValueError, match="not finite"):
        BO.check_query_with_boost(3.0, **{**ok, "max_abs_prior": 2e38})


def test_the_cli_flags_and_their_refusals(monkeypatch):
    from arxiv_rag_amd import generate_embeddings_parallel as G
    p = G.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["in", "--queries", "q.txt"]
    a = p.parse_args(base + ["--boost-key", "quality_score", "--boost-weight", "0.1"])
    assert G.check_boost_args(a) is None and G.boost_spec_of(a) == {"key": "quality_score", "missing": 0.0}
    a = p.parse_args(base + ["--boost-key", "year", "--boost-weight", "-2", "--boost-decay-origin", "2024", "--boost-half-life", "3"])
    assert G.check_boost_args(a) is None
    assert G.boost_spec_of(a) == {"key": "year", "missing": 0.0, "decay": "exp", "origin": 2024.0, "half_life": 3.0}
    assert G.check_boost_args(p.parse_args(base)) is None and G.boost_spec_of(p.parse_args(base)) is None
    for extra, part in ((["--boost-key", "y"], "go together"), (["--boost-weight", "0.1"], "go together"),
                        (["--boost-half-life", "2"], "go together"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--boost-half-life", "2"], "--boost-decay-origin"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--boost-decay-origin", "1", "--boost-half-life", "0"], "--boost-half-life"),
                        (["--boost-key", "y", "--boost-weight", "inf"], "finite"), (["--boost-key", "y", "--boost-weight", "nan"], "finite"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--hybrid-alpha", "0.5"], "--hybrid-alpha"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--group-by-paper"], "--group-by-paper"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--min-score", "0.3"], "--min-score"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--ivf-lists", "64", "--nprobe", "4"], "--nprobe"),
                        (["--boost-key", "y", "--boost-weight", "0.1", "--binary-candidates", "40"], "--binary-candidates")):
        msg = G.check_boost_args(p.parse_args(base + extra))
        assert msg is not None and part in msg, (extra, msg)
    assert "--queries" in G.check_boost_args(p.parse_args(["in", "--boost-key", "y", "--boost-weight", "0.1"]))
    a = p.parse_args(base + ["--boost-key", "y", "--boost-weight", "0.1"])
    a.where_filters = [None]
    assert "--where-file" in G.check_boost_args(a)
    a.where_filters = None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU rank" in G.check_boost_args(a)
    assert G.main(base + ["--boost-key", "y"]) == 2              # refused before the input directory is looked at
