"""The GEMM epilogues of the default (LayerNorm-fold) forward checked against float64, element by element, through the parity taps
arx_gemm_bf16_ex / arx_fold_ln (include/arx.h), which launch exactly what encoder_run launches:
  1. every epilogue mode (csrc/gemm.h, 0..6) on every shipped kernel (variants 89, 8, 9, 13, 71; 70 on its own row counts) at the encoder
     shapes of the three presets and at ragged row counts around the 8- / 16-row exchange of epilogue v3, N % 256 == 128 and == 0, odd
     numbers of k-tiles and a multi-tile-row batch: every output element inside the per-element budget of tests/helpers.py, every
     partial-statistics slab entry and final (mean, rstd) inside theirs, NaN-payload guard fills intact wherever nothing may be written;
  2. on the same data each fault of EPI_FAULTS / STAT_FAULTS, computed in float64 on the reference side, breaks the budget;
  3. bit relations: variant 9 == variant 8, a second call == the first, a row's output and statistics independent of the batch around it;
  4. the polynomial GELU swept through the real epilogue over [-12, 12] and the special values;
  5. fold_ln_kernel against float64 and the loop producer -> ln_finalize -> consumer against LN(y) W^T + b from the unfolded weights;
  6. the tap refuses what the kernels refuse.
Budgets are derived (tests/helpers.py), never measured; the printed worst / budget figures of one run are in profiles/gemm_epilogue_fp64.md."""
import ctypes

import numpy as np
import pytest

from tests.helpers import (EPI_FAULTS, GELU_POLY_BOUND, STAT_FAULTS, U8, U24, epi_fault_applies, epilogue_inputs, epilogue_ref_args,
                           fold_ln_fp64, gelu_fp64, gemm_epilogue_budget, gemm_epilogue_fp64, layer_norm_fp64, row_stats_fp64)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD_ROWS = 24
GUARD_BITS = 0x7FC1                                   # bf16 NaN with a payload: a stray store of any value changes it
GUARD_BITS32 = 0x7FC12345                             # the same for the f32 statistics buffers
TILE_VARIANTS = (89, 8, 9, 13, 71)
M_EDGE = (1, 7, 8, 9, 15, 17, 121, 129, 255, 257, 263, 264, 391, 1041)
M_SMALL = (1, 12, 16, 17, 100, 256)
ROLE_MODES = {"qkv": (0, 3), "oproj": (2, 5, 6), "fc1": (1, 4), "fc2": (2, 5, 6), "all": tuple(range(7))}


def _roles(H, F):
    return [("qkv", 3 * H, H), ("oproj", H, H), ("fc1", F, H), ("fc2", H, F)]


# group -> [(role, N, K, row counts)]: each role runs the modes the forward gives it (ROLE_MODES); the shapes no role owns run all seven
GROUPS = {
    "minilm": [(r, N, K, M_EDGE) for r, N, K in _roles(384, 1536)],                      # N % 256 == 128: 384, 1152
    "mpnet": [(r, N, K, M_EDGE) for r, N, K in _roles(768, 3072)],
    "bge-large": [(r, N, K, (9, 257, 1041)) for r, N, K in _roles(1024, 4096)],
    "odd-k-tiles": [("all", 256, 192, (17, 264, 1041)), ("all", 768, 320, (17, 264, 1041)), ("all", 384, 448, (17, 264, 1041))],
    "multi-tile-rows": [("all", 768, 768, (70001,))],       # 274 x 3 tiles: the persistent kernel walks several per block, ragged last tile row
}
SMALL_GROUPS = {       # variant 70: every (N, K) it serves; its split count varies with both the shape and the row count
    "minilm": [(r, N, K, M_SMALL) for r, N, K in _roles(384, 1536)],
    "mpnet": [(r, N, K, M_SMALL) for r, N, K in _roles(768, 3072)],
    "bge-large": [(r, N, K, M_SMALL) for r, N, K in _roles(1024, 4096)],
    "odd-k-tiles": [("all", 256, 192, M_SMALL), ("all", 768, 320, M_SMALL), ("all", 384, 448, M_SMALL)],
}


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _filled(shape, bits, dtype):
    return torch.full(shape, bits, dtype=dtype, device="cuda")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run_ex(hip, d, mode, variant, rows=None, check=True):
    """One arx_gemm_bf16_ex call on the operands of epilogue_inputs (the first `rows` rows of them) into guard-filled buffers ->
    dict(out bf16 [M, N], stats {psum, psq [N / 64, M], mean, rstd [M]} or None, guard: list of violated guards, rc)."""
    M = rows or d["M"]
    N, K = d["N"], d["K"]
    ln_in, stats = mode in (3, 4), mode in (5, 6)
    W = d["Wf"] if ln_in else d["W0"]
    buf = _filled((M + GUARD_ROWS, N), GUARD_BITS, torch.int16)
    e = hip.GemmEpilogueC(mode=mode, variant=variant, eps=d["eps"], bias=_ptr(d["c"] if ln_in else d["bias"]), resid=_ptr(d["resid"]),
                          a_mean=_ptr(d["a_mean"]), a_rstd=_ptr(d["a_rstd"]), s_vec=_ptr(d["s"]), r_mean=_ptr(d["r_mean"]),
                          r_rstd=_ptr(d["r_rstd"]), r_gamma=_ptr(d["r_gamma"]), r_beta=_ptr(d["r_beta"]), row_cap=d["row_cap"])
    keep = [buf]
    if stats:
        ld, np_ = M + 8, N // 64
        slabs = [_filled((np_ + 2, ld), GUARD_BITS32, torch.int32) for _ in range(2)]
        fin = [_filled((M + 8,), GUARD_BITS32, torch.int32) for _ in range(2)]
        n_rows = torch.tensor([M], dtype=torch.int32, device="cuda")
        e.part_sum, e.part_sq, e.part_ld = slabs[0].data_ptr(), slabs[1].data_ptr(), ld
        e.out_mean, e.out_rstd, e.n_rows = fin[0].data_ptr(), fin[1].data_ptr(), n_rows.data_ptr()
        keep += slabs + fin + [n_rows]
    rc = hip.load().arx_gemm_bf16_ex(d["A"].data_ptr(), W.data_ptr(), buf.data_ptr(), M, N, K, ctypes.byref(e),
                                     torch.cuda.current_stream().cuda_stream)
    if check:
        hip.check(rc, "arx_gemm_bf16_ex")
    torch.cuda.synchronize()
    guard = []
    if not (buf[M:] == GUARD_BITS).all().item():
        guard.append("output rows >= M")
    res = {"out": buf[:M].view(torch.bfloat16), "stats": None, "guard": guard, "rc": rc}
    if stats and rc == 0:
        if variant == 70:
            if not all((s == GUARD_BITS32).all().item() for s in slabs):
                guard.append("variant 70 wrote a slab")
        else:
            if not all((s[:, M:] == GUARD_BITS32).all().item() for s in slabs):
                guard.append("slab rows >= M")
            if not all((s[np_:] == GUARD_BITS32).all().item() for s in slabs):
                guard.append("slabs beyond N / 64")
        if not all((f[M:] == GUARD_BITS32).all().item() for f in fin):
            guard.append("out_mean / out_rstd beyond M")
        res["stats"] = {"psum": slabs[0][:np_, :M].view(torch.float32), "psq": slabs[1][:np_, :M].view(torch.float32),
                        "mean": fin[0][:M].view(torch.float32), "rstd": fin[1][:M].view(torch.float32)}
    return res


def _reference(d, mode):
    """(pre, budget, {fault: worst fault / budget}) of one (operands, mode): reference side only"""
    args = epilogue_ref_args(d, mode)
    A64, W64 = args["A"].double(), args["W"].double()
    acc, absacc = A64 @ W64.T, A64.abs() @ W64.abs().T
    pre, err = gemm_epilogue_fp64(mode, acc=acc, absacc=absacc, **args)
    bud = gemm_epilogue_budget(pre, err)
    faults = {}
    for f in EPI_FAULTS:
        if epi_fault_applies(f, mode, d["M"]):
            bad = gemm_epilogue_fp64(mode, acc=acc, absacc=absacc, fault=f, **args)[0]
            faults[f] = ((bad - pre).abs() / bud).max().item()
    return pre, bud, faults


def _check_stats(res, pre, d, variant, what, fails):
    """kernel statistics against float64 sums of the kernel's own output -> (worst / budget, {fault: fault / budget})"""
    ref = row_stats_fp64(res["out"], d["eps"])
    worst = 0.0
    for k, (want, b) in ref.items():
        if variant == 70 and k in ("psum", "psq"):
            continue
        got = res["stats"][k].double()
        if not torch.isfinite(got).all().item():
            fails.append((what, k, "non-finite or unwritten statistic"))
            continue
        worst = max(worst, ((got - want).abs() / b).max().item())
    faults = {}
    for f in STAT_FAULTS:
        bad = row_stats_fp64(res["out"], d["eps"], pre=pre, fault=f)
        faults[f] = max(((bad[k] - want).abs() / b).max().item() for k, (want, b) in ref.items())
    return worst, faults


def _run_group(hip, label, cells, variants):
    """Every (shape, row count, mode, variant) of a group: outputs, statistics, guards, variant 9 == 8; one line per (shape, mode);
    every failure is collected so that one run shows them all.  Each fault must break the budget at every row count, except `trunc`,
    which must break it at one row count of the (shape, mode) at least: truncation costs up to one ulp where rounding costs half, and
    only an element that loses nearly all of it, low in its binade, rises above a budget that also carries the accumulation bound
    (at K = 4096 about half of the rounding term); a one-row batch need not hold such an element (printed: the largest over the row
    counts; for every other fault the smallest)."""
    fails = []
    for role, N, K, Ms in cells:
        agg = {}                                                 # mode -> {"v": {variant: worst}, "s": {variant: worst}, "f": {fault: min}}
        for M in Ms:
            d = epilogue_inputs(M, N, K, seed=1000 * (N % 997) + 10 * (K % 991) + M % 7919, device="cuda")
            for mode in ROLE_MODES[role]:
                a = agg.setdefault(mode, {"v": {}, "s": {}, "f": {}})
                pre, bud, faults = _reference(d, mode)
                outs = {}
                for v in variants:
                    what = (label, N, K, M, mode, v)
                    res = run_ex(hip, d, mode, v)
                    outs[v] = res
                    for gname in res["guard"]:
                        fails.append((what, "guard fill overwritten", gname))
                    got = res["out"].double()
                    if not torch.isfinite(got).all().item():
                        fails.append((what, "non-finite output"))
                        continue
                    r = ((got - pre).abs() / bud).max().item()
                    a["v"][v] = max(a["v"].get(v, 0.0), r)
                    if r > 1:
                        fails.append((what, "output outside the budget", r))
                    if mode in (5, 6):
                        sr, sf = _check_stats(res, pre, d, v, what, fails)
                        a["s"][v] = max(a["s"].get(v, 0.0), sr)
                        if sr > 1:
                            fails.append((what, "statistics outside the budget", sr))
                        faults.update(sf)
                if 8 in outs and 9 in outs:
                    same = torch.equal(outs[8]["out"].view(torch.int16), outs[9]["out"].view(torch.int16))
                    if mode in (5, 6):
                        same = same and all(torch.equal(outs[8]["stats"][k].view(torch.int32), outs[9]["stats"][k].view(torch.int32))
                                            for k in outs[8]["stats"])
                    if not same:
                        fails.append(((label, N, K, M, mode), "variant 9 differs from variant 8"))
                for f, r in faults.items():
                    if f == "trunc":      # shows on the few elements that lose almost a whole ulp low in their binade: pooled over the row counts
                        a["f"][f] = max(a["f"].get(f, 0.0), r)
                        continue
                    a["f"][f] = min(a["f"].get(f, float("inf")), r)
                    if not r > 1:
                        fails.append(((label, N, K, M, mode), f, "the budget does not see this fault", r))
        for mode, a in agg.items():
            if not a["f"]["trunc"] > 1:
                fails.append(((label, N, K, mode), "trunc", "the budget does not see this fault at any row count", a["f"]["trunc"]))
            print(f"epilogue {label:15s} N={N:4d} K={K:4d} mode {mode} M={Ms[0]}..{Ms[-1]}: worst/budget "
                  + " ".join(f"v{v}={r:.3f}" for v, r in a["v"].items())
                  + (" | stats " + " ".join(f"v{v}={r:.3f}" for v, r in a["s"].items()) if a["s"] else "")
                  + " | smallest fault/budget " + " ".join(f"{f}={r:.3g}" for f, r in a["f"].items()))
    assert not fails, fails[:40]


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_mode_kernel_and_edge_shape_vs_fp64(hip, group):
    _run_group(hip, group, GROUPS[group], TILE_VARIANTS)


@pytest.mark.parametrize("group", list(SMALL_GROUPS))
def test_small_batch_kernel_every_mode_vs_fp64(hip, group):
    cells = [(role, N, K, Ms) for role, N, K, Ms in SMALL_GROUPS[group]]
    # statistics modes: the row is reduced inside one block, N <= 1024 (every O-projection / FFN-2 shape is)
    assert all(N <= 1024 for role, N, K, Ms in cells if set(ROLE_MODES[role]) & {5, 6} and role != "all")
    _run_group(hip, "small " + group, cells, (70,))


def _same(a, b):
    ok = torch.equal(a["out"].view(torch.int16), b["out"].view(torch.int16))
    if a["stats"] is not None:
        ok = ok and all(torch.equal(a["stats"][k].view(torch.int32), b["stats"][k].view(torch.int32)) for k in a["stats"])
    return ok


def test_bit_relations_hold_in_every_mode(hip):
    """A second call repeats the first bit for bit (every kernel, 70 included); on the tile kernels the first 391 rows of a 1041-row batch
    equal a 391-row batch of the same rows, output and statistics (corpus rows are batch-independent; the split-K kernel chooses its
    split count by the row count and makes no such promise)."""
    fails = []
    for N, K in ((384, 384), (768, 768), (1152, 384), (768, 3072), (768, 320)):
        d = epilogue_inputs(1041, N, K, seed=N + K, device="cuda")
        for mode in range(7):
            for v in TILE_VARIANTS:
                full, again, part = run_ex(hip, d, mode, v), run_ex(hip, d, mode, v), run_ex(hip, d, mode, v, rows=391)
                if not _same(full, again):
                    fails.append((N, K, mode, v, "a second call differs"))
                head = {"out": full["out"][:391], "stats": None if full["stats"] is None else
                        {k: (s[:, :391] if s.dim() == 2 else s[:391]) for k, s in full["stats"].items()}}
                if not _same(head, part):
                    fails.append((N, K, mode, v, "rows depend on the batch around them"))
            if mode in (5, 6) and N > 1024:
                continue
            a, b = run_ex(hip, d, mode, 70, rows=100), run_ex(hip, d, mode, 70, rows=100)
            if not _same(a, b):
                fails.append((N, K, mode, 70, "a second call differs"))
    assert not fails, fails


# ---- 4. GELU sweep -------------------------------------------------------------------------------------------------------------------
SWEEP_N, SWEEP_M, SWEEP_K = 1152, 64, 64                  # 1024 grid columns x 64 rows = 2^16 grid points, 128 columns of special values
BF16_MAX = float.fromhex("0x1.fep127")


def _sweep_operands(nontrivial):
    """A = identity (row m is one-hot at k = m), so acc[m][n] = W[n][m] exactly; W holds bf16 values, v = rstd_m (acc - mean_m s_n) + c_n.
    Targets: half of the grid uniform on [-5, 0], half on [-11.95, 11.95]; the special columns cycle +-1e4, +-0, +-largest finite bf16.  The
    non-trivial form takes rstd_m a power of two, mean_m multiples of 1/4 and s_n multiples of 1/64 (rstd_m mean_m s_n is exact in fp32
    and W' = bf16(target / rstd + mean s - c / rstd) puts v next to the same grid); there the largest finite bf16, which rstd = 2 would
    take to infinity, is replaced by 1e30.  Returns the operand dict and v in float64 computed from the stored values."""
    g = torch.Generator(device="cpu"); g.manual_seed(4)
    n_grid = 1024
    t = torch.cat([-5 * torch.rand((n_grid * SWEEP_M) // 2, generator=g, dtype=torch.float64),
                   23.9 * torch.rand((n_grid * SWEEP_M) // 2, generator=g, dtype=torch.float64) - 11.95])
    t = t[torch.randperm(t.numel(), generator=g)].view(n_grid, SWEEP_M)
    big = 1e30 if nontrivial else BF16_MAX
    sp = torch.tensor([1e4, -1e4, 0.0, -0.0, big, -big], dtype=torch.float64)
    t = torch.cat([t, sp.repeat((SWEEP_N - n_grid) * SWEEP_M // 6 + 1)[:(SWEEP_N - n_grid) * SWEEP_M].view(-1, SWEEP_M)])
    c = torch.cat([(torch.rand(n_grid, generator=g) - 0.5) * 0.1, torch.zeros(SWEEP_N - n_grid)]).float()
    m, n = torch.arange(SWEEP_M), torch.arange(SWEEP_N)
    if nontrivial:
        rstd = 2.0 ** ((m % 3) - 1).double()
        mean = ((m % 7) - 3).double() * 0.25
        s = torch.cat([((n[:n_grid] % 13) - 6).double() / 64, torch.zeros(SWEEP_N - n_grid, dtype=torch.float64)])
    else:
        rstd, mean, s = torch.ones(SWEEP_M, dtype=torch.float64), torch.zeros(SWEEP_M, dtype=torch.float64), torch.zeros(SWEEP_N, dtype=torch.float64)
    W = ((t - c.double()[:, None]) / rstd[None, :] + mean[None, :] * s[:, None]).to(torch.bfloat16)
    W = torch.where(t == 0, t.to(torch.bfloat16), W) if not nontrivial else W            # keeps the sign of -0
    v = rstd[None, :] * (W.double() - mean[None, :] * s[:, None]) + c.double()[:, None]     # [N, M]
    cap = 256
    pad = lambda x: torch.cat([x.float(), torch.zeros(cap - SWEEP_M)]).cuda()
    d = {"M": SWEEP_M, "N": SWEEP_N, "K": SWEEP_K, "row_cap": cap, "eps": 1e-5, "A": torch.eye(SWEEP_M).to(torch.bfloat16).cuda(),
         "W0": W.cuda(), "Wf": W.cuda(), "bias": c.cuda(), "c": c.cuda(), "s": s.float().cuda(), "a_mean": pad(mean), "a_rstd": pad(rstd),
         "resid": None, "r_mean": None, "r_rstd": None, "r_gamma": None, "r_beta": None}
    return d, v.T.contiguous().cuda()


@pytest.mark.parametrize("variant", [8, 13, 70, 71])
def test_gelu_sweep_through_the_epilogue(hip, variant):
    """|out - GELU64(v)| <= U8 |GELU64(v)| + 1.75e-4 + u |v| on every grid point and special value, outputs finite, and out in
    [-1.75e-4, 0] for v <= -6; the float64 tanh approximation breaks the same budget on the same grid."""
    for mode, nontrivial in ((1, False), (4, False), (4, True)):
        d, v = _sweep_operands(nontrivial)
        ref = gelu_fp64(v)
        ref = torch.where(v.abs() > 1e3, v.clamp_min(0), ref)                  # erf has saturated: GELU(v) = max(v, 0), no inf * 0
        bud = U8 * ref.abs() + GELU_POLY_BOUND + U24 * v.abs()
        res = run_ex(hip, d, mode, variant)
        assert not res["guard"], (variant, mode, nontrivial, res["guard"])
        out = res["out"].double()
        assert torch.isfinite(out).all().item(), (variant, mode, nontrivial, "non-finite output")
        r = (out - ref).abs() / bud
        i = int(r.argmax())
        print(f"gelu sweep v{variant} mode {mode} {'non-trivial' if nontrivial else 'plain'}: worst/budget {r.max().item():.3f} at v = {v.flatten()[i].item():.4f}; "
              f"worst |error| beyond the rounding {((out - ref).abs() - U8 * ref.abs()).max().item():.3e}")
        assert r.max().item() <= 1, (variant, mode, nontrivial, r.max().item(), v.flatten()[i].item())
        tail = out[v <= -6]
        assert tail.numel() > 1000 and (tail <= 0).all().item() and (tail >= -GELU_POLY_BOUND).all().item(), (variant, mode, nontrivial, "negative tail")
        grid = v.abs() <= 12
        tanh = 0.5 * v * (1 + torch.tanh(np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3)))
        tr = ((tanh - ref).abs() / bud)[grid].max().item()
        assert tr > 1, (variant, mode, nontrivial, "the sweep would not notice the tanh GELU", tr)
        assert int(grid.sum()) >= 1 << 16


# ---- 5. fold --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(1152, 384), (1536, 384), (2304, 768), (3072, 768), (3072, 1024), (4096, 1024)])
def test_fold_and_the_producer_finalize_consumer_loop(hip, N, K):
    """arx_fold_ln against float64, then the loop the forward runs: a mode 5 producer writes pre-LN rows y [M, K] and (through
    ln_finalize_kernel, or in its own epilogue for variant 70) their statistics; a mode 3 consumer takes y, the device's own (W', s, c) and
    the device's own statistics, and must equal LN(y) W^T + b in float64 from the UNFOLDED weights within: the mode 3 budget, plus the
    fold's weight rounding U8 sum_k |yhat_k W_k gamma_k| (each W'[n][k] is the bf16 rounding of W gamma), plus what the statistics'
    own budgets (row_stats_fp64) allow: |d rstd / rstd| |v - c| + rstd |d mean| |s_n|, plus the fold's c budget and rstd |mean| times its
    s budget."""
    lib, st = hip.load(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu"); g.manual_seed(N + K)
    W0 = (0.05 * torch.randn((N, K), generator=g)).to(torch.bfloat16).cuda()
    gamma, beta = (1 + 0.3 * (2 * torch.rand(K, generator=g) - 1)).cuda(), (0.2 + 0.3 * torch.randn(K, generator=g)).cuda()
    bias = (0.5 + torch.randn(N, generator=g)).cuda()
    Wf = _filled((N + 2, K), GUARD_BITS, torch.int16)
    s, c = _filled((N + 8,), GUARD_BITS32, torch.int32), _filled((N + 8,), GUARD_BITS32, torch.int32)
    hip.check(lib.arx_fold_ln(W0.data_ptr(), gamma.data_ptr(), beta.data_ptr(), bias.data_ptr(), Wf.data_ptr(), s.data_ptr(), c.data_ptr(),
                              N, K, st), "arx_fold_ln")
    torch.cuda.synchronize()
    assert (Wf[N:] == GUARD_BITS).all().item() and (s[N:] == GUARD_BITS32).all().item() and (c[N:] == GUARD_BITS32).all().item()
    Wf, s, c = Wf[:N].view(torch.bfloat16), s[:N].view(torch.float32), c[:N].view(torch.float32)
    assert torch.equal(Wf.view(torch.int16), (W0.float() * gamma).to(torch.bfloat16).view(torch.int16)), "W' is not bf16(fp32(W gamma))"
    prod, c64, c_bud = fold_ln_fp64(W0, gamma, beta, bias)
    s_bud = K * U24 * Wf.double().abs().sum(1)
    sr = ((s.double() - Wf.double().sum(1)).abs() / s_bud).max().item()
    cr = ((c.double() - c64).abs() / c_bud).max().item()
    assert sr <= 1 and cr <= 1, (N, K, "s / c outside the budget", sr, cr)
    line = f"fold N={N} K={K}: s worst/budget {sr:.3f}, c {cr:.3f}; loop worst/budget"
    for v in (89, 13, 71, 70):
        M = 250
        p = epilogue_inputs(M, K, 128, seed=K + v, device="cuda")              # producer: y = A W^T + b + resid, [M, K]
        prod_res = run_ex(hip, p, 5, v)
        assert not prod_res["guard"], (N, K, v, prod_res["guard"])
        y = prod_res["out"].contiguous()
        cap = p["row_cap"]
        pad = lambda x: torch.cat([x, torch.zeros(cap - M, device="cuda")]).contiguous()
        d = {"M": M, "N": N, "K": K, "row_cap": cap, "eps": p["eps"], "A": y, "Wf": Wf.contiguous(), "W0": W0, "c": c.contiguous(),
             "bias": bias, "s": s.contiguous(), "a_mean": pad(prod_res["stats"]["mean"]), "a_rstd": pad(prod_res["stats"]["rstd"]),
             "resid": None, "r_mean": None, "r_rstd": None, "r_gamma": None, "r_beta": None, "s_unf": None}
        res = run_ex(hip, d, 3, v)
        assert not res["guard"], (N, K, v, res["guard"])
        y64 = y.double()
        yhat = (y64 - y64.mean(1, keepdim=True)) / (y64.var(1, unbiased=False, keepdim=True) + p["eps"]).sqrt()
        want = layer_norm_fp64(y64, gamma.double(), beta.double(), p["eps"]) @ W0.double().T + bias.double()
        pre, err = gemm_epilogue_fp64(3, **epilogue_ref_args(d, 3))
        stats = row_stats_fp64(y, p["eps"])
        (mean, dmean), (rstd, drstd) = stats["mean"], stats["rstd"]
        bud = (gemm_epilogue_budget(want, err) + U8 * (yhat.abs() @ prod.abs().T)
               + (drstd / rstd)[:, None] * (pre - c.double()).abs() + (rstd * dmean)[:, None] * s.double().abs()[None, :] + c_bud[None, :]
               + (rstd * mean.abs())[:, None] * s_bud[None, :])
        r = ((res["out"].double() - want).abs() / bud).max().item()
        bad = layer_norm_fp64(y64, gamma.double().roll(1), beta.double(), p["eps"]) @ W0.double().T + bias.double()      # gamma one column off
        fr = ((bad - want).abs() / bud).max().item()
        line += f" v{v}={r:.3f} (gamma one column off: {fr:.1f})"
        assert r <= 1, (N, K, v, "consumer outside the budget", r)
        assert fr > 1, (N, K, v, "the loop's budget does not see a shifted gamma", fr)
    print(line)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_tap_refuses_what_the_kernels_refuse(hip):
    """Missing pointers per mode, N % 64 != 0 in the statistics modes, variant 70 beyond 256 rows or with statistics beyond N = 1024, an
    unknown mode or variant, row vectors shorter than a staged tile: ARX_ERR_ARG with a message and nothing launched (the guard-filled
    output keeps its fill)."""
    d = epilogue_inputs(300, 1152, 128, seed=1, device="cuda")

    def refused(mode, variant, rows=None, **override):
        dd = dict(d, **override)
        res = run_ex(hip, dd, mode, variant, rows=rows, check=False)
        msg = hip.load().arx_last_error().decode()
        M = rows or dd["M"]
        untouched = (res["out"].view(torch.int16) == GUARD_BITS).all().item() and not res["guard"]
        assert res["rc"] == -1 and msg and untouched, (mode, variant, override.keys(), res["rc"], msg, untouched)

    refused(7, 13); refused(-1, 13); refused(0, 12); refused(0, 0)
    refused(0, 13, bias=None)
    refused(2, 13, resid=None); refused(5, 13, resid=None); refused(6, 8, resid=None)
    for k in ("a_mean", "a_rstd", "s"):
        refused(3, 8, **{k: None}); refused(4, 13, **{k: None})
    for k in ("r_mean", "r_rstd", "r_gamma", "r_beta"):
        refused(6, 9, **{k: None})
    refused(3, 8, row_cap=300); refused(6, 89, row_cap=511); refused(4, 13, row_cap=299)
    refused(0, 70); refused(5, 70, rows=100)                                   # 300 rows; statistics at N = 1152
    d = epilogue_inputs(64, 1128, 64, seed=2, device="cuda")                   # N % 8 == 0 but not % 64
    refused(5, 13); refused(6, 71)
    d = epilogue_inputs(64, 1124, 64, seed=2, device="cuda")
    refused(0, 13)
    # statistics modes without their output buffers: run_ex always provides them, so call the tap directly
    d = epilogue_inputs(64, 256, 64, seed=3, device="cuda")
    out = _filled((64, 256), GUARD_BITS, torch.int16)
    for drop in ("out_mean", "part_sum", "n_rows"):
        bufs = {k: torch.zeros(4 * 72, device="cuda") for k in ("part_sum", "part_sq", "out_mean", "out_rstd")}
        bufs["n_rows"] = torch.tensor([64], dtype=torch.int32, device="cuda")
        e = hip.GemmEpilogueC(mode=5, variant=13, eps=1e-5, bias=_ptr(d["bias"]), resid=_ptr(d["resid"]), part_ld=72,
                              **{k: (None if k == drop else b.data_ptr()) for k, b in bufs.items()})
        rc = hip.load().arx_gemm_bf16_ex(d["A"].data_ptr(), d["W0"].data_ptr(), out.data_ptr(), 64, 256, 64, ctypes.byref(e), None)
        torch.cuda.synchronize()
        assert rc == -1 and hip.load().arx_last_error() and (out == GUARD_BITS).all().item(), (drop, rc)
