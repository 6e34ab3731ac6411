"""The float64 GEMM-epilogue references and budgets of tests/helpers.py (gemm_epilogue_fp64, row_stats_fp64) on CPU, with a plain fp32
emulation of the kernels' arithmetic (bf16 operands, fp32 accumulation and epilogue, round-to-nearest bf16 output, fp32 statistics of
the rounded values) standing in for them: a faithful implementation stays inside every budget, and every fault the GPU module
tests/test_gpu_gemm_epilogue_fp64.py lists breaks it.  The GPU module trusts these as its yardstick."""
import numpy as np
import pytest

from tests.helpers import (EPI_FAULTS, STAT_FAULTS, U24, epi_fault_applies, epilogue_inputs, epilogue_ref_args, gemm_epilogue_budget,
                           gemm_epilogue_fp64, gelu_fp64, row_stats_fp64)

torch = pytest.importorskip("torch")


def emulate_fp32(mode, d):
    """(bf16 output, stats dict) of mode `mode` in fp32 torch arithmetic; exact-erf GELU (the kernels' polynomial has its own documented
    bound, which the budget carries)"""
    M, N = d["M"], d["N"]
    a = epilogue_ref_args(d, mode)
    acc = a["A"].float() @ a["W"].float().T
    if mode in (3, 4):
        v = d["a_rstd"][:M, None] * (acc - d["a_mean"][:M, None] * d["s"][None]) + d["c"]
    else:
        v = acc + d["bias"]
    if mode in (1, 4):
        v = gelu_fp64(v.double()).float()
    if mode in (2, 5):
        v = v + d["resid"].float()
    if mode == 6:
        v = v + (((d["resid"].float() - d["r_mean"][:M, None]) * d["r_rstd"][:M, None]) * d["r_gamma"] + d["r_beta"])
    out = v.to(torch.bfloat16)
    x = out.float().view(M, N // 64, 64)
    ps, pq = x.sum(-1).T.contiguous(), (x * x).sum(-1).T.contiguous()
    mu = ps.sum(0) * np.float32(1.0 / N)
    rstd = ((pq.sum(0) * np.float32(1.0 / N) - mu * mu).clamp_min(0) + np.float32(d["eps"])).rsqrt()
    return out, {"psum": ps, "psq": pq, "mean": mu, "rstd": rstd}


@pytest.mark.parametrize("M,N,K", [(37, 128, 64), (130, 384, 768), (64, 256, 3072), (1, 384, 384), (2, 768, 192)])
def test_budget_holds_for_fp32_arithmetic_and_sees_every_fault(M, N, K):
    d = epilogue_inputs(M, N, K, seed=M + N + K)
    for mode in range(7):
        args = epilogue_ref_args(d, mode)
        A64, W64 = args["A"].double(), args["W"].double()
        acc, absacc = A64 @ W64.T, A64.abs() @ W64.abs().T
        pre, err = gemm_epilogue_fp64(mode, acc=acc, absacc=absacc, **args)
        bud = gemm_epilogue_budget(pre, err)
        out, st = emulate_fp32(mode, d)
        r = ((out.double() - pre).abs() / bud).max().item()
        assert r <= 1, (mode, M, N, K, "a faithful fp32 implementation is outside the budget", r)
        for f in EPI_FAULTS:
            if not epi_fault_applies(f, mode, M):
                continue
            bad = gemm_epilogue_fp64(mode, acc=acc, absacc=absacc, fault=f, **args)[0]
            fr = ((bad - pre).abs() / bud).max().item()
            assert fr > 1, (mode, M, N, K, f, "the budget does not see this fault", fr)
        if mode in (5, 6):
            ref = row_stats_fp64(out, d["eps"])
            for k, (want, b) in ref.items():
                sr = ((st[k].double() - want).abs() / b).max().item()
                assert sr <= 1, (mode, M, N, K, k, "faithful fp32 statistics outside the budget", sr)
            for f in STAT_FAULTS:
                bad = row_stats_fp64(out, d["eps"], pre=pre, fault=f)
                fr = max(((bad[k] - want).abs() / b).max().item() for k, (want, b) in ref.items())
                assert fr > 1, (mode, M, N, K, f, "the statistics budget does not see this fault", fr)


def test_the_tanh_gelu_is_a_different_activation_on_the_sweep_grid():
    """tests/test_gpu_gemm_epilogue_fp64.py sweeps GELU over [-12, 12] with the budget U8 |GELU(v)| + 1.75e-4 + u |v|: the tanh
    approximation, in float64, must break it (so the sweep would notice another activation)."""
    v = torch.linspace(-12, 12, 1 << 16, dtype=torch.float64)
    ref = gelu_fp64(v)
    tanh = 0.5 * v * (1 + torch.tanh(np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3)))
    r = ((tanh - ref).abs() / (2.0 ** -8 * ref.abs() + 1.75e-4 + U24 * v.abs())).max().item()
    assert r > 1, r
