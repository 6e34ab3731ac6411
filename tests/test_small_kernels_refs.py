"""The references and budgets of tests/small_kernels_fp64.py on CPU: each agrees with an independent statement of the same operation
(the oracle's merge, torch's bf16 cast, a plain fp32 emulation of the kernel's arithmetic), and each rejects the faults planted on the
reference side.  tests/test_gpu_small_kernels_fp64.py trusts these as its yardstick."""
import numpy as np
import pytest

from oracle import search_oracle as SO
from tests import small_kernels_fp64 as R

torch = pytest.importorskip("torch")


def _existing_merge_inputs():
    """the inputs of tests/test_gpu_parity.py::test_merge_kernel_exact"""
    rs = np.random.RandomState(0)
    P, nq, k = 8, 37, 10
    s = -np.sort(-rs.standard_normal((P, nq, k)).astype(np.float32), axis=2)
    i = rs.randint(0, 10**9, size=(P, nq, k)).astype(np.int64)
    s[3, :, 5:] = -np.inf; i[3, :, 5:] = -1
    s[1, 0, 0] = s[2, 0, 0] = 9.0; i[1, 0, 0] = 500; i[2, 0, 0] = 100
    return s, i, k


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_merge_ref_agrees_with_the_oracle_and_sees_its_faults():
    s, i, k = _existing_merge_inputs()
    ref = R.merge_ref(s, i, k)
    assert _same(ref, SO.merge_partials(s, i, k))
    assert ref[1][0, 0] == 100 and ref[1][0, 1] == 500
    for f in R.MERGE_FAULTS:
        assert not _same(ref, R.merge_ref(s, i, k, fault=f)), f


@pytest.mark.parametrize("P,k", [(1, 1), (1, 32), (3, 7), (8, 10), (130, 31), (128, 32), (4096, 1)])
def test_merge_inputs_hold_what_the_gpu_test_needs(P, k):
    """merge_inputs: distinct ids per query up to 2^40, sorted lists, the roles of its docstring; merge_ref agrees with the oracle on them
    and, wherever the shape can show the fault at all, differs from the faulty variants."""
    nq = 13
    s, i = R.merge_inputs(P, k, nq, seed=P * 100 + k)
    assert s.shape == i.shape == (P, nq, k) and i.max() == 2 ** 40
    assert ((i < 0) == np.isneginf(s)).all()
    for q in range(nq):
        v = i[:, q][i[:, q] >= 0]
        assert len(np.unique(v)) == len(v)
    assert (s[:, :, :-1] >= s[:, :, 1:]).all()
    ref = R.merge_ref(s, i, k)
    assert _same(ref, SO.merge_partials(s, i, k))
    assert (ref[1][1] == -1).all() and (ref[1][7] == -1).all()                       # role 1: every part empty
    assert (ref[1][2, -1] == -1) and (k == 1 or ref[1][2, 0] >= 0)                   # role 2: fewer than k valid
    start = R.last_slot_start(P, k)
    if start % k == 0 and P * k - start >= k:                                        # role 3: the answer sits in the last slot
        cand = {int(x) for x in i[start // k:, 3].reshape(-1)}
        assert all(int(x) in cand for x in ref[1][3])
    if P >= 2:
        tied = np.argwhere(s[:, 0] == 50.0)                                           # role 0: the winner's tie, lower id in the later part
        assert len(tied) == 2 and tied[0][0] < tied[1][0] and i[tied[1][0], 0, tied[1][1]] < i[tied[0][0], 0, tied[0][1]]
        assert ref[0][0, 0] == 50.0 and ref[1][0, 0] == i[tied[1][0], 0, tied[1][1]]
        assert k == 1 or (ref[0][0, 1] == 50.0 and ref[1][0, 1] == i[tied[0][0], 0, tied[0][1]])
        assert not _same(ref, R.merge_ref(s, i, k, fault="tie_high_id"))
        assert not _same(ref, R.merge_ref(s, i, k, fault="skip_last_part"))
    u, _ = R.merge_inputs(P, k, 6, seed=5, sort_lists=False)
    assert k < 4 or not (u[:, :, :-1] >= u[:, :, 1:]).all()


def test_bf16_ref_agrees_with_torch_and_sees_its_faults():
    ex = R.bf16_exhaustive_bits()
    assert ex.shape == (65536 * 6,)
    for bits in (ex, R.bf16_random_bits()):
        want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = R.bf16_rne_ref(bits)
        nan = R.f32_is_nan(bits)
        assert np.array_equal(got[~nan], want[~nan])
        assert R.bf16_is_nan(got[nan]).all() and R.bf16_is_nan(want[nan]).all()
        assert np.array_equal(got[nan] >> 15, (bits[nan] >> 31).astype(np.uint16))   # the reference keeps a NaN's sign
        assert not R.bf16_is_nan(got[~nan]).any()
    fin = ~R.f32_is_nan(ex)
    ref = R.bf16_rne_ref(ex)
    assert ref[ex == 0x7F7FFFFF][0] == 0x7F80 and ref[ex == 0xFF7FFFFF][0] == 0xFF80          # above the largest bf16 -> inf
    assert not np.array_equal(ref[fin], R.bf16_rne_ref(ex, fault="trunc")[fin])
    ties = (ex & 0xFFFF) == 0x8000
    tie_even = ties & fin & ((ex >> 16) & 1 == 0)
    assert tie_even.any() and (ref[tie_even] != R.bf16_rne_ref(ex, fault="half_up")[tie_even]).all()
    assert np.array_equal(ref[fin & ~ties], R.bf16_rne_ref(ex, fault="half_up")[fin & ~ties])  # half-up differs on ties only
    # payload only in the low half, at or below the tie: the bare rounding turns these NaNs into +-inf
    low_nan = R.f32_is_nan(ex) & ((ex & 0x007F0000) == 0) & ((ex & 0xFFFF) <= 0x8000)
    assert low_nan.sum() == 6 and not R.bf16_is_nan(R.bf16_rne_ref(ex, fault="add_7fff")[low_nan]).any()
    assert np.array_equal(ref[fin], R.bf16_rne_ref(ex, fault="add_7fff")[fin])


@pytest.mark.parametrize("dim", [8, 72, 504, 520, 768, 1032, 8192])
def test_norm_window_holds_for_fp32_arithmetic(dim):
    pool = R.norm_pool(dim, seed=dim, n=7)
    for fam in range(4):
        rows = pool[fam * 7:(fam + 1) * 7]
        lo, hi = R.norm_window(R.max_norm_ref(rows), dim)
        got = R.emulate_max_norm_f32(rows)
        assert lo <= got <= hi, (dim, fam, got / lo - 1)
        if dim > 512:
            assert not lo <= R.emulate_max_norm_f32(rows, fault="first_512") <= hi, (dim, fam)


def test_norm_window_rejects_a_bound_that_is_not_rounded_up():
    """sqrt(fp32 sum) without the upward factor: on a row whose fp32 sum of squares lands below the exact sum (found by a seed search)
    the result is below the true norm, and the window's lower edge refuses it."""
    dim, found = 768, None
    for seed in range(200):
        rs = np.random.RandomState(seed)
        row = (rs.standard_normal((1, dim)) / np.sqrt(dim)).astype(np.float16)
        ref = R.max_norm_ref(row)
        if R.emulate_max_norm_f32(row, fault="no_up_factor") < ref:
            found = (seed, row, ref)
            break
    assert found is not None, "no row with an fp32 sum below its exact sum among 200 seeds"
    seed, row, ref = found
    lo, hi = R.norm_window(ref, dim)
    assert not lo <= R.emulate_max_norm_f32(row, fault="no_up_factor") <= hi
    assert lo <= R.emulate_max_norm_f32(row) <= hi
    print(f"norm window: seed {seed}: sqrt(fp32 sum) / ref - 1 = {R.emulate_max_norm_f32(row, fault='no_up_factor') / ref - 1:.3e}")


def test_max_norm_ref_specials():
    z = np.zeros((3, 16), np.float16)
    assert R.max_norm_ref(z) == 0.0
    z[2, 5] = np.inf
    assert R.max_norm_ref(z) == np.inf
    z[2, 6] = np.nan
    assert np.isnan(R.max_norm_ref(z))


@pytest.mark.parametrize("dim", [4, 12, 252, 260, 768, 8192])
def test_cosine_budget_holds_for_fp32_arithmetic_and_sees_its_faults(dim):
    e = R.cosine_rows(33, dim, seed=dim)
    ref, S = R.cosine_ref(e)
    ok = np.isfinite(ref)
    assert (~ok).sum() == 2 and np.isnan(ref[15]) and np.isnan(ref[16])               # the zero row 16: both cosines touching it
    assert abs(ref[1] - 1) < 1e-15 and abs(ref[3] + 1) < 1e-15 and (S[ok] >= np.abs(ref[ok]) - 1e-15).all()
    bud = R.cosine_budget(dim, S)
    got = R.emulate_cosine_f32(e).astype(np.float64)
    assert np.array_equal(np.isnan(got), ~ok)
    r = (np.abs(got - ref)[ok] / bud[ok]).max()
    assert r <= 1, (dim, "a plain fp32 cosine is outside the budget", r)
    line = [f"cosine D={dim}: fp32 emulation worst/budget {r:.3f}"]
    for f in R.COSINE_FAULTS:
        if f == "drop_last4" and dim == 4:
            continue                                                                  # nothing left to read
        bad = R.cosine_ref(e, fault=f)[0]
        both = ok & np.isfinite(bad)
        fr = np.abs(bad - ref)[both] / bud[both]
        # identical / negated pairs keep their cosine when both rows lose the same columns: every OTHER pair must move
        plain = np.ones(both.sum(), bool) if f == "row+2" else ~np.isin(np.flatnonzero(both), (1, 3))
        assert np.median(fr[plain]) > 1 and fr.max() > 1, (dim, f, "the budget does not see this fault", fr.max())
        line.append(f"{f} median fault/budget {np.median(fr[plain]):.3g}")
    print(" | ".join(line))
