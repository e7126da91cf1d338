"""CPU self-checks of the LayerNorm-conditioning harness (tests/_ln_cond.py) that tests/test_gpu_ln_cond.py relies on.

1. The generator hits every prescribed |mean| / sigma after rounding to bf16 / fp32, and rows of one launch never share statistics.
2. fp32 emulations of the kernels' formulas (two-pass LayerNorm, pooled finalize in both loop shapes) and the reference ops stay inside
   the derived bounds on every case of the GPU tables -- the bounds do not flag correct arithmetic.
3. Each planted defect in a Python stand-in breaks a bound on at least one row, and the failure names that row -- the bounds have teeth.
   The row-misrouting defects are also shown to PASS the whole-tensor check of tests/test_gpu_ops.py (rel-L2 <= 4e-3) on that file's
   `randn * 2 + 0.3` inputs: the gap these tests close.  No GPU code is involved.
"""
import pytest
import torch

import _ln_cond as L
from _ln_cond import BF, F32
from oracle.ops_ref import RefOps

ROW_C = [192, 768, 1024, 1028, 2048, 2052, 2730, 3072]                     # the row-kernel table of the GPU tests
FINALIZE_SETS = [(768, 64, 12), (1024, 64, 16), (2730, 32, 88), (341, 32, 12), (100, 64, 2), (64, 64, 1), (1090, 64, 18)]     # C, npp, P
FINALIZE_P = [7, 8, 9, 15, 16, 17, 33]                                       # npp = 32, C = P * 32 - 5
TOL_BF = 4e-3                                                                # the whole-tensor tolerance of tests/test_gpu_ops.py


@pytest.fixture(scope="module")
def ref():
    return RefOps()


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C", [64, 100, 192, 768, 1028, 2730])
def test_generator_hits_the_prescribed_ratios_after_rounding(C, dtype):
    M = 84                                                                   # lcm(7 ratios, 4 scales, 3 outliers): every combination once
    x, d = L.skewed_rows(M, C, 3, dtype)
    assert x.dtype == dtype and tuple(x.shape) == (M, C)
    mean, var = x.double().mean(-1), x.double().var(-1, unbiased=False)       # descriptors are those of the STORED values
    assert torch.allclose(mean, d["mean"], rtol=1e-12, atol=0) and torch.allclose(var, d["var"], rtol=1e-12, atol=0)
    r = mean.abs() / var.sqrt()
    for i in range(M):
        r0 = float(d["ratio0"][i])
        assert (abs(float(r[i]) / r0 - 1) <= 0.01) if r0 > 0 else (float(r[i]) <= 0.01), f"{L.describe(d, i)}: achieved ratio {float(r[i]):.4g}"
        assert abs(float(var[i].sqrt()) / float(d["scale"][i]) - 1) <= 0.5, f"{L.describe(d, i)}: sigma {float(var[i].sqrt()):.3g}"
    pairs = {(float(d["ratio0"][i]), float(d["scale"][i])) for i in range(28)}
    assert len(pairs) == 21, "every (ratio, scale) pair occurs within 28 rows"
    combos = {(float(d["ratio0"][i]), float(d["scale"][i]), bool(d["outlier"][i])) for i in range(M)}
    assert len(combos) == 42
    rstd = d["rstd"]
    for i in range(M - 1):                                                   # neighbours never share (mean, rstd)
        assert abs(float(rstd[i] / rstd[i + 1]) - 1) > 0.5 and float(d["mean"][i]) != float(d["mean"][i + 1])
    o = x[d["outlier"] & (d["ratio0"] <= 20)].double()                      # (above that, bf16 leaves a row two or three levels)
    dev = (o - o.mean(-1, keepdim=True)).abs()
    top = dev.topk(3, dim=-1).indices.sort(-1).values
    assert (top == torch.tensor([0, C // 2, C - 1])).all(), "outlier channels: first, middle, last column"


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C", ROW_C)
def test_two_pass_emulation_is_inside_the_bounds_and_one_pass_is_not(C, dtype):
    x, d = L.skewed_rows(37, C, 11, dtype)
    mean, rstd = L.emul_ln_two_pass(x)
    for what, err, bound in (("mean", (mean.double() - d["mean"]).abs(), L.ln_mean_bound(d)),
                             ("rstd", (rstd.double() / d["rstd"] - 1).abs(), L.ln_rstd_bound(d) * torch.ones(37, dtype=torch.float64))):
        worst, msg = L.check_rows(err, bound, d, f"two-pass {what} C={C}")
        assert msg is None and worst <= 0.5, msg or worst
    _, rstd1 = L.emul_ln_two_pass(x, one_pass=True)
    worst, msg = L.check_rows((rstd1.double() / d["rstd"] - 1).abs(), L.ln_rstd_bound(d) * torch.ones(37, dtype=torch.float64), d, "one-pass rstd")
    assert msg is not None and "row " in msg and ("ratio 1000" in msg or "ratio 100" in msg), msg
    # ... and only rows whose mean dwarfs their spread give it away: the ratio-0 rows are fine
    ok = (rstd1.double() / d["rstd"] - 1).abs()[d["ratio0"] == 0] <= L.ln_rstd_bound(d)
    assert ok.all()


def _finalize_case(C, npp, P, M, outliers, seed=5):
    x, d = L.skewed_rows(M, C, seed, F32, outliers=outliers)
    return L.exact_partials(x, npp, P), d


def _finalize_ratios(part, npp, C, P_valid, d, **kw):
    mean, rstd = L.emul_finalize(part, npp, C, **kw)
    rm, mm = L.check_rows((mean.double() - d["mean"]).abs(), L.finalize_mean_bound(P_valid, d), d, "finalize mean")
    rr, mr = L.check_rows((rstd.double() / d["rstd"] - 1).abs(), L.finalize_rstd_bound(P_valid, d), d, "finalize rstd")
    return rm, rr, mm, mr


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("shape", ["8+tail", "16clamped"])
@pytest.mark.parametrize("C,npp,P", FINALIZE_SETS + [(p * 32 - 5, 32, p) for p in FINALIZE_P])
def test_finalize_emulation_stays_below_0p3_of_both_bounds(C, npp, P, shape, outliers):
    part, d = _finalize_case(C, npp, P, 84, outliers)
    Pv = (C + npp - 1) // npp
    assert torch.isnan(part[Pv:]).all() and torch.isfinite(part[:Pv]).all()    # slices past C are poison: they must be ignored
    rm, rr, mm, mr = _finalize_ratios(part, npp, C, Pv, d, shape=shape)
    assert mm is None and mr is None and rm <= 0.3 and rr <= 0.3, (rm, rr, mm, mr)


def test_finalize_loop_shapes_are_the_same_arithmetic():
    for C, npp, P in FINALIZE_SETS:
        part, _ = _finalize_case(C, npp, P, 42, True)
        a, b = L.emul_finalize(part, npp, C, shape="8+tail"), L.emul_finalize(part, npp, C, shape="16clamped")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", ["8+tail", "16clamped"])
@pytest.mark.parametrize("defect,which", [("no_between", "rstd"), ("past_C", "both"), ("skip_ragged", "both"), ("mean_P_npp", "mean")])
@pytest.mark.parametrize("C,npp,P", [(2730, 32, 88), (341, 32, 12)])
def test_finalize_defects_break_a_bound_and_name_the_row(C, npp, P, defect, which, shape):
    part, d = _finalize_case(C, npp, P, 84, True)
    Pv = (C + npp - 1) // npp
    _, _, mm, mr = _finalize_ratios(part, npp, C, Pv, d, shape=shape, defect=defect)
    if which in ("mean", "both"):
        assert mm is not None and "row " in mm and "ratio " in mm and "scale 2^" in mm, mm
    if which in ("rstd", "both"):
        assert mr is not None and "row " in mr and "ratio " in mr and "scale 2^" in mr, mr


def _folded_problem(x, N, seed):
    """A q|k|v-style folded GEMM of rows x (bf16 copy as the A operand, statistics of the stored bf16 rows in fp32)."""
    M, K = x.shape
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.05
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    b = torch.randn(N, generator=g)
    A = x.to(BF)
    mean64, rstd64, _ = L.ln_ref64(A)
    Wf = (W * gamma).to(BF)
    return dict(A=A, Wf=Wf, mean=mean64.float(), rstd=rstd64.float(), colsum=Wf.float().sum(1), bias=W @ beta + b)


@pytest.mark.parametrize("K", [192, 768])
def test_reference_folded_gemm_is_inside_the_gemm_bound(ref, K):
    x, d = L.skewed_rows(261, K, 21, BF)
    p = _folded_problem(x, 192, 22)
    out64, bound = L.folded_gemm_ref64(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"])
    got = torch.empty(261, 192, dtype=BF)
    ref.gemm_nt_ln(p["A"], p["Wf"], got, bias=p["bias"], ln_mean=p["mean"], ln_rstd=p["rstd"], ln_colsum=p["colsum"], epi=0)
    worst, msg = L.check_rows((got.double() - out64).abs(), bound + L.bf16_half_ulp(out64), d, "RefOps folded GEMM (bf16)")
    assert msg is None, msg
    extra = torch.randn(261, 192, generator=torch.Generator().manual_seed(23))
    got32 = torch.empty(261, 192)
    ref.gemm_nt_ln(p["A"], p["Wf"], got32, bias=p["bias"], extra=extra, ln_mean=p["mean"], ln_rstd=p["rstd"], ln_colsum=p["colsum"], epi=6)
    out64, bound = L.folded_gemm_ref64(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"], extra=extra)
    worst, msg = L.check_rows((got32.double() - out64).abs(), bound, d, "RefOps folded GEMM (fp32 residual)")
    assert msg is None, msg
    good = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"])
    out64, bound = L.folded_gemm_ref64(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"])
    worst, msg = L.check_rows((good.double() - out64).abs(), bound, d, "stand-in without a defect")
    assert msg is None, msg


@pytest.mark.parametrize("defect", ["xor1", "clamp_m2", "no_colsum"])
def test_gemm_epilogue_defects_break_the_bound_on_skewed_rows(defect):
    x, d = L.skewed_rows(261, 768, 21, BF)
    p = _folded_problem(x, 192, 22)
    out64, bound = L.folded_gemm_ref64(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"])
    bad = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"], defect=defect).to(BF)
    worst, msg = L.check_rows((bad.double() - out64).abs(), bound + L.bf16_half_ulp(out64), d, defect)
    assert msg is not None and "row " in msg and "ratio " in msg, msg
    if defect == "xor1":
        assert "row 254" in msg or "row 255" in msg, msg
        assert worst > 100, "rows 2^10 apart in scale: a misrouted statistic misses by orders of magnitude"
    if defect == "clamp_m2":
        assert "row 260" in msg and worst > 100, msg


@pytest.mark.parametrize("defect,M,K", [("xor1", 1000, 1024), ("clamp_m2", 394, 768), ("clamp_m2", 1000, 1024)])
def test_misrouted_row_statistics_slip_past_the_whole_tensor_check(defect, M, K):
    """The gap: on the inputs and shapes of tests/test_gpu_ops.py (randn * 2 + 0.3; M, C = 394, 768 and 1000, 1024) the same defects stay
    under rel-L2 <= 4e-3.  (Measured: a swapped row pair reads 5.6e-4 of 1000 rows -- and 6.8e-3 of 394, where the old check would
    have seen it; one misrouted row reads 1.3e-3 .. 2.0e-3.)"""
    x = L.plain_rows(M, K, 72)
    p = _folded_problem(x, 192, 74)
    good = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"]).to(BF)
    bad = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"], defect=defect).to(BF)
    assert not torch.equal(bad, good)
    r = L.rel_l2(bad, good)
    print(f"{defect} M={M} K={K}: whole-tensor rel-L2 {r:.2e}")
    assert r <= TOL_BF, f"{defect}: rel-L2 {r:.2e}"


def test_dropped_mean_colsum_against_the_whole_tensor_check():
    """`mean * colsum` dropped: measured, not assumed.  With the column sums of a random W (.) gamma (|colsum| ~ 0.05 sqrt(K) = 1.4) the
    offset 0.3 of the old inputs is already enough for the whole-tensor check to see the missing term (rel-L2 ~ 0.1 >> 4e-3): unlike the
    two misrouting defects this one did not slip through.  On the skewed rows it misses the bound by more than 10^3."""
    x = L.plain_rows(394, 768, 72)
    p = _folded_problem(x, 192, 74)
    good = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"]).to(BF)
    bad = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"], defect="no_colsum").to(BF)
    r = L.rel_l2(bad, good)
    print(f"no_colsum: whole-tensor rel-L2 {r:.2e}")
    assert r > TOL_BF
    x, d = L.skewed_rows(261, 768, 21, BF)
    p = _folded_problem(x, 192, 22)
    out64, bound = L.folded_gemm_ref64(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"])
    bad = L.standin_folded_gemm(p["A"], p["Wf"], p["mean"], p["rstd"], p["colsum"], p["bias"], defect="no_colsum").to(BF)
    worst, msg = L.check_rows((bad.double() - out64).abs(), bound + L.bf16_half_ulp(out64), d, "no_colsum")
    assert worst > 1e3 and "ratio 1000" in msg, msg


def test_a_correctly_rounded_bf16_value_needs_the_exact_half_ulp():
    """Why the bf16 term of the bounds is bf16_half_ulp and not 2^-9 |y|: rounding the exact value errs by up to 2^-8 |y|."""
    y = torch.linspace(1.0, 2.0, 4097, dtype=torch.float64)[:-1]
    err = (y.float().to(BF).double() - y).abs()
    assert float((err / y).max()) > 1.9 * 2.0 ** -9 and (err <= L.bf16_half_ulp(y)).all()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32_rows", "bf16_rows"])
def test_refops_spread_of_the_folded_to_plain_ratio(ref, dtype):
    """The margin of the GPU claim test is three times RefOps' own spread of folded / plain over 8 seeds; re-measured here."""
    ratios = []
    for seed in range(8):
        pr = L.claim_problem(seed, dtype)
        plain, folded = L.claim_chains(ref, pr)
        ratios.append([f / p for f, p in zip(L.claim_rms(folded, pr), L.claim_rms(plain, pr))])
    t = torch.tensor(ratios, dtype=torch.float64)
    spread = float(((t / t.mean(0)) - 1).abs().max())
    print("folded/plain per group, mean over seeds:", [f"{v:.3f}" for v in t.mean(0).tolist()], f"spread {spread:.3f}")
    assert spread <= L.REFOPS_RATIO_SPREAD[dtype] * 1.1, spread
    if dtype == BF:                                                 # engine.py: the sub-LayerNorm folds are never worse than the plain schedule
        assert float(t.max()) <= 1.0
