"""The exact-operand GEMM instrument (tests/_exact_gemm.py) checked without a GPU.

  * agreement with the oracle: on every case family the GPU module runs, the RefOps GEMMs equal the float64 reference bit for bit -- which
    ties the new reference to the project's oracle and shows that the 2^24 precondition does what it claims (RefOps accumulates in fp32 in
    whatever order the BLAS picks);
  * sensitivity: six corruptions of one expected output, small against the whole tensor; which of them today's relative-L2 check accepts,
    and that the bit comparator rejects every one;
  * the non-linear epilogues: a plain fp32 evaluation of SwiGLU / GELU / QuickGELU on the exact pre-activations stays inside the per-element
    bound and the 1 % share of the GPU test, so the inputs allow the check.
"""
import pytest
import torch

import _exact_gemm as X
from _exact_gemm import BF, F32
from oracle.ops_ref import RefOps

TOL_BF, TOL_F32 = 4e-3, 2e-5                # tests/test_gpu_ops.py


def rel(a, b):                              # tests/test_gpu_ops.py
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def ref():
    return RefOps()


def same_bits(got, want):
    return X.bits_mismatch("cpu", got, want) is None


# ------------------------------------------------------------------------------------------------ the selection
def test_the_selection_covers_every_value_and_every_pair_of_edge_classes():
    assert {t[0] for t in X.TRIPLES} == set(X.M_VALUES) and {t[1] for t in X.TRIPLES} == set(X.N_VALUES) and {t[2] for t in X.TRIPLES} == set(X.K_VALUES)
    assert {(X.m_class(M), X.n_class(N)) for M, N, _ in X.TRIPLES} == {(i, j) for i in range(4) for j in range(4)}
    assert 28 <= len(X.TRIPLES) <= 34 and len(set(X.TRIPLES)) == len(X.TRIPLES)
    assert all(N % 32 == 0 for _, N, _ in X.TRIPLES_N32 + X.F8_SHAPES) and {K for _, _, K in X.F8_SHAPES} == {128, 256, 384}
    assert {m_ for m_, _, _ in X.BM192_SHAPES} == {192, 193, 383, 385, 449}
    assert {(K + 63) // 64 for _, _, K in X.WGRAD_SHAPES} == {1, 2, 3, 13}
    assert {T for T, _, _ in X.WGRAD_TN_SHAPES} == {1, 7, 63, 64, 65, 200}
    assert {N for _, N, _ in X.WGRAD_TN_SHAPES} == {8, 24, 248, 256, 264} == {K for _, _, K in X.WGRAD_TN_SHAPES}
    assert set(X.FLAGS) == {0, 1, 0x10, 0x20, 0x30, 0x31, 0x70, 0x71, 0x8070, 0x90, 0xB0, 0x10B0}


def test_generators_are_seeded_and_hold_what_they_promise():
    a, b = X.int_bf16((64, 256), 3, 5), X.int_bf16((64, 256), 3, 5)
    assert torch.equal(a, b) and not torch.equal(a, X.int_bf16((64, 256), 3, 6))
    af = a.float()
    assert set(af.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0} and 0.28 < float((af == 0).float().mean()) < 0.39
    assert set(X.rstd_f32(300, 1).tolist()) == {0.5, 1.0, 2.0}
    assert set(X.pow2_f32(300, 1).tolist()) == {0.5, 1.0, 2.0}
    codes = X.e4m3_codes((16, 128), 3, 2)
    assert codes.dtype == torch.uint8 and set(codes.view(torch.float8_e4m3fn).float().unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert X.quantum(torch.tensor([0.5, 3.0])) == 0.5 and X.quantum(torch.tensor([2.0, 4.0])) == 1.0 and X.quantum(torch.tensor([0.375])) == 0.125


def test_a_case_outside_the_precondition_raises():
    o = X.operands(64, 64, 448, 1)
    X.exact_gemm(o["A"], o["B"], o["bias"])
    with pytest.raises(X.ExactnessError, match="2\\^24"):
        X.exact_gemm(o["A"], o["B"], o["bias"] * 2.0 ** 15)                  # |bias| up to 3.3e7 steps
    with pytest.raises(X.ExactnessError, match="2\\^24"):
        X.exact_gemm(o["A"], o["B"], o["bias"] + 2.0 ** -14)                 # a step of 2^-14 under values of ~1000
    with pytest.raises(X.ExactnessError):
        X.exact_stats(X.exact_gemm(o["A"], o["B"], o["bias"] * 8), 64)       # squares of ~8000 over 64 columns
    with pytest.raises(X.ExactnessError, match="rounding claim"):
        X.assert_rounding_is_tested("small values", X.exact_gemm(o["A"], o["B"]))


# ------------------------------------------------------------------------------------------------ agreement with the oracle
@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_oracle_gemm_nt_equals_the_exact_reference(ref, M, N, K):
    """RefOps.gemm_nt, epilogues 0, 1, 2, 4, 5, and the pre-activations of the non-linear cases."""
    o = X.operands(M, N, K, seed=100)
    v = X.exact_gemm(o["A"], o["B"], o["bias"])
    X.assert_rounding_is_tested(f"wide[{M},{N},{K}]", v)
    c = torch.empty(M, N, dtype=BF)
    ref.gemm_nt(o["A"], o["B"], c, o["bias"], epi=0)
    assert same_bits(c, X.want_bf16(v))
    c = torch.empty(M, N)
    ref.gemm_nt(o["A"], o["B"], c, o["bias"], epi=1)
    assert same_bits(c, X.want_f32(v))
    ref.gemm_nt(o["A"], o["B"], c, o["bias"], o["res"], epi=2)
    assert same_bits(c, X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], o["res"])))
    c = o["res"].clone()
    ref.gemm_nt(o["A"], o["B"], c, epi=4)
    assert same_bits(c, X.want_f32(X.exact_gemm(o["A"], o["B"], None, o["res"])))
    G = X.patch_group(M)
    rows = M + (M + G - 1) // G
    pos = X.int_f32((G + 1, N), 1000, 107)
    orow, prow = X.patch_rows(M, G)
    want = torch.full((rows, N), float("nan"))
    want[orow] = X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], pos[prow]))
    if M % G == 0:                                                            # RefOps states whole images only
        c = torch.full((rows, N), float("nan"))
        ref.gemm_nt(o["A"], o["B"], c, o["bias"], pos, epi=5, group=G)
        assert same_bits(c, want)
    else:
        assert same_bits(want[orow], (X.exact_gemm(o["A"], o["B"], o["bias"]) + pos[prow].double()).float())
    for epi in (3, 7, 8):
        a = X.act_case(M, N, K, 300 + epi, epi)
        pre = a["pre"]
        c = torch.empty(M, a["B"].shape[0])
        ref.gemm_nt(a["A"], a["B"], c, a["bias"], epi=1)
        assert same_bits(c, X.want_f32(pre))


@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_oracle_gemm_nt_ln_equals_the_exact_reference(ref, M, N, K):
    """RefOps.gemm_nt_ln: epilogue 6, epilogue 0 with the fold, epilogues 2 / 6 with the bf16 copy and the statistics partials."""
    o = X.operands(M, N, K, seed=200)
    ln = (o["mean"], o["rstd"], o["colsum"])
    c = torch.empty(M, N)
    ref.gemm_nt_ln(o["A"], o["B"], c, bias=o["bias"], extra=o["res"], ln_mean=ln[0], ln_rstd=ln[1], ln_colsum=ln[2], epi=6)
    assert same_bits(c, X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], o["res"], ln=ln)))
    v0 = X.exact_gemm(o["A"], o["B"], o["bias"], ln=ln)
    X.assert_rounding_is_tested(f"ln wide[{M},{N},{K}]", v0)
    cb = torch.empty(M, N, dtype=BF)
    ref.gemm_nt_ln(o["A"], o["B"], cb, bias=o["bias"], ln_mean=ln[0], ln_rstd=ln[1], ln_colsum=ln[2], epi=0)
    assert same_bits(cb, X.want_bf16(v0))
    s = X.operands(M, N, K, seed=210, profile="stats")
    ln = (s["mean"], s["rstd"], s["colsum"])
    S = (N + 63) // 64
    for epi, fold in ((2, None), (6, ln)):
        v = X.exact_gemm(s["A"], s["B"], s["bias"], s["res"], ln=fold)
        X.assert_rounding_is_tested(f"stats[{M},{N},{K}] epi {epi}", v)
        c, xb, part = torch.empty(M, N), torch.empty(M, N, dtype=BF), torch.empty(S, M, 2)
        kw = dict(ln_mean=ln[0], ln_rstd=ln[1], ln_colsum=ln[2]) if fold else {}
        ref.gemm_nt_ln(s["A"], s["B"], c, bias=s["bias"], extra=s["res"], stats_part=part, xb_out=xb, epi=epi, **kw)
        assert same_bits(c, X.want_f32(v)) and same_bits(xb, X.want_bf16(v)) and same_bits(part, X.exact_stats(v, 64))


@pytest.mark.parametrize("M,N,K", X.TRIPLES_N32)
def test_oracle_split_stream_equals_the_exact_reference(ref, M, N, K):
    """RefOps.gemm_nt_ln_split chained as the tower chains it: fp32 in -> planes -> planes -> fp32 out."""
    o = X.operands(M, N, K, seed=400, profile="stats")
    x1, x2, x3 = X.split_chain(o, M, N)
    ln = (o["mean"], o["rstd"], o["colsum"])
    hi, lo, part = torch.empty(M, N, dtype=BF), torch.empty(M, N, dtype=torch.int16), torch.empty((N + 63) // 64, M, 2)
    ref.gemm_nt_ln_split(o["A"], o["B"], hi, lo, o["bias"], *ln, x_in=o["res"], stats_part=part)
    h, l = RefOps.split_planes(X.want_f32(x1))
    assert same_bits(hi, h) and same_bits(lo, l) and same_bits(part, X.exact_stats(x1, 64))
    ref.gemm_nt_ln_split(o["A"], o["B"], hi, lo, o["bias"], *ln, stats_part=part)
    h, l = RefOps.split_planes(X.want_f32(x2))
    assert same_bits(hi, h) and same_bits(lo, l) and same_bits(part, X.exact_stats(x2, 64))
    out = torch.empty(M, N)
    ref.gemm_nt_ln_split(o["A"], o["B"], hi, lo, o["bias"], *ln, x_out=out)
    assert same_bits(out, X.want_f32(x3))
    ties = int(((X.want_f32(x1).view(torch.int32) & 0xFFFF) == 0x8000).sum())
    assert M * N < X.CENSUS_MIN_ELEMENTS or ties >= 10      # the hi plane's rule (halves away from zero) is exercised


@pytest.mark.parametrize("M,N,K", X.WGRAD_SHAPES)
def test_oracle_wgrad_equals_the_exact_reference(ref, M, N, K):
    A, B, base = X.int_bf16((M, K), 3, 500), X.int_bf16((N, K), 2, 501), X.int_f32((M, N), 1000, 502)
    dW = base.clone()
    ref.gemm_wgrad(A, B, dW, None)
    assert same_bits(dW, X.want_f32(X.exact_gemm(A, B, None, base)))


@pytest.mark.parametrize("T,N,K", X.WGRAD_TN_SHAPES)
def test_oracle_wgrad_tn_equals_the_exact_reference(ref, T, N, K):
    dY, Xt, base = X.int_bf16((T, N), 3, 510), X.int_bf16((T, K), 2, 511), X.int_f32((N, K), 1000, 512)
    dW = base.clone()
    ref.gemm_wgrad_tn(dY, Xt, dW, None)
    assert same_bits(dW, X.want_f32(X.exact_gemm(dY.T, Xt.T, None, base)))


@pytest.mark.parametrize("M,N,K8", X.F8_SHAPES)
def test_oracle_fp8_gemm_equals_the_exact_reference(ref, M, N, K8):
    A8, B8 = X.e4m3_codes((M, K8), 3, 600), X.e4m3_codes((N, K8), 2, 601)
    rs, cs, bias, res = X.pow2_f32(M, 602), X.pow2_f32(N, 603), X.int_f32((N,), 1000, 604), X.int_f32((M, N), 1000, 605)
    v = X.exact_gemm(A8, B8, bias, scales=(rs, cs))
    X.assert_rounding_is_tested(f"f8[{M},{N},{K8}]", v)
    c = torch.empty(M, N, dtype=BF)
    ref.gemm_nt_f8(A8, B8, c, rs, cs, bias=bias, epi=0)
    assert same_bits(c, X.want_bf16(v))
    c = torch.empty(M, N)
    ref.gemm_nt_f8(A8, B8, c, rs, cs, bias=bias, extra=res, epi=2)
    assert same_bits(c, X.want_f32(X.exact_gemm(A8, B8, bias, res, scales=(rs, cs))))


def test_oracle_fp8_quantiser_on_power_of_two_rows(ref):
    x, codes, scale = X.fp8_quant_case(37, 200, 610)
    q, s = torch.full((37, 256), 0x55, dtype=torch.uint8), torch.empty(37)
    ref.quant_rows_fp8(x, q, s)
    assert torch.equal(q, codes) and torch.equal(s, scale)


# ------------------------------------------------------------------------------------------------ sensitivity
def test_the_bit_comparator_rejects_what_the_relative_l2_check_accepts():
    """Six corruptions of one bf16 output (449 x 516, K = 448), each small against the whole tensor.  Today's check of a bf16 GEMM output is
    rel() <= TOL_BF: it accepts five of them (the second on an output whose bias is small against the products).  The sixth -- the bias of the last vector lane of the last partial tile taken from four
    columns further left -- it accepts when the bias is small against the products (|bias| = 1 against products of
    rms ~48) and rejects on the wide-bias operands of this module, where four columns of 516 carry a wrong +-1000.  The bit comparator
    rejects all of them and names the place."""
    M, N, K = 449, 516, 448
    o = X.operands(M, N, K, seed=700)
    v = X.exact_gemm(o["A"], o["B"], o["bias"])
    want = X.want_bf16(v)
    wf = want.float()
    spacing = X.bf16_spacing(wf.double()).float()
    corrupt = {}
    c = wf.clone(); c[200, 300] += spacing[200, 300]
    corrupt["1 one element moved by one bf16 spacing"] = c.to(BF)
    trunc = (v.float().view(torch.int32) & ~0xFFFF).view(F32).to(BF)
    corrupt["3 truncation instead of round-to-nearest-even"] = trunc
    bits = v.float().view(torch.int32)
    away = torch.where((bits & 0xFFFF) == 0x8000, ((bits + 0x8000) & ~0xFFFF).view(F32), wf).to(BF)
    corrupt["4 ties rounded away from zero"] = away
    drop = v.clone()
    drop[160:176, 272:288] -= o["A"][160:176, 64:128].double() @ o["B"][272:288, 64:128].double().T
    corrupt["5 one K tile of 64 dropped for one 16x16 block"] = X.want_bf16(drop)
    small = X.int_f32((N,), 1, 701)
    vs = X.exact_gemm(o["A"], o["B"], small)
    shifted = small.clone(); shifted[N - 4:] = small[N - 8:N - 4]
    assert not torch.equal(shifted, small)
    # 2 on the small-bias output (with +-1000 of bias per column a neighbour's value is far off and rel-L2 sees it): the row of the last
    # column whose distance to its neighbour is the median one
    ws = X.want_bf16(vs)
    dist = (ws[:, N - 1].float() - ws[:, N - 2].float()).abs()
    row = int(dist.argsort()[M // 2])
    c = ws.clone(); c[row, N - 1] = c[row, N - 2]
    corrupt["2 one element of the last ragged column replaced by its neighbour"] = c
    accepted = {}
    for name, bad in corrupt.items():
        base = ws if name[0] == "2" else want
        assert int((bad.view(torch.int16) != base.view(torch.int16)).sum()) > 0, name
        accepted[name[0]] = rel(bad, base) <= TOL_BF
        msg = X.bits_mismatch(name, bad, base)
        assert msg is not None and "differ in bits" in msg, name
        if name[0] == "2":
            assert f"({row}, {N - 1})" in msg and "only in the last partial column tile" in msg
        with pytest.raises(AssertionError):
            X.assert_bits_equal(name, bad, base)
    assert accepted == {"1": True, "2": True, "3": True, "4": True, "5": True}, accepted
    # 6: small bias -> accepted by rel-L2; wide bias -> rejected by it; the comparator rejects both and confines them to the last column tile
    bad6 = X.want_bf16(X.exact_gemm(o["A"], o["B"], shifted))
    assert rel(bad6, X.want_bf16(vs)) <= TOL_BF
    msg = X.bits_mismatch("6 bias shifted by four columns in the last partial tile", bad6, X.want_bf16(vs))
    assert msg is not None and "only in the last partial column tile" in msg and "(0, 2)" in msg
    wide_shift = o["bias"].clone(); wide_shift[N - 4:] = o["bias"][N - 8:N - 4]
    assert rel(X.want_bf16(X.exact_gemm(o["A"], o["B"], wide_shift)), want) > TOL_BF
    # the fp32 bound cannot tell a different summation order from one term counted twice with a tiny weight: one product of one element
    v32 = X.want_f32(v)
    twice = v32.clone(); twice[300, 100] += 1.0
    assert rel(twice, v32) <= TOL_F32 and X.bits_mismatch("one product counted twice", twice, v32) is not None


def test_the_comparator_localises_and_names_untouched_prefill():
    want = torch.arange(300 * 260, dtype=F32).reshape(300, 260)
    got = want.clone()
    got[256:, 256:] = float("nan")
    msg = X.bits_mismatch("corner", got, want, tile=(256, 256))
    assert "176 of 78000" in msg and "[(1, 1)]" in msg and "only in the last partial row tile, only in the last partial column tile" in msg
    assert "176 of them are untouched NaN prefill: tile not written" in msg and "(256, 256): got nan want 66816.0" in msg
    got = want.clone(); got[3, 7] = -1.0; got[140, 200] = 5.0
    msg = X.bits_mismatch("inner", got, want, tile=(128, 128))
    assert "2 of 78000" in msg and "[(0, 0), (1, 1)]" in msg and "not confined" in msg and "prefill" not in msg
    assert X.bits_mismatch("same", want, want.clone()) is None
    nz = torch.zeros(4, 4); mz = -nz
    assert X.bits_mismatch("signed zero", mz, nz) is not None                 # bits, not values
    f = X.Failures(); f.bits("a", want, want.clone()); f.done()
    f.bits("b", got, want)
    with pytest.raises(AssertionError, match="1 failing combinations"):
        f.done()


# ------------------------------------------------------------------------------------------------ the non-linear epilogues' inputs
ACT_CPU_SHARE = {}


@pytest.mark.parametrize("epi", [3, 7, 8])
def test_plain_fp32_activations_stay_inside_the_bound_and_the_share(epi):
    """The GPU check of epilogues 3 / 7 / 8 allows one bf16 spacing + 8 * 2^-23 * max |pre| per element and 1 % of elements that differ from
    bf16(float64 activation) at all.  A plain fp32 evaluation of the same formulas on the same exact pre-activations must fit -- on every
    triple -- or the inputs are wrong (not the cap)."""
    worst = 0.0
    for M, N, K in X.TRIPLES:
        pre = X.act_case(M, N, K, 300 + epi, epi)["pre"]
        assert float(pre.abs().max()) <= 16.0
        got = X.act32(pre, epi, N).to(BF)
        msg, share = X.activation_mismatch(f"fp32 epi {epi} [{M},{N},{K}]", got, pre, epi, N)
        assert msg is None, msg
        if M * N >= X.CENSUS_MIN_ELEMENTS:
            worst = max(worst, share)
            assert float((pre < 0).double().mean()) > 0.05 and pre.unique().numel() > 100          # both signs, many distinct values
    ACT_CPU_SHARE[epi] = worst
    print(f"epi {epi}: largest share of elements differing from bf16(float64) under plain fp32: {worst:.3%}")
    assert worst <= X.ACT_MAX_SHARE / 2                                        # room for a kernel's own exp / erf


def test_every_other_gpu_case_family_meets_its_preconditions():
    """The operands of the remaining GPU cases (non-linear epilogues behind the fold, the 192-row forms, the persistent tile loop) pass the
    2^24 precondition, the rounding census and the [-16, 16] range -- so an ExactnessError can never be what fails on the GPU."""
    for M, N, K in X.TRIPLES:
        for epi in (3, 7, 8):
            a = X.act_case(M, N, K, 320 + epi, epi, fold=True)
            for pre in (a["pre_ln"], a["pre"]):
                msg, share = X.activation_mismatch(f"fp32 ln epi {epi} [{M},{N},{K}]", X.act32(pre, epi, N).to(BF), pre, epi, N)
                assert msg is None and (M * N < X.CENSUS_MIN_ELEMENTS or share <= X.ACT_MAX_SHARE / 2), (msg, share)
    for M, N, K in X.BM192_SHAPES:
        o = X.operands(M, N, K, seed=800)
        X.assert_rounding_is_tested("bm192", X.exact_gemm(o["A"], o["B"], o["bias"]))
        X.exact_gemm(o["A"], o["B"], o["bias"], o["res"])
        a = X.operands(M, N, K, seed=810, profile="act", rows_b=2 * N)
        pre = X.exact_gemm(a["A"], a["B"], a["bias"])
        assert X.activation_mismatch("bm192", X.act32(pre, 3, N).to(BF), pre, 3, N)[0] is None
    for N in (1100, 1120):
        o = X.operands(1300, N, 128, seed=900)
        X.assert_rounding_is_tested("persistent", X.exact_gemm(o["A"], o["B"], o["bias"]))
    for N in (548, 576):
        a = X.operands(1300, N, 128, seed=910, profile="act", rows_b=2 * N)
        pre = X.exact_gemm(a["A"], a["B"], a["bias"])
        assert X.activation_mismatch("persistent", X.act32(pre, 3, N).to(BF), pre, 3, N)[0] is None
