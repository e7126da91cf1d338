"""`-m gpu`: read and write extents of every kernel behind the C ABI (include/clipself_hip.h).

test_extents: each case of tests/_extents.py on tensors that are views inside NaN / sentinel halos with a padded row stride, bit for bit
against the same op on compact clean tensors, and every halo byte of every output and workspace unchanged (the harness and what it can
see: tests/_extents.py; its own checks: tests/test_extents_harness_cpu.py).

test_layernorm_ragged_*: LayerNorm rows that end inside a 4-element vector (C % 4 != 0: 2730 hidden units in 2752-wide storage) with NaN
in every pad column of x, dy, gamma and beta, against an fp64 LayerNorm of the C real columns at the bounds of test_layernorm_fwd_bwd.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import CASES, run_case, up  # noqa: E402
from test_gpu_ops import BF, F32, TOL_BF, TOL_F32, check, rnd  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("name", list(CASES))
def test_extents(hip, name, pad):
    problems = run_case(hip, CASES[name], "cuda", pad, key=name)
    assert not problems, f"{name} (row strides + {pad}):\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ LayerNorm, C % 4 != 0
_LN = {}


def _ln_ref(M, C, xdt):
    """fp64 LayerNorm forward / backward of the C real columns; computed once per shape and shared."""
    key = (M, C, xdt)
    if key not in _LN:
        x = (rnd((M, C), F32, 2.0, seed=20) + 0.5).to(xdt)
        gamma, beta = 1 + rnd((C,), F32, 0.2, seed=21), rnd((C,), F32, 0.2, seed=22)
        dy = rnd((M, C), BF, seed=23)
        xd, g, d = x.double(), gamma.double(), dy.double()
        mu = xd.mean(-1, keepdim=True)
        r = torch.rsqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
        xh = (xd - mu) * r
        gy = d * g
        dx = r * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
        _LN[key] = dict(x=x, gamma=gamma, beta=beta, dy=dy, y=xh * g + beta.double(), mean=mu[:, 0], rstd=r[:, 0], dx=dx,
                        dgamma=(d * xh).sum(0), dbeta=d.sum(0))
    return _LN[key]


def _padded(t, ld, fill=NAN):
    """[M, C] -> the [M, C] view of a [M, ld] device tensor whose other columns hold `fill`; vectors likewise ([C] of [ld])."""
    big = torch.full(t.shape[:-1] + (ld,), fill, dtype=t.dtype, device="cuda")
    big[..., :t.shape[-1]] = t.cuda()
    return big, big[..., :t.shape[-1]]


def _pads_ok(tag, big, C, sentinel_bits):
    """[C, roundup4(C)) exact zeros (include/clipself_hip.h, cs_layernorm_fwd / _bwd), everything from roundup4(C) on untouched."""
    it = {2: torch.int16, 4: torch.int32}[big.element_size()]
    assert int((big[:, C:up(C, 4)].view(it) != 0).sum()) == 0, f"{tag}: columns [C, roundup4(C)) are not exact zeros"
    assert int((big[:, up(C, 4):].view(it) != sentinel_bits).sum()) == 0, f"{tag}: columns past roundup4(C) were written"


def _sentinel(M, ld, dtype):
    """Output rows filled with a NaN pattern; returns (tensor, the pattern as a signed integer)."""
    it, v = (torch.int16, 0x7FA5 - 0x10000 + 0x8000) if dtype == BF else (torch.int32, -0x5A5A5B)
    return torch.full((M, ld), v, dtype=it, device="cuda").view(dtype), v


@pytest.mark.parametrize("xdt", [F32, BF])
@pytest.mark.parametrize("C", [6, 130, 2730])
def test_layernorm_ragged_forward_ignores_nan_padding(hip, C, xdt):
    M, ld = 37, up(C, 8) + 8
    w = _ln_ref(M, C, xdt)
    tag = f"ln_ragged[{C},{'f32' if xdt == F32 else 'bf16'}]"
    _, x = _padded(w["x"], ld)
    _, gamma = _padded(w["gamma"], ld)
    _, beta = _padded(w["beta"], ld)
    ybig, sv = _sentinel(M, ld, BF)
    mean, rstd = torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
    hip.layernorm_fwd(x, gamma, beta, ybig[:, :C], mean, rstd)
    check(tag + ".y", ybig[:, :C], w["y"], TOL_BF)
    check(tag + ".mean", mean, w["mean"], TOL_F32)
    check(tag + ".rstd", rstd, w["rstd"], TOL_F32)
    _pads_ok(tag + ".y", ybig, C, sv)
    # statistics only (y = NULL): the same numbers
    m2, r2 = torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
    hip.layernorm_fwd(x, gamma, beta, None, m2, r2)
    assert torch.equal(m2, mean) and torch.equal(r2, rstd), f"{tag}: statistics-only run differs"
    # with the fused e4m3 copy: y unchanged, codes and scales those of the row quantiser on y, padding bytes zero
    y2big, _ = _sentinel(M, ld, BF)
    Kp = up(C, 128)
    q1, s1 = torch.full((M, Kp + 8), 0x55, dtype=torch.uint8, device="cuda"), torch.full((M,), NAN, device="cuda")
    hip.layernorm_fwd_q8(x, gamma, beta, y2big[:, :C], q1[:, :Kp], s1)
    assert torch.equal(y2big.view(torch.int16), ybig.view(torch.int16)), f"{tag}: y differs under the fused quantiser"
    yc = torch.zeros(M, up(C, 8), dtype=BF, device="cuda")
    yc[:, :C] = ybig[:, :C]
    q0, s0 = torch.full((M, Kp), 0xAA, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    hip.quant_rows_fp8(yc, q0, s0)
    assert torch.equal(s0, s1), f"{tag}: row scales"
    assert torch.equal(q0, q1[:, :Kp]), f"{tag}: {int((q0 != q1[:, :Kp]).sum())} e4m3 codes differ"
    assert int(q1[:, C:Kp].max()) == 0 and int((q1[:, Kp:] != 0x55).sum()) == 0, f"{tag}: e4m3 padding"


@pytest.mark.parametrize("xdt", [F32, BF])
@pytest.mark.parametrize("C", [6, 130, 2730])
def test_layernorm_ragged_backward_ignores_nan_padding(hip, C, xdt):
    M, ld = 37, up(C, 8) + 8
    w = _ln_ref(M, C, xdt)
    tag = f"ln_ragged[{C},{'f32' if xdt == F32 else 'bf16'}]"
    _, x = _padded(w["x"], ld)
    _, dy = _padded(w["dy"], ld)
    _, gamma = _padded(w["gamma"], ld)
    mean, rstd = w["mean"].float().cuda(), w["rstd"].float().cuda()
    ws = torch.empty(hip.layernorm_bwd_workspace(M, C), dtype=torch.uint8, device="cuda")
    base = rnd((M, C), F32, seed=24)
    cs0 = rnd((C,), F32, seed=26)
    Kp = up(C, 128)
    for mode, odt in ((0, BF), (1, F32), (2, F32)):
        want = w["dx"] + (base.double() if mode == 2 else 0)
        tol = TOL_BF if odt == BF else 1e-4

        def fresh():
            big, sv = _sentinel(M, ld, odt)
            if mode == 2:
                big[:, :C] = base.cuda()                    # the pad columns keep the NaN pattern: accumulate mode must not carry it over
            return big, sv

        # parameter gradients written
        dxbig, sv = fresh()
        dg, db = torch.full((ld,), NAN, device="cuda"), torch.full((ld,), NAN, device="cuda")
        hip.layernorm_bwd(dy, x, gamma, mean, rstd, dxbig[:, :C], mode, dg[:C], db[:C], False, ws)
        check(f"{tag}.dx{mode}", dxbig[:, :C], want, tol)
        check(f"{tag}.dgamma{mode}", dg[:C], w["dgamma"], 1e-4)
        check(f"{tag}.dbeta{mode}", db[:C], w["dbeta"], 1e-4)
        _pads_ok(f"{tag}.dx{mode}", dxbig, C, sv)
        assert bool(torch.isnan(dg[C:]).all()) and bool(torch.isnan(db[C:]).all()), f"{tag}: dgamma / dbeta written past C"
        # frozen parameters: the same dx
        dx2, _ = fresh()
        hip.layernorm_bwd(dy, x, gamma, mean, rstd, dx2[:, :C], mode)
        assert torch.equal(dx2[:, :C], dxbig[:, :C]), f"{tag}.dx{mode}: frozen form differs"
        if mode == 0:
            continue
        # bf16 copy + its column sums (accumulated) [+ the e4m3 copy]
        for q8 in (False, True):
            dx3, _ = fresh()
            cbig, csv = _sentinel(M, ld, BF)
            cs = torch.full((ld,), NAN, device="cuda")
            cs[:C] = cs0.cuda()
            dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            kw = {}
            if q8:
                q1, s1 = torch.full((M, Kp + 8), 0x55, dtype=torch.uint8, device="cuda"), torch.full((M,), NAN, device="cuda")
                kw = dict(q8=q1[:, :Kp], q_scale=s1)
            hip.layernorm_bwd(dy, x, gamma, mean, rstd, dx3[:, :C], mode, dg, db, True, ws, dx_copy=cbig[:, :C], copy_colsum=cs[:C], **kw)
            sub = f"{tag}.copy{'+q8' if q8 else ''}"
            check(f"{sub}.dx{mode}", dx3[:, :C], want, 1e-4)
            check(f"{sub}.dgamma{mode}", dg, w["dgamma"], 1e-4)
            assert torch.equal(cbig[:, :C], dx3[:, :C].to(BF)), f"{sub}: the copy is the rounded stream"
            check(f"{sub}.colsum{mode}", cs[:C] - cs0.cuda(), cbig[:, :C].double().sum(0), 1e-4)
            assert bool(torch.isnan(cs[C:]).all()), f"{sub}: copy_colsum written past C"
            _pads_ok(f"{sub}.dx{mode}", dx3, C, -0x5A5A5B)
            _pads_ok(f"{sub}.dx_copy{mode}", cbig, C, csv)
            if q8:
                cc = torch.zeros(M, up(C, 8), dtype=BF, device="cuda")
                cc[:, :C] = cbig[:, :C]
                q0, s0 = torch.full((M, Kp), 0xAA, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
                hip.quant_rows_fp8(cc, q0, s0)
                assert torch.equal(s0, s1) and torch.equal(q0, q1[:, :Kp]), f"{sub}: e4m3 copy != quant_rows_fp8(dx_copy)"
                assert int(q1[:, C:Kp].max()) == 0 and int((q1[:, Kp:] != 0x55).sum()) == 0, f"{sub}: e4m3 padding"
