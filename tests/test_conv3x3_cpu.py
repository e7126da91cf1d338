"""CPU: conv.Conv3x3 -- the detector heads' 3 x 3 convolutions -- on the reference backend (tests/_conv_ref.RefOpsConv): the packing of the
weights, the state dict, the module's kernel route and autograd function on both routes (exact operands bit for bit against float64
autograd, random operands inside the derived bounds), the fallbacks, and that the checks reject planted errors."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _conv_ref import (BF, F32, ROUTES, SHAPE_IDS, SHAPES, RefOpsConv, bounds, case, check_bound, index_conv3x3, index_im2col, layer,
                       map_of, rne_bf16, rows_of, run_layer, same_bits)
from clipself_amd import conv as C
from clipself_amd.conv import Conv3x3, pack_weights

SMALL = SHAPES[:5]                      # the 33 x 17 map adds nothing the index expressions could get wrong; it runs on the GPU
SMALL_IDS = SHAPE_IDS[:5]


@pytest.fixture(scope="module")
def ops():
    return RefOpsConv()


# ------------------------------------------------------------------------------------------------ operands and state
def test_packing_of_wg_and_wgt():
    w = torch.randn(16, 64, 3, 3, generator=torch.Generator().manual_seed(1)).to(BF).to(F32)
    Wg, WgT = pack_weights(w)
    assert Wg.dtype == BF and tuple(Wg.shape) == (16, 9 * 64) and WgT.dtype == BF and tuple(WgT.shape) == (64, 9 * 16)
    for co, ci, ky, kx in [(0, 0, 0, 0), (3, 7, 0, 2), (15, 63, 2, 1), (9, 31, 1, 1), (4, 5, 2, 0)]:
        t = ky * 3 + kx
        assert float(Wg[co, t * 64 + ci]) == float(w[co, ci, ky, kx])
        assert float(WgT[ci, t * 16 + co]) == float(w[co, ci, 2 - ky, 2 - kx])
    # every element, by the definition's loops
    want = torch.stack([w[:, :, t // 3, t % 3] for t in range(9)], 1).reshape(16, 9 * 64)           # [co, t, ci]
    assert torch.equal(Wg.float(), want)
    wantT = torch.stack([w[:, :, 2 - t // 3, 2 - t % 3].T for t in range(9)], 1).reshape(64, 9 * 16)  # [ci, t, co]
    assert torch.equal(WgT.float(), wantT)


def test_state_dict_loads_strictly_both_ways_and_parameters_match_conv2d():
    torch.manual_seed(3)
    ref = nn.Conv2d(64, 16, 3, padding=1)
    torch.manual_seed(3)
    m = Conv3x3(64, 16)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), ref.parameters()))                  # the same initialisation
    ref2 = nn.Conv2d(64, 16, 3, padding=1)
    m.load_state_dict(ref2.state_dict(), strict=True)
    assert torch.equal(m.weight, ref2.weight) and torch.equal(m.bias, ref2.bias)
    back = nn.Conv2d(64, 16, 3, padding=1)
    back.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(back.weight, ref2.weight)
    nb = Conv3x3(64, 16, bias=False)
    nb.load_state_dict(nn.Conv2d(64, 16, 3, padding=1, bias=False).state_dict(), strict=True)
    for bad in (dict(kernel_size=1, padding=0), dict(stride=2), dict(padding=0), dict(dilation=2, padding=2), dict(groups=2),
                dict(padding_mode="reflect")):
        with pytest.raises(AssertionError):
            Conv3x3(64, 16, **bad)
    with pytest.raises(AssertionError):
        Conv3x3(64, 16, route="winograd")


def test_packed_weights_follow_the_version_counters(ops):
    x, w, b, dy, _ = case(SHAPES[1], "exact")
    m = layer(ops, w, b, fused=True)
    a = m.gemm_weights()
    assert m.gemm_weights()[0] is a[0]                                  # cached
    with torch.no_grad():
        m.weight.mul_(2)
    assert torch.equal(m.gemm_weights()[0].float(), a[0].float() * 2)   # rebuilt
    with torch.no_grad():
        m.bias.add_(1)
    assert torch.equal(m.gemm_weights()[2], b + 1)


# ------------------------------------------------------------------------------------------------ the reference ops themselves
@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_index_expressions_are_torch_conv2d(shape):
    """The CPU backend's ops, written from the header, against F.conv2d on exact operands (every element, bit for bit), and the explicit
    matrix against F.unfold."""
    N, H, W, Cin, Cout = shape
    x, w, b, dy, ref = case(shape, "exact")
    Wg, _ = pack_weights(w)
    y = index_conv3x3(rows_of(x), Wg, b, N, H, W, F32)
    same_bits(map_of(y, N, H, W).contiguous(), ref["y"].to(F32), "index_conv3x3")
    cols = index_im2col(rows_of(x), N, H, W, 0, N * H * W)
    unf = F.unfold(x, 3, padding=1).reshape(N, Cin, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * Cin)   # [n, p, t, ci]
    assert torch.equal(cols.float(), unf)
    r0 = (N * H * W) // 3
    assert torch.equal(index_im2col(rows_of(x), N, H, W, r0, N * H * W - r0), cols[r0:])


# ------------------------------------------------------------------------------------------------ the layer on the reference backend
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_exact_operands_bit_for_bit(ops, shape, route):
    x, w, b, dy, ref = case(shape, "exact")
    m = layer(ops, w, b, fused=True, route=route)
    y, dx, dw, db = run_layer(m, x, dy)
    assert y.dtype == F32 and dx.dtype == F32 and dw.dtype == F32 and db.dtype == F32 and tuple(dw.shape) == tuple(w.shape)
    assert y.permute(0, 2, 3, 1).is_contiguous() and dx.shape == x.shape                 # channel-last out of channel-last in
    for k, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        same_bits(got, ref[k].to(F32), f"{route} {k}")
    yb, dxb, dwb, dbb = run_layer(m, x, dy, dtype=BF)
    assert yb.dtype == BF and dxb.dtype == BF and dwb.dtype == F32
    same_bits(yb, rne_bf16(ref["y"]), f"{route} bf16 y")
    same_bits(dxb, rne_bf16(ref["dx"]), f"{route} bf16 dx")
    same_bits(dwb, ref["dw"].to(F32), f"{route} dw of a bf16 input")
    again = run_layer(m, x, dy, channel_last=False)                                      # an NCHW-contiguous input, and the same bits
    assert all(torch.equal(a, c) for a, c in zip((y, dx, dw, db), again))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_random_operands_within_the_derived_bounds(ops, shape, route):
    x, w, b, dy, ref = case(shape, "random")
    m = layer(ops, w, b, fused=True, route=route)
    for dtype in (F32, BF):
        got = dict(zip(("y", "dx", "dw", "db"), run_layer(m, x, dy, dtype=dtype)))
        tol = bounds(ref, shape, bf16_out=dtype == BF)
        for k in ("y", "dx", "dw", "db"):
            check_bound(f"{route} {dtype} {k}", got[k], ref[k], tol[k])


def test_inputs_of_any_strides_and_frozen_parameters(ops):
    shape = SHAPES[1]
    N, H, W, Cin, Cout = shape
    x, w, b, dy, ref = case(shape, "exact")
    m = layer(ops, w, b, fused=True)
    wide = torch.zeros(N, Cin + 8, H, W + 3)
    wide[:, 4:4 + Cin, :, 1:1 + W] = x
    view = wide[:, 4:4 + Cin, :, 1:1 + W].requires_grad_(True)                           # neither NCHW-contiguous nor channel-last
    y = m(view)
    same_bits(y, ref["y"].to(F32), "strided input")
    for p in m.parameters():
        p.requires_grad_(False)
    xin = x.clone().requires_grad_(True)
    m(xin).backward(dy)
    same_bits(xin.grad, ref["dx"].to(F32), "dx with frozen parameters")
    assert m.weight.grad is None and m.bias.grad is None
    with torch.no_grad():
        same_bits(m(x), ref["y"].to(F32), "no_grad forward")


# ------------------------------------------------------------------------------------------------ dispatch
def test_fallbacks_and_fused_true_outside_the_coverage(ops, monkeypatch):
    x, w, b, dy, ref = case(SHAPES[1], "exact")
    called = []
    spy = RefOpsConv()
    spy.conv3x3 = lambda *a, **k: called.append("conv3x3") or RefOpsConv.conv3x3(spy, *a, **k)
    # fused=False: torch's convolution, whatever the backend
    m = layer(spy, w, b, fused=False)
    y = m(x)
    assert not called and type(y.grad_fn).__name__ != "_Conv3x3FnBackward"
    same_bits(y.detach(), ref["y"].to(F32), "fused=False")
    # a CPU tensor on the product's own lookup (no backend handed in): torch, and fused=True has nothing to run on
    m = layer(None, w, b)
    same_bits(m(x).detach(), ref["y"].to(F32), "CPU tensor")
    with pytest.raises(NotImplementedError):
        layer(None, w, b, fused=True)(x)
    # fused=None follows FUSED_CONV_DEFAULT
    for default in (False, True):
        monkeypatch.setattr(C, "FUSED_CONV_DEFAULT", default)
        called.clear()
        layer(spy, w, b)(x)
        assert bool(called) == default
    # a backend without the flag
    class NoConv(RefOpsConv):
        CONV3X3 = False
    same_bits(layer(NoConv(), w, b)(x).detach(), ref["y"].to(F32), "backend without CONV3X3")
    # Cin = 32: outside the coverage -> torch; fused=True raises
    g = torch.Generator().manual_seed(2)
    x32, w32, b32 = (torch.randint(-8, 9, s, generator=g).float() for s in ((2, 32, 3, 5), (16, 32, 3, 3), (16,)))
    called.clear()
    y32 = layer(spy, w32, b32)(x32)
    assert not called and torch.equal(y32, F.conv2d(x32, w32, b32, padding=1))
    with pytest.raises(NotImplementedError):
        layer(spy, w32, b32, fused=True)(x32)
    with pytest.raises(NotImplementedError):
        layer(spy, torch.zeros(12, 64, 3, 3), torch.zeros(12), fused=True)(x)           # Cout % 8 != 0
    with pytest.raises(NotImplementedError):
        layer(spy, w, b, fused=True)(x.double())


# ------------------------------------------------------------------------------------------------ the checks reject planted errors
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("flaw", ["swap", "no_x", "no_image"])
@pytest.mark.parametrize("route", ROUTES)
def test_checks_reject_a_flawed_gather(flaw, route):
    """ky / kx swapped | no x-range check (a tap wraps to the neighbouring row) | no image-range check (a tap bleeds into image n + 1),
    each planted in a copy of the reference op: the exact check and the bound check both fail, on the forward and on the gradients."""
    shape = SHAPES[1]                                                    # 2 images of 3 x 5: non-square, more than one image
    bad = RefOpsConv()
    bad.flaws = (flaw,)
    for kind in ("exact", "random"):
        x, w, b, dy, ref = case(shape, kind)
        y, dx, dw, db = run_layer(layer(bad, w, b, fused=True, route=route), x, dy)
        tol = bounds(ref, shape)
        for k, got in (("y", y), ("dx", dx), ("dw", dw)):
            if kind == "exact":
                assert _fails(lambda: same_bits(got, ref[k].to(F32), k)), (flaw, route, k)
            else:
                assert _fails(lambda: check_bound(k, got, ref[k], tol[k])), (flaw, route, k)


@pytest.mark.parametrize("route", ROUTES)
def test_checks_reject_unflipped_dgrad_weights(ops, route, monkeypatch):
    def transposed_not_flipped(weight):
        Wg, _ = pack_weights(weight)
        Cout, Cin = weight.shape[:2]
        return Wg, weight.detach().to(BF).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).contiguous()
    monkeypatch.setattr(C, "pack_weights", transposed_not_flipped)
    shape = SHAPES[3]                                                    # Cout % 64 == 0: dgrad on the implicit route too
    for kind in ("exact", "random"):
        x, w, b, dy, ref = case(shape, kind)
        y, dx, dw, db = run_layer(layer(ops, w, b, fused=True, route=route), x, dy)
        if kind == "exact":
            same_bits(y, ref["y"].to(F32), "y")                          # the forward is untouched ...
            assert _fails(lambda: same_bits(dx, ref["dx"].to(F32), "dx"))   # ... the input gradient is not
        else:
            assert _fails(lambda: check_bound("dx", dx, ref["dx"], bounds(ref, shape)["dx"]))


def test_checks_reject_a_bias_added_twice_on_the_im2col_route():
    class TwiceBias(RefOpsConv):
        def gemm_nt(self, A, B, Cm, bias=None, **kw):
            super().gemm_nt(A, B, Cm, None if bias is None else 2 * bias, **kw)
    shape = SHAPES[1]
    for kind in ("exact", "random"):
        x, w, b, dy, ref = case(shape, kind)
        m = layer(TwiceBias(), w, b, fused=True, route="im2col")
        y = m(x).detach()
        if kind == "exact":
            assert _fails(lambda: same_bits(y, ref["y"].to(F32), "y"))
        else:
            assert _fails(lambda: check_bound("y", y, ref["y"], bounds(ref, shape)["y"]))
        good = layer(TwiceBias(), w, b, fused=True, route="implicit")(x).detach()       # the implicit route has no gemm_nt in it
        if kind == "exact":
            same_bits(good, ref["y"].to(F32), "y")
