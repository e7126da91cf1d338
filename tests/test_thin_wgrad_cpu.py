"""`-m "not gpu"`: epilogue 12 of cs_gemm_nt (the thin layers' weight and bias gradient) and what is built on it, on the CPU backend
tests/_thin_wgrad_ref.RefOpsThinWgrad: the restatement itself against float64, every planted error rejected, Conv1x1Thin / thin_heads /
FCNMaskHead's tail / LinearThin on the direct route bit for bit against float64 autograd, today's calls where the backend lacks
THIN_WGRAD, LinearThin's dispatch and state dict, ConvFCBBoxHead's fc_reg."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _fc_ref
from _thin_ref import BF, F32, LAYER_SHAPES, LAYOUTS, RefOpsThin, check_exact, check_thin
from _thin_wgrad_ref import (WGRAD_FLAWS, Counting, RefOpsThinWgrad, check_linear, check_result, dy_forms, linear_thin, operands, rounding_case,
                             run_linear)

GEOMS = [(3, 5, 7), (2, 4, 4), (1, 1, 1), (2, 16, 8), (2, 3, 4)]


@pytest.fixture(scope="module")
def ops():
    return RefOpsThinWgrad()


@pytest.fixture(autouse=True)
def direct_route_on(monkeypatch):
    """The switch forced on, whatever the measurement set it to: these tests are about the route, not about its default."""
    from clipself_amd import conv
    monkeypatch.setattr(conv, "THIN_WGRAD_DEFAULT", True)


def _call(ops, x, dy, form, xdt=F32, accumulate_into=None):
    """One thin_wgrad on `ops` -> (dW [N, K], db [N], workspace)."""
    name, R, d1, d2 = form
    M, K = x.shape
    N = dy.shape[1]
    dW = torch.full((16, K + 4), float("nan")) if accumulate_into is None else accumulate_into
    ws = torch.full((ops.thin_wgrad_workspace(M, N, K),), float("nan"))
    ops.thin_wgrad(d1, x.to(xdt), dW[:N, :K], R=R, dY2=d2, workspace=ws)
    assert bool(torch.isnan(dW[N:]).all()) and bool(torch.isnan(dW[:, K:]).all()), "rows >= N or columns >= K were touched"
    assert float(ws[N:16].abs().sum()) == 0
    return dW[:N, :K].clone(), ws[:N].clone(), ws


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("N,K", [(1, 64), (3, 256), (15, 64), (16, 320), (12, 256), (4, 64)])
def test_restatement_against_float64(ops, N, K, kind):
    for B, h, w in GEOMS:
        M, R = B * h * w, h * w
        x, dy = operands(M, N, K, kind)
        for form in dy_forms(dy, R, N):
            for xdt in (F32, BF):
                xin = x.to(xdt).to(F32)
                dw, db, _ = _call(ops, xin, dy, form, xdt)
                check_result(dw, db, xin, dy, kind, f"ref {kind} M={M} N={N} K={K} {form[0]} {xdt}")


def test_restatement_rounds_dy_and_overwrites(ops):
    x, dy = rounding_case()
    for form in dy_forms(dy, 35, 15):
        dw, db, _ = _call(ops, x, dy, form)
        check_result(dw, db, x, dy, "exact", f"rounding {form[0]}")
    with pytest.raises(ValueError):
        ops.thin_wgrad(dy, x, torch.empty(15, 64), workspace=torch.empty(ops.thin_wgrad_workspace(105, 15, 64) - 1))
    with pytest.raises(ValueError):
        ops.thin_wgrad(dy, x, torch.empty(15, 64), workspace=torch.empty(ops.thin_wgrad_workspace(105, 15, 64), dtype=torch.float64))


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _checks(ops):
    """The kernel-level checks of tests/test_gpu_thin_wgrad.py on a backend: exact + random operands on the ragged geometry in every
    form, fp32 X that bf16 does not hold, the dY-rounding case, the overwrite, and a case with more than one workgroup."""
    def run():
        for kind in ("exact", "random"):
            x, dy = operands(105, 15, 64, kind)
            for form in dy_forms(dy, 35, 15):
                dw, db, _ = _call(ops, x, dy, form)
                check_result(dw, db, x, dy, kind, "planted")
        x, dy = rounding_case()
        dw, db, _ = _call(ops, x, dy, dy_forms(dy, 35, 15)[0])
        check_result(dw, db, x, dy, "exact", "planted rounding")
        x, dy = operands(2 * 128 + 1, 3, 64, "ternary")                  # three workgroups, the last one ragged
        dw, db, _ = _call(ops, x, dy, dy_forms(dy, 257, 3)[1])
        check_result(dw, db, x, dy, "ternary", "planted partials")
        x, dy = operands(32, 4, 64, "exact")                             # dW is overwritten: a second call into the first one's result
        buf = torch.full((16, 68), float("nan"))
        _call(ops, x, dy, dy_forms(dy, 16, 4)[0], accumulate_into=buf)
        dw, db, _ = _call(ops, x, dy, dy_forms(dy, 16, 4)[0], accumulate_into=buf)
        check_result(dw, db, x, dy, "exact", "planted overwrite")
    return run


def test_clean_restatement_passes_the_checks(ops):
    _checks(ops)()


@pytest.mark.parametrize("flaw", WGRAD_FLAWS)
def test_every_planted_error_is_rejected(flaw):
    assert _fails(_checks(RefOpsThinWgrad(flaws=(flaw,)))), f"the checks accept the planted error {flaw!r}"


# ------------------------------------------------------------------------------------------------ the layers on the direct route
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_conv1x1thin_direct_route(ops, shape, layout, dtype, kind):
    check_thin(ops, shape, layout, dtype, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape,widths", [((105, 64, 15), [3, 12]), ((32, 256, 16), [4, 12]), ((256, 320, 12), [11, 1])])
def test_thin_heads_pair_direct_route(ops, shape, widths, layout, dtype, kind):
    check_thin(ops, shape, layout, dtype, kind, widths=widths)


@pytest.mark.parametrize("kind", ["rpn2", "mask"])
def test_modules_exact_on_the_direct_route(kind):
    c = Counting(direct=True)
    check_exact(kind, c)
    assert c.calls["thin_wgrad"] >= 1


def test_flawed_backend_fails_the_layer_checks():
    for flaw in ("second_block_first_width", "ragged_tail_dropped", "partial_dropped"):
        bad = RefOpsThinWgrad(flaws=(flaw,))
        assert _fails(lambda: check_thin(bad, (105, 64, 15), "nchw", F32, "exact", widths=[3, 12])), flaw


# ------------------------------------------------------------------------------------------------ which calls are made
def _thin_calls(c, widths, dtype=F32, layout="channel_last"):
    check_thin(c, (105, 64, 15), layout, dtype, "exact", widths=widths)
    return c.calls


def test_without_the_flag_todays_calls_are_made_and_with_it_none_of_them():
    old = _thin_calls(Counting(direct=False), [3, 12])
    assert old["colsum_bf16"] == 1 and old["gemm_wgrad_tn"] + old["gemm_wgrad"] == 1 and old["thin_wgrad"] == 0
    assert old["cast_f32_bf16"] == 1 and old["nchw_to_rows"] == 2        # the fp32 map's cast and dy_rows16's two permutations
    new = _thin_calls(Counting(direct=True), [3, 12])
    assert new["colsum_bf16"] == 0 and new["gemm_wgrad_tn"] + new["gemm_wgrad"] == 0 and new["thin_wgrad"] == 1
    assert new["cast_f32_bf16"] == 0 and new["nchw_to_rows"] == 0
    plain = RefOpsThin()                                                 # the backend of tests/_thin_ref: no THIN_WGRAD, no thin_wgrad at all
    assert not hasattr(plain, "thin_wgrad")
    check_thin(plain, (105, 64, 15), "channel_last", F32, "exact", widths=[3, 12])


def test_the_default_switch_selects_the_route(monkeypatch):
    from clipself_amd import conv
    monkeypatch.setattr(conv, "THIN_WGRAD_DEFAULT", False)
    off = _thin_calls(Counting(direct=True), [15])
    assert off["thin_wgrad"] == 0 and off["colsum_bf16"] == 1
    monkeypatch.setattr(conv, "THIN_WGRAD_DEFAULT", True)
    on = _thin_calls(Counting(direct=True), [15])
    assert on["thin_wgrad"] == 1 and on["colsum_bf16"] == 0


def test_mask_tail_calls():
    from clipself_amd import conv
    old, new = Counting(direct=False), Counting(direct=True)
    check_exact("mask", old)
    check_exact("mask", new)
    # the tail's own colsum (the deconvolution's bias) stays; conv_logits' one goes
    assert old.calls["thin_wgrad"] == 0 and new.calls["thin_wgrad"] == 1
    assert new.calls["colsum_bf16"] == old.calls["colsum_bf16"] - 1
    assert new.calls["gemm_wgrad_tn"] + new.calls["gemm_wgrad"] == old.calls["gemm_wgrad_tn"] + old.calls["gemm_wgrad"] - 1
    assert conv.FUSED_THIN_DEFAULT is False


def test_a_frozen_weight_still_gets_its_bias_gradient(ops):
    x, w, b, dy, ref = _fc_ref.case((105, 64, 15), "exact", act=None)
    from _thin_ref import run_thin, same_bits, thin_layers
    mods = thin_layers(ops, w, b, [3, 12])
    mods[0].weight.requires_grad_(False)
    inp = x.view(3, 5, 7, 64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    from clipself_amd.conv import thin_heads
    ys = thin_heads(inp, mods)
    gs = [dy[:, :3].reshape(3, 5, 7, 3).permute(0, 3, 1, 2).contiguous(), dy[:, 3:].reshape(3, 5, 7, 12).permute(0, 3, 1, 2).contiguous()]
    torch.autograd.backward(ys, gs)
    assert mods[0].weight.grad is None
    same_bits(torch.cat([mods[0].bias.grad, mods[1].bias.grad]), ref["db"], "db with a frozen weight")
    same_bits(mods[1].weight.grad.view(12, 64), ref["dw"][3:], "dw of the second module")


# ------------------------------------------------------------------------------------------------ LinearThin
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("shape", [(105, 64, 4), (1, 64, 1), (300, 512, 4), (33, 320, 16)])
def test_linear_thin_against_float64_autograd(ops, shape, dtype, kind):
    check_linear(ops, shape, kind, dtype)


def test_linear_thin_3d_input_and_both_routes():
    for c in (Counting(direct=True), Counting(direct=False)):
        check_linear(c, (300, 512, 4), "exact", F32, view=(2, 150, 512))
        check_linear(c, (300, 512, 4), "exact", BF)
        assert (c.calls["thin_wgrad"] > 0) == c.THIN_WGRAD and (c.calls["colsum_bf16"] > 0) != c.THIN_WGRAD


def test_linear_thin_state_dict_and_dispatch(ops):
    from clipself_amd.linear import LinearThin
    torch.manual_seed(3)
    a = LinearThin(128, 4, ops=ops, fused=True)
    torch.manual_seed(3)
    b = nn.Linear(128, 4)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    x = torch.randn(7, 128)
    plain = LinearThin(128, 4)
    plain.load_state_dict(b.state_dict())
    assert torch.equal(plain(x), F.linear(x, b.weight, b.bias))          # no backend: F.linear's bits
    none =LinearThin(128, 4, ops=ops, fused=None)                       # FUSED_THIN_DEFAULT is off: torch
    none.load_state_dict(b.state_dict())
    assert torch.equal(none(x), F.linear(x, b.weight, b.bias))
    y = a(x)
    assert y.dtype == F32 and "LinearThin" in type(y.grad_fn).__name__
    assert a(x.to(BF)).dtype == F32                                      # fp32 out whatever the input's dtype
    with pytest.raises(NotImplementedError):
        LinearThin(128, 20, ops=ops, fused=True)(x)
    with pytest.raises(NotImplementedError):
        LinearThin(100, 4, ops=ops, fused=True)(torch.randn(7, 100))
    class NoThin(RefOpsThinWgrad):
        THIN_HEADS = False
    with pytest.raises(NotImplementedError):
        LinearThin(128, 4, ops=NoThin(), fused=True)(x)


def test_linear_thin_repacks_after_a_step(ops):
    x, w, b, dy, _ = _fc_ref.case((105, 64, 4), "exact", act=None)
    m = linear_thin(ops, w, b)
    y0 = run_linear(m, x, dy)[0]
    with torch.no_grad():
        m.weight.mul_(2)
    assert torch.equal(run_linear(m, x, dy)[0] - b, 2 * (y0 - b))


# ------------------------------------------------------------------------------------------------ ConvFCBBoxHead
HEAD = dict(in_channels=64, conv_out_channels=64, fc_out_channels=64, roi_feat_size=7, num_classes=5, norm_cfg=dict(type="SyncBN"),
            num_shared_convs=1, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1)


def test_bbox_head_builds_linear_thin_for_class_agnostic_regression(ops):
    from clipself_amd.bbox_head import ConvFCBBoxHead
    from clipself_amd.linear import LinearThin
    torch.manual_seed(5)
    h = ConvFCBBoxHead(ops=ops, fused=True, reg_class_agnostic=True, **HEAD)
    assert isinstance(h.fc_reg, LinearThin) and h.fc_reg.fused is None and h.fc_reg.out_features == 4
    wide = ConvFCBBoxHead(ops=ops, fused=True, reg_class_agnostic=False, **HEAD)
    assert type(wide.fc_reg) is nn.Linear and wide.fc_reg.out_features == 20
    odd = ConvFCBBoxHead(ops=ops, fused=True, reg_class_agnostic=True, **{**HEAD, "fc_out_channels": 72})
    assert type(odd.fc_reg) is nn.Linear                                 # 72 % 64 != 0
    # a reference-keyed state dict: plain tensors under mmdet's names
    torch.manual_seed(5)
    twin = ConvFCBBoxHead(ops=None, fused=False, reg_class_agnostic=True, **HEAD)
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    assert "fc_reg.weight" in sd and "fc_reg.bias" in sd
    h.load_state_dict(sd, strict=True)
    twin.load_state_dict(h.state_dict(), strict=True)
    # fused=True, fused_reg=None: bbox_pred is F.linear of the x_reg the layer saw, bit for bit
    seen = {}
    h.fc_reg.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach().clone()))
    x = torch.randn(6, 64, 7, 7, generator=torch.Generator().manual_seed(6)).to(BF).to(F32)
    _, pred = h(x)
    assert torch.equal(pred, F.linear(seen["x"], h.fc_reg.weight, h.fc_reg.bias)) and "LinearThin" not in type(pred.grad_fn).__name__
    k = ConvFCBBoxHead(ops=ops, fused=True, fused_reg=True, reg_class_agnostic=True, **HEAD)
    k.load_state_dict(sd, strict=True)
    _, pred_k = k(x)
    assert pred_k.dtype == F32 and "LinearThin" in type(pred_k.grad_fn).__name__
    pred_k.sum().backward()
    assert k.fc_reg.weight.grad is not None and k.fc_reg.bias.grad is not None
    assert torch.equal(k.fc_reg.bias.grad, torch.full((4,), 6.0))
