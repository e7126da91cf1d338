"""CPU: the thin 1 x 1 convolutions and the two heads built on them (conv.Conv1x1Thin, conv.thin_heads, rpn_head.RPNHead,
mask_head.FCNMaskHead) on the reference backend of tests/_thin_ref.py -- state dicts against the torch twins, the reference's config
dicts, exact operands bit for bit against float64 autograd, random operands inside the derived bounds, dispatch, the wrappers'
packing, and the six planted errors the exact checks reject."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _thin_ref import (BF, F32, FLAWS, KINDS, LAYER_SHAPES, LAYOUTS, PARITY_REL_L2, REFERENCE_MASK_HEAD, REFERENCE_RPN_HEAD, RefOpsThin,
                       TwinMaskHead, TwinRPNHead, check_dy_rounding, check_exact, check_thin, make_module, make_twin, parity, random_case,
                       run_module)
from clipself_amd import conv as conv_mod
from clipself_amd.conv import Conv1x1, Conv1x1Thin, Conv3x3, thin_heads
from clipself_amd.mask_head import FCNMaskHead
from clipself_amd.neck import Deconv2x2
from clipself_amd.norm_act import BatchNormAct2d, ConvModule
from clipself_amd.rpn_head import RPNHead


@pytest.fixture(scope="module")
def ops():
    return RefOpsThin()


# ------------------------------------------------------------------------------------------------ state dicts and configs
@pytest.mark.parametrize("norm_cfg", [None, dict(type="SyncBN", requires_grad=True)], ids=["nonorm", "SyncBN"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_state_dict_is_the_twins_strict_both_ways(kind, norm_cfg):
    m, (twin, _) = make_module(kind, None, fused=None, norm_cfg=norm_cfg), make_twin(kind, norm_cfg=norm_cfg)
    assert list(m.state_dict()) == list(twin.state_dict())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in twin.state_dict().items()}
    twin.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(twin.state_dict(), strict=True)
    keys = set(m.state_dict())
    if kind == "rpn2":
        assert {"rpn_conv.0.conv.weight", "rpn_conv.1.conv.weight", "rpn_cls.weight", "rpn_cls.bias", "rpn_reg.weight", "rpn_reg.bias"} <= keys
        assert ("rpn_conv.0.bn.running_mean" in keys) == (norm_cfg is not None) and ("rpn_conv.0.conv.bias" in keys) == (norm_cfg is None)
    if kind == "rpn1":
        assert {"rpn_conv.weight", "rpn_conv.bias"} <= keys
    if kind == "mask":
        assert {"convs.0.conv.weight", "upsample.weight", "upsample.bias", "conv_logits.weight", "conv_logits.bias"} <= keys
        assert ("convs.1.bn.num_batches_tracked" in keys) == (norm_cfg is not None)


def test_the_references_config_dicts_construct_the_modules():
    rpn = RPNHead(**REFERENCE_RPN_HEAD)
    assert type(rpn.rpn_cls) is Conv1x1Thin and type(rpn.rpn_reg) is Conv1x1Thin and len(rpn.rpn_conv) == 2
    assert tuple(rpn.rpn_cls.weight.shape) == (3, 256, 1, 1) and tuple(rpn.rpn_reg.weight.shape) == (12, 256, 1, 1)
    first = rpn.rpn_conv[0]
    assert type(first) is ConvModule and type(first.conv) is Conv3x3 and type(first.bn) is BatchNormAct2d and first.bn.act == "relu" and first.conv.bias is None
    assert 0.008 < float(rpn.rpn_reg.weight.detach().std()) < 0.012 and 0.009 < float(first.conv.weight.detach().std()) < 0.011       # Normal, std 0.01
    assert float(rpn.rpn_cls.bias.detach().abs().max()) == 0.0 and all(p.requires_grad for p in rpn.parameters())
    two = RPNHead(**dict(REFERENCE_RPN_HEAD, loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False)))
    assert two.rpn_cls.out_channels == 6
    frozen = RPNHead(**dict(REFERENCE_RPN_HEAD, norm_cfg=dict(type="SyncBN", requires_grad=False)))
    assert not frozen.rpn_conv[0].bn.weight.requires_grad and frozen.rpn_conv[0].conv.weight.requires_grad
    with pytest.raises(NotImplementedError, match="norm_cfg"):
        RPNHead(**dict(REFERENCE_RPN_HEAD, norm_cfg=dict(type="GN", num_groups=32)))

    mask = FCNMaskHead(**REFERENCE_MASK_HEAD)
    assert len(mask.convs) == 4 and type(mask.upsample) is Deconv2x2 and type(mask.conv_logits) is Conv1x1Thin
    assert tuple(mask.conv_logits.weight.shape) == (1, 256, 1, 1) and tuple(mask.upsample.weight.shape) == (256, 256, 2, 2)
    assert float(mask.upsample.bias.detach().abs().max()) == 0.0 and float(mask.conv_logits.bias.detach().abs().max()) == 0.0
    std = (2.0 / (256 * 4)) ** 0.5                                       # Kaiming normal, fan_out of a [Cin, Cout, 2, 2] weight = Cin * 4
    assert 0.9 * std < float(mask.upsample.weight.detach().std()) < 1.1 * std
    wide = FCNMaskHead(**dict(REFERENCE_MASK_HEAD, class_agnostic=False, num_classes=80))
    assert type(wide.conv_logits) is Conv1x1 and wide.conv_logits.out_channels == 80
    for option in (dict(type="bilinear", scale_factor=2), dict(type="nearest", scale_factor=2), dict(type="carafe", scale_factor=2),
                   dict(type="deconv", scale_factor=4)):
        with pytest.raises(NotImplementedError, match=option["type"]):
            FCNMaskHead(**dict(REFERENCE_MASK_HEAD, upsample_cfg=option))


def test_conv1x1thin_is_conv2d_by_parameters_and_state_dict(ops):
    torch.manual_seed(3)
    a = Conv1x1Thin(64, 12)
    torch.manual_seed(3)
    b = nn.Conv2d(64, 12, 1)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    x = torch.randn(2, 64, 3, 5)
    assert torch.equal(a(x), b(x))                                       # no backend: F.conv2d
    with pytest.raises(AssertionError, match="at most 16"):
        Conv1x1Thin(64, 17)
    assert conv_mod.FUSED_THIN_DEFAULT in (False, True) and conv_mod.THIN_MAX_N == 16


def test_packed_weights_are_cached_on_the_version_counters(ops):
    a, b = Conv1x1Thin(64, 3, ops=ops, fused=True), Conv1x1Thin(64, 12, ops=ops, fused=True, bias=False)
    Wp, bias = conv_mod._thin_packed((a, b))
    assert conv_mod._thin_packed((a, b))[0] is Wp and Wp.dtype == BF and tuple(Wp.shape) == (15, 64) and tuple(bias.shape) == (15,)
    assert torch.equal(Wp[:3], a.weight.detach().view(3, 64).to(BF)) and torch.equal(Wp[3:], b.weight.detach().view(12, 64).to(BF))
    assert float(bias[3:].abs().max()) == 0.0
    with torch.no_grad():
        b.weight.mul_(2)
    W2, _ = conv_mod._thin_packed((a, b))
    assert W2 is not Wp and torch.equal(W2[3:], b.weight.detach().view(12, 64).to(BF))
    assert tuple(a.gemm_weights()[0].shape) == (3, 64)


# ------------------------------------------------------------------------------------------------ exact operands through both modules
@pytest.mark.parametrize("kind", ["rpn2", "rpn1", "mask"])
def test_exact_operands_bit_for_bit(ops, kind):
    outs = check_exact(kind, ops)
    assert all(o.is_contiguous() for o in outs)


# ------------------------------------------------------------------------------------------------ the layers alone
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_conv1x1thin_against_float64_autograd(ops, shape, layout, dtype, kind):
    check_thin(ops, shape, layout, dtype, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape,widths", [((105, 64, 15), [3, 12]), ((32, 256, 16), [4, 12]), ((256, 320, 12), [11, 1])])
def test_thin_heads_pair_against_float64_autograd(ops, shape, widths, layout, dtype, kind):
    check_thin(ops, shape, layout, dtype, kind, widths=widths)


def test_thin_heads_is_one_forward_and_one_gradient_launch(ops):
    calls = []

    class Counting(RefOpsThin):
        def thin_fwd(self, *a, **k):
            calls.append("fwd")
            return super().thin_fwd(*a, **k)

        def thin_dgrad(self, *a, **k):
            calls.append("dgrad")
            return super().thin_dgrad(*a, **k)
    o = Counting()
    a, b = Conv1x1Thin(64, 3, ops=o, fused=True), Conv1x1Thin(64, 12, ops=o, fused=True)
    x = torch.randn(2, 64, 4, 4).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ya, yb = thin_heads(x, [a, b])
    assert ya.untyped_storage().data_ptr() == yb.untyped_storage().data_ptr()          # one allocation, two contiguous NCHW tensors
    ya.sum().backward()                                                  # yb's gradient is missing: zeros
    assert calls == ["fwd", "dgrad"]
    assert float(b.weight.grad.abs().max()) == 0.0 and float(a.weight.grad.abs().max()) > 0 and float(a.bias.grad[0]) == 32.0
    calls.clear()
    wide = [Conv1x1Thin(64, 8, ops=o, fused=True), Conv1x1Thin(64, 12, ops=o, fused=True)]
    ys = thin_heads(x.detach(), wide)                                    # widths past 16: module by module
    assert calls == ["fwd", "fwd"] and [tuple(y.shape) for y in ys] == [(2, 8, 4, 4), (2, 12, 4, 4)]


def test_the_input_gradient_rounds_dy_to_bf16(ops):
    check_dy_rounding(ops)


# ------------------------------------------------------------------------------------------------ the modules with norm
@pytest.mark.parametrize("kind", ["rpn2", "mask1"])
def test_random_operands_with_norm_within_the_threshold(ops, kind):
    """Measured on the CPU backend: profiles/thin_heads_parity.md."""
    worst = parity(kind, ops)
    assert max(worst) <= PARITY_REL_L2, (worst, PARITY_REL_L2)


# ------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("kind", ["rpn2", "mask1"])
def test_fused_false_is_the_torch_route_with_the_twins_bits(ops, kind):
    state, xs, gs, outs, dx, dp = random_case(kind)
    m = make_module(kind, ops, fused=False, norm_cfg=dict(type="BN")).train()
    m.load_state_dict(state, strict=True)
    got_outs, got_dx, got_dp = run_module(m, xs, gs)
    assert all(torch.equal(a, b) for a, b in zip(got_outs, outs)) and all(torch.equal(a, b) for a, b in zip(got_dx, dx))
    assert all(torch.equal(got_dp[k], dp[k]) for k in dp)


def test_fused_true_raises_outside_the_coverage(ops):
    with pytest.raises(NotImplementedError, match="Cin % 64"):
        Conv1x1Thin(32, 3, ops=ops, fused=True)(torch.randn(1, 32, 2, 2))
    with pytest.raises(NotImplementedError, match="Cin % 64"):
        thin_heads(torch.randn(1, 32, 2, 2), [Conv1x1Thin(32, 3, ops=ops, fused=True), Conv1x1Thin(32, 12, ops=ops, fused=True)])
    with pytest.raises(NotImplementedError, match="Cin % 64"):
        Conv1x1Thin(64, 3, ops=ops, fused=True)(torch.randn(1, 64, 2, 2, dtype=torch.float64))
    loose = Conv1x1Thin(32, 3, ops=ops, fused=None)
    x = torch.randn(1, 32, 2, 2)
    assert torch.equal(loose(x), F.conv2d(x, loose.weight, loose.bias))
    with pytest.raises(NotImplementedError, match="coverage"):
        FCNMaskHead(num_convs=0, in_channels=64, conv_out_channels=32, class_agnostic=True, ops=ops, fused=True)(torch.randn(1, 64, 2, 2))

    class NoThin:
        name = "nothin"

        def empty(self, shape, dtype):
            return torch.empty(shape, dtype=dtype)
    plain = Conv1x1Thin(64, 3, ops=NoThin(), fused=None)
    y = plain(torch.randn(1, 64, 2, 2))
    assert "Thin" not in type(y.grad_fn).__name__


def test_wrappers_pack_the_arguments_and_assert_the_layouts():
    from clipself_amd.hip import EPI_THIN_DGRAD, EPI_THIN_FWD, HipOps
    assert HipOps.THIN_HEADS is True and (EPI_THIN_FWD, EPI_THIN_DGRAD) == (10, 11)
    X, W = torch.zeros(70, 64 + 8, dtype=BF)[:, :64], torch.zeros(15, 64, dtype=BF)
    rows, planes = torch.zeros(70, 15), torch.zeros(70 * 15)
    assert HipOps._thin_form(X, W, rows, None, 0, None) == (70, 15, 64, 0, 15, 0)
    assert HipOps._thin_form(X.float(), W, rows[:, :15], None, 0, None) == (70, 15, 64, 0, 15, 1)
    assert HipOps._thin_form(X, W, planes[:70 * 3], planes[70 * 3:], 35, 3) == (70, 15, 64, 35, 3, 0)
    assert HipOps._thin_form(X, W, planes, None, 35, None) == (70, 15, 64, 35, 15, 0)
    for bad in (lambda: HipOps._thin_form(X, W, rows, None, 0, 3),                               # rows form has no split
                lambda: HipOps._thin_form(X, W, planes[:70 * 3], None, 35, 3),                   # a split below N needs the second block
                lambda: HipOps._thin_form(X, W, planes[:70 * 3], planes[70 * 3:], 36, 3),        # M % R
                lambda: HipOps._thin_form(X, W, planes[:70 * 3], planes[70 * 4:], 35, 3),        # the second block holds M * (N - s)
                lambda: HipOps._thin_form(X, torch.zeros(17, 64, dtype=BF), torch.zeros(70, 17), None, 0, None),      # N <= 16
                lambda: HipOps._thin_form(X[:, :32], W[:, :32], rows, None, 0, None),            # K % 64
                lambda: HipOps._thin_form(X.t(), W, rows, None, 0, None),                        # rows: last stride 1
                lambda: HipOps._thin_form(X, W.float(), rows, None, 0, None)):                   # W is bf16
        with pytest.raises(AssertionError):
            bad()


# ------------------------------------------------------------------------------------------------ planted errors
# which exact check shows which flaw: the RPN pair (split 3 of 15, bias, two blocks), the mask head (rows form with the ReLU gate), the
# dY rounding check
REJECTED_BY = {"split_off_by_one": "rpn2", "plane_index_swapped": "rpn2", "bias_second_block_only": "pair", "second_block_ignored": "rpn2",
               "gate_lt": "mask", "dy_not_rounded": None}


@pytest.mark.parametrize("flaw", FLAWS)
def test_the_exact_checks_reject_a_defective_restatement(flaw):
    bad = RefOpsThin(flaws=(flaw,))
    with pytest.raises(AssertionError, match="differ"):
        if REJECTED_BY[flaw] is None:
            check_dy_rounding(bad)
        elif REJECTED_BY[flaw] == "pair":                               # integer biases in [-8, 8] on both modules
            check_thin(bad, (105, 64, 15), "channel_last", F32, "exact", widths=[3, 12])
        else:
            check_exact(REJECTED_BY[flaw], bad)
    if flaw in ("split_off_by_one", "plane_index_swapped", "second_block_ignored"):
        with pytest.raises(AssertionError, match="differ"):
            check_thin(bad, (105, 64, 15), "channel_last", F32, "exact", widths=[3, 12])
