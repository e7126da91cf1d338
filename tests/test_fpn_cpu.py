"""CPU: the detector's feature pyramid (clipself_amd/fpn.py, conv.Conv1x1, norm_act.ConvModule(kernel_size=)) on the reference backend of
tests/_fpn_ref.py -- state dicts against the torch twin, exact operands bit for bit against float64 autograd, random operands inside the
derived bounds (Conv1x1) and the recorded rel-L2 thresholds (the module with norm), dispatch, and the six planted errors the checks reject."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _fpn_ref import (BF, CONV1X1_SHAPES, EXACT_GEOMS, LAYOUTS, PARITY_GRAD_REL_L2, PARITY_OUT_REL_L2, REFERENCE_NECK, RefOpsFPN, TwinFPN,
                      check_conv1x1, check_exact, flawed_fpn, parity, random_case, run_module)
from clipself_amd.conv import Conv1x1, Conv3x3
from clipself_amd.fpn import FPN
from clipself_amd.norm_act import BatchNormAct2d, ConvModule


@pytest.fixture(scope="module")
def ops():
    return RefOpsFPN()


def kernel_fpn(ops, **extra):
    return lambda *a, **k: FPN(*a, ops=ops, fused=True, **k, **extra)


# ------------------------------------------------------------------------------------------------ state dict
@pytest.mark.parametrize("norm_cfg", [None, dict(type="SyncBN", requires_grad=True)], ids=["nonorm", "SyncBN"])
def test_state_dict_is_the_twins_strict_both_ways(norm_cfg):
    m, twin = FPN([64, 128, 64], 32, 5, norm_cfg=norm_cfg), TwinFPN([64, 128, 64], 32, 5, norm_cfg=norm_cfg)
    assert list(m.state_dict()) == list(twin.state_dict())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in twin.state_dict().items()}
    twin.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(twin.state_dict(), strict=True)
    keys = set(m.state_dict())
    if norm_cfg is None:
        assert {"lateral_convs.0.conv.weight", "lateral_convs.0.conv.bias", "fpn_convs.2.conv.bias"} <= keys and not any(".bn." in k for k in keys)
    else:
        want = {f"lateral_convs.0.bn.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
        assert want | {"lateral_convs.0.conv.weight", "fpn_convs.0.conv.weight"} <= keys and not any(k.endswith("conv.bias") for k in keys)


def test_the_references_config_dict_constructs_the_module():
    m = FPN(**REFERENCE_NECK)
    assert len(m.lateral_convs) == len(m.fpn_convs) == 4 and m.num_outs == 5
    lat, out = m.lateral_convs[0], m.fpn_convs[3]
    assert type(lat.conv) is Conv1x1 and type(out.conv) is Conv3x3 and type(lat.bn) is BatchNormAct2d
    assert lat.act is None and lat.bn.act is None and out.bn.act is None and lat.conv.bias is None
    assert tuple(lat.conv.weight.shape) == (256, 768, 1, 1) and tuple(out.conv.weight.shape) == (256, 256, 3, 3)
    assert all(p.requires_grad for p in m.parameters())
    bound = (6.0 / (768 + 256)) ** 0.5                                  # Xavier-uniform, gain 1
    top = float(lat.conv.weight.detach().abs().max())
    assert 0.9 * bound < top <= bound
    frozen = FPN(**dict(REFERENCE_NECK, norm_cfg=dict(type="SyncBN", requires_grad=False)))
    assert not frozen.lateral_convs[0].bn.weight.requires_grad and frozen.lateral_convs[0].conv.weight.requires_grad
    plain = FPN([64] * 2, 64, 2)
    assert float(plain.lateral_convs[0].conv.bias.detach().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ exact operands
@pytest.mark.parametrize("name", list(EXACT_GEOMS))
def test_exact_operands_bit_for_bit(ops, name):
    check_exact(kernel_fpn(ops), name)


# ------------------------------------------------------------------------------------------------ Conv1x1 alone
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(CONV1X1_SHAPES))
def test_conv1x1_against_float64_autograd(ops, shape, layout, dtype, kind):
    check_conv1x1(ops, shape, layout, dtype, kind)


def test_conv1x1_is_conv2d_by_parameters_and_state_dict():
    torch.manual_seed(3)
    a = Conv1x1(64, 24)
    torch.manual_seed(3)
    b = nn.Conv2d(64, 24, 1)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    x = torch.randn(2, 64, 3, 5)
    assert torch.equal(a(x), b(x))                                       # no backend: F.conv2d


def test_conv1x1_packs_its_weights_once_per_version(ops):
    m = Conv1x1(64, 8, ops=ops, fused=True)
    first = m.gemm_weights()
    assert m.gemm_weights()[0] is first[0] and tuple(first[1].shape) == (64, 64) and float(first[1][:, 8:].abs().max()) == 0.0
    with torch.no_grad():
        m.weight.mul_(2)
    assert m.gemm_weights()[0] is not first[0] and torch.equal(m.gemm_weights()[0], (m.weight.detach().view(8, 64)).to(BF))


# ------------------------------------------------------------------------------------------------ random operands, with norm
def test_random_operands_with_norm_within_the_recorded_thresholds(ops):
    """Measured on the CPU backend: outputs and input gradients 2.6371e-3, parameter gradients 2.8333e-3 (profiles/fpn_parity.md)."""
    worst_out, worst_grad = parity(kernel_fpn(ops))
    assert worst_out <= PARITY_OUT_REL_L2, (worst_out, PARITY_OUT_REL_L2)
    assert worst_grad <= PARITY_GRAD_REL_L2, (worst_grad, PARITY_GRAD_REL_L2)


# ------------------------------------------------------------------------------------------------ the extra level
@pytest.mark.parametrize("fused", [False, True])
def test_extra_level_is_the_subsample_of_the_last_output(ops, fused):
    sizes = [24, 12, 6, 3] if not fused else [16, 8, 4, 2]              # an odd-sized outs[3] on the torch route
    torch.manual_seed(5)
    m = FPN([64] * 4, 64, 6, ops=ops, fused=fused)
    outs = m(tuple(torch.randn(2, 64, s, s) for s in sizes))
    assert len(outs) == 6 and tuple(outs[4].shape) == (2, 64, (sizes[3] + 1) // 2, (sizes[3] + 1) // 2)
    assert torch.equal(outs[4], outs[3][..., ::2, ::2]) and torch.equal(outs[5], outs[4][..., ::2, ::2])


# ------------------------------------------------------------------------------------------------ dispatch
def test_fused_false_is_the_torch_route_with_the_twins_bits(ops):
    state, xs, gs, outs, dx, dp, _ = random_case()
    m = FPN([64] * 4, 64, 5, norm_cfg=dict(type="BN"), ops=ops, fused=False).train()
    m.load_state_dict(state, strict=True)
    got_outs, got_dx, got_dp = run_module(m, xs, gs)
    assert all(torch.equal(a, b) for a, b in zip(got_outs, outs)) and all(torch.equal(a, b) for a, b in zip(got_dx, dx))
    assert all(torch.equal(got_dp[k], dp[k]) for k in dp)
    assert FPN([64] * 2, 64, 2)(tuple(torch.randn(1, 64, s, s) for s in (4, 2)))[0].grad_fn is not None      # no backend at all: torch


def test_fused_true_raises_outside_the_coverage(ops):
    maps = lambda C, sizes: tuple(torch.randn(1, C, s, s) for s in sizes)
    with pytest.raises(NotImplementedError, match="twice"):
        FPN([64] * 3, 64, 3, ops=ops, fused=True)(maps(64, (8, 4, 3)))                     # a level that is not twice the next one
    loose = FPN([64] * 3, 64, 3, ops=ops, fused=None)
    assert [tuple(o.shape[2:]) for o in loose(maps(64, (8, 4, 3)))] == [(8, 8), (4, 4), (3, 3)]       # mmdet's size=prev_shape
    with pytest.raises(NotImplementedError, match="Cin % 64"):
        FPN([32] * 2, 64, 2, ops=ops, fused=True)(maps(32, (4, 2)))
    for option in (dict(add_extra_convs="on_input"), dict(start_level=1), dict(end_level=2), dict(no_norm_on_lateral=True),
                   dict(act_cfg=dict(type="ReLU")), dict(upsample_cfg=dict(mode="bilinear")), dict(upsample_cfg=dict(scale_factor=2, mode="nearest"))):
        with pytest.raises(NotImplementedError, match=next(iter(option))):
            FPN([64] * 4, 64, 5, **option)
    with pytest.raises(NotImplementedError, match="norm_cfg"):
        FPN([64] * 4, 64, 5, norm_cfg=dict(type="GN", num_groups=32))


def test_conv_module_keeps_its_positional_forms():
    a, b = ConvModule(64, 64), ConvModule(64, 64, True, "relu")
    for m in (a, b):
        assert type(m.conv) is Conv3x3 and m.conv.bias is None and m.bn.act == "relu" and m.conv.padding == (1, 1)
    c = ConvModule(64, 32, False, None, kernel_size=1)
    assert type(c.conv) is Conv1x1 and c.bn is None and c.conv.bias is not None and c.conv.padding == (0, 0)
    x = torch.randn(1, 64, 3, 3)
    assert torch.equal(c(x), F.conv2d(x, c.conv.weight, c.conv.bias))
    with pytest.raises(AssertionError):
        ConvModule(64, 64, kernel_size=5)


def test_wrappers_pack_the_form_and_assert_the_layouts():
    from clipself_amd.hip import HipOps
    assert HipOps.FPN_TOPDOWN is True
    coarse, fine = torch.zeros(2 * 3 * 5, 24 + 8, dtype=BF)[:, :24], torch.zeros(2 * 6 * 10, 24)
    assert HipOps._topdown_form(7, coarse, fine, 2, 3, 5, 24, True) == 7 | 1 << 8 | 1 << 9 | 1 << 10 | 0 << 11 | 5 << 12
    assert HipOps._topdown_form(8, fine[:30], torch.zeros(120, 24, dtype=BF), 2, 3, 5, 24, False) == 8 | 1 << 8 | 0 << 10 | 1 << 11 | 5 << 12
    for bad in (lambda: HipOps._topdown_form(7, coarse, fine[:-1], 2, 3, 5, 24, True),             # the fine map has 4 * B * h * w rows
                lambda: HipOps._topdown_form(7, coarse.t(), fine, 2, 3, 5, 24, True),               # rows: last stride 1
                lambda: HipOps._topdown_form(7, coarse, fine, 2, 3, 5, 16, True),                   # C is the maps' width
                lambda: HipOps._topdown_form(7, coarse, fine, 2, 3, 1 << 20, 24, True)):            # w has 20 bits
        with pytest.raises(AssertionError):
            bad()


# ------------------------------------------------------------------------------------------------ planted errors
@pytest.mark.parametrize("flaw", ["fine_width_w", "pool_drops_tap", "ignores_accumulate"])
def test_the_exact_check_rejects_defective_ops(flaw):
    bad = RefOpsFPN(flaws=(flaw,))
    with pytest.raises(AssertionError, match="differ"):
        check_exact(kernel_fpn(bad), "wide3")                            # h != w: an upsample that indexes fine rows with w shows here
    if flaw != "fine_width_w":
        with pytest.raises(AssertionError, match="differ"):
            check_exact(kernel_fpn(bad), "square4")


@pytest.mark.parametrize("flaw", ["up_lateral", "extra_from_merged"])
def test_the_exact_check_rejects_defective_modules(ops, flaw):
    for name in EXACT_GEOMS:
        with pytest.raises(AssertionError, match="differ"):
            check_exact(lambda *a, **k: flawed_fpn(flaw, *a, ops=ops, fused=True, **k), name)


def test_the_parity_check_rejects_a_relu_on_the_laterals(ops):
    worst_out, worst_grad = parity(lambda *a, **k: flawed_fpn("lateral_relu", *a, ops=ops, fused=True, **k))
    assert worst_out > 10 * PARITY_OUT_REL_L2 and worst_grad > 10 * PARITY_GRAD_REL_L2
    with pytest.raises(AssertionError, match="differ"):
        check_exact(lambda *a, **k: flawed_fpn("lateral_relu", *a, ops=ops, fused=True, **k), "square4")
