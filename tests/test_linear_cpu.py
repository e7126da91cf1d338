"""CPU: linear.LinearAct and bbox_head.ConvFCBBoxHead -- the box head's FCs -- on the reference backend (tests/_fc_ref.RefOpsFC): the
packing of the weights, the state dict, the layer's kernel route and autograd function with and without `spatial` (exact operands bit
for bit against float64 autograd, random operands inside the derived bounds), split-K as the header states it, the fallbacks, the head's
key names and outputs, and that the checks reject planted errors."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _fc_ref import (BF, F32, RefOpsFC, auto_splits, bounds, case, check_bound, layer, reference, rne_bf16, run_layer, same_bits)
from clipself_amd import linear as L
from clipself_amd.bbox_head import ConvFCBBoxHead
from clipself_amd.linear import LinearAct, pack_weights

# (rows, in, out, geom): one K tile, out % 64 != 0 (padded dgrad) | the flatten form on a 2 x 2 map, out % 64 != 0 |
# the flatten form with C = 64, P = 49: 49 K tiles, which the automatic rule cuts in two
CASES = [((5, 128, 16), None), ((3, 256, 24), (64, 2, 2)), ((6, 3136, 64), (64, 7, 7))]
IDS = ["5x128x16", "3x(64x2x2)x24", "6x(64x7x7)x64"]


@pytest.fixture(scope="module")
def ops():
    return RefOpsFC()


def _spatial(geom):
    return None if geom is None else (geom[0], geom[1] * geom[2])


# ------------------------------------------------------------------------------------------------ operands and state
def test_packing_follows_the_channel_last_rows():
    C, P, out = 64, 4, 8
    w = torch.randn(out, C * P, generator=torch.Generator().manual_seed(1)).to(BF).to(F32)
    Wp, WpT = pack_weights(w, (C, P))
    assert Wp.dtype == BF and tuple(Wp.shape) == (out, C * P) and tuple(WpT.shape) == (C * P, 64)
    for o, c, p in [(0, 0, 0), (3, 7, 1), (7, 63, 3), (5, 31, 2)]:
        assert float(Wp[o, p * C + c]) == float(w[o, c * P + p])
        assert float(WpT[p * C + c, o]) == float(w[o, c * P + p])
    assert bool((WpT[:, out:] == 0).all())                               # the dgrad's K padding
    x = torch.randn(3, C, 2, 2, generator=torch.Generator().manual_seed(2)).to(BF).to(F32)
    rows = x.permute(0, 2, 3, 1).reshape(3, P * C)                       # the channel-last map's memory, seen as [K, P*C]
    assert torch.equal(rows.double() @ Wp.double().T, x.flatten(1).double() @ w.double().T)
    plain, plainT = pack_weights(w)
    assert torch.equal(plain.float(), w) and torch.equal(plainT[:, :out].float(), w.T)


def test_state_dict_loads_strictly_both_ways_and_parameters_match_linear():
    torch.manual_seed(3)
    ref = nn.Linear(128, 16)
    torch.manual_seed(3)
    m = LinearAct(128, 16, act="relu")
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), ref.parameters()))                  # the same initialisation
    ref2 = nn.Linear(128, 16)
    m.load_state_dict(ref2.state_dict(), strict=True)
    assert torch.equal(m.weight, ref2.weight) and torch.equal(m.bias, ref2.bias)
    back = nn.Linear(128, 16)
    back.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(back.weight, ref2.weight)
    LinearAct(256, 8, bias=False, spatial=(64, 4)).load_state_dict(nn.Linear(256, 8, bias=False).state_dict(), strict=True)
    for bad in (dict(act="gelu"), dict(spatial=(64, 3)), dict(splits=0)):
        with pytest.raises(AssertionError):
            LinearAct(256, 8, **bad)


def test_packed_weights_follow_the_version_counters(ops):
    x, w, b, dy, _ = case(CASES[0][0], "exact")
    m = layer(ops, w, b, fused=True, act="relu")
    a = m.gemm_weights()
    assert m.gemm_weights()[0] is a[0]
    with torch.no_grad():
        m.weight.mul_(2)
    assert torch.equal(m.gemm_weights()[0].float(), a[0].float() * 2)
    with torch.no_grad():
        m.bias.add_(1)
    assert torch.equal(m.gemm_weights()[2], b + 1)


# ------------------------------------------------------------------------------------------------ the op as the header states it
def test_reference_gemm_splits_and_rejections(ops):
    assert auto_splits(4096, 512, 12544) == 8 and auto_splits(8000, 512, 12544) == 4 and auto_splits(4096, 512, 512) == 1
    assert auto_splits(6, 64, 3136) == 2
    x, w, b, dy, ref = case((6, 3136, 64), "exact")
    X, W = x.to(BF), w.to(BF)
    for epi, want in ((0, F.linear(x.double(), w.double(), b.double())), (9, ref["y"])):
        for s in (1, 2, 3, 5, 0):
            n = s if s > 0 else auto_splits(6, 64, 3136)
            C = torch.full((6, 64), float("nan"), dtype=BF)
            ops.gemm_nt(X, W, C, b, extra=torch.full((n * 6 * 64,), float("nan")) if n > 1 else None, epi=epi, splits=s)
            same_bits(C, rne_bf16(want), f"epi {epi} splits {s}")
    C = torch.empty(6, 64, dtype=BF)
    with pytest.raises(RuntimeError):
        ops.gemm_nt(X, W, C, b, extra=torch.empty(50 * 6 * 64), epi=9, splits=50)                    # 49 K tiles
    with pytest.raises(RuntimeError):
        ops.gemm_nt(X, W, C, b, extra=None, epi=9, splits=2)
    with pytest.raises(RuntimeError):
        ops.gemm_nt(X, W, C, b, extra=torch.empty(2 * 6 * 64 - 1), epi=0, splits=2)
    with pytest.raises(RuntimeError):
        ops.gemm_nt(X, W, torch.empty(6, 64), b, extra=torch.empty(2 * 6 * 64), epi=1, splits=2)


def test_relu_edge_values(ops):
    """Pre-activations of exactly +0, -0 (unreachable: an fp32 sum that starts at +0 ends at +0), a negative integer and NaN."""
    A = torch.zeros(4, 64, dtype=BF)
    A[:, 0] = torch.tensor([1.0, 1.0, 1.0, 1.0])
    W = torch.zeros(8, 64, dtype=BF)
    W[:, 0] = 3.0
    bias = torch.tensor([-3.0, -0.0, -5.0, float("nan"), 2.0, -3.0, -4.0, 0.0])
    C = torch.full((4, 8), float("nan"), dtype=BF)
    ops.gemm_nt(A, W, C, bias, epi=9)
    want = F.relu(3.0 + bias.double()).to(BF).expand(4, 8)
    assert torch.equal(C[:, [0, 1, 2, 4, 5, 6, 7]].view(torch.int16), want[:, [0, 1, 2, 4, 5, 6, 7]].contiguous().view(torch.int16))
    assert bool(C[:, 3].isnan().all())


# ------------------------------------------------------------------------------------------------ the layer on the reference backend
@pytest.mark.parametrize("act", ["relu", None])
@pytest.mark.parametrize("shape,geom", CASES, ids=IDS)
def test_layer_exact_operands_bit_for_bit(ops, shape, geom, act):
    x, w, b, dy, ref = case(shape, "exact", act)
    for splits in (None, 1, 2):
        if splits == 2 and shape[1] < 128:
            continue
        m = layer(ops, w, b, fused=True, act=act, spatial=_spatial(geom), splits=splits)
        for dtype in (F32, BF):
            y, dx, dw, db = run_layer(m, x, dy, dtype, geom)
            assert type(m(x.view(-1, *geom) if geom else x).grad_fn).__name__ == "_LinearActFnBackward"
            same_bits(y, rne_bf16(ref["y"]).to(dtype), f"y {dtype} splits={splits}")
            same_bits(dx, ref["dx"].to(dtype) if dtype == F32 else rne_bf16(ref["dx"]), f"dx {dtype}")
            same_bits(dw, ref["dw"].to(F32), "dw in nn.Linear's layout")
            same_bits(db, ref["db"].to(F32), "db")
            if geom is not None:
                assert dx.shape == x.shape


@pytest.mark.parametrize("shape,geom", CASES, ids=IDS)
def test_layer_random_operands_within_the_derived_bounds(ops, shape, geom):
    x, w, b, dy, _ = case(shape, "random")
    m = layer(ops, w, b, fused=True, act="relu", spatial=_spatial(geom))
    for dtype in (F32, BF):
        y, dx, dw, db = run_layer(m, x, dy, dtype, geom)
        ref = reference(x, w, b, dy, mask=y > 0)                          # the gate of the layer's own saved output
        tol = bounds(ref, shape, splits=8, bf16_dx=dtype == BF)
        for k, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
            check_bound(f"{IDS[CASES.index((shape, geom))]} {dtype} {k}", got, ref[k], tol[k])


def test_spatial_layer_equals_linear_on_the_flattened_map(ops):
    """Channel-last and NCHW-contiguous maps, fp32 and bf16, give nn.Linear(x.flatten(1)) bit for bit; the returned gradient is a
    channel-last map."""
    shape, geom = CASES[2]
    x, w, b, dy, ref = case(shape, "exact")
    m = layer(ops, w, b, fused=True, act="relu", spatial=_spatial(geom))
    lin = nn.Linear(shape[1], shape[2])
    lin.load_state_dict(m.state_dict(), strict=True)
    want = F.relu(lin(x.view(-1, *geom).flatten(1))).detach()
    for cl in (True, False):
        for dtype in (F32, BF):
            y, dx, dw, db = run_layer(m, x, dy, dtype, geom, channel_last=cl)
            same_bits(y.float(), want.to(BF).float(), f"channel_last={cl} {dtype}")
            same_bits(dw, ref["dw"].to(F32), "dw")
    inp = x.view(-1, *geom).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    m(inp).sum().backward()
    assert inp.grad.permute(0, 2, 3, 1).is_contiguous()


def test_fallbacks_and_fused_true_outside_the_coverage(ops, monkeypatch):
    x, w, b, dy, ref = case(CASES[0][0], "exact")
    called = []
    spy = RefOpsFC()
    spy.gemm_nt = lambda *a, **k: called.append("gemm_nt") or RefOpsFC.gemm_nt(spy, *a, **k)
    y = layer(spy, w, b, fused=False, act="relu")(x)
    assert not called and type(y.grad_fn).__name__ != "_LinearActFnBackward"
    same_bits(y.detach(), ref["y"].to(F32), "fused=False")
    same_bits(layer(None, w, b, act="relu")(x).detach(), ref["y"].to(F32), "CPU tensor")
    with pytest.raises(NotImplementedError):
        layer(None, w, b, fused=True, act="relu")(x)
    for default in (True, False):
        monkeypatch.setattr(L, "FUSED_FC_DEFAULT", default)
        called.clear()
        layer(spy, w, b, act="relu")(x)
        assert bool(called) == default

    class NoFC(RefOpsFC):
        LINEAR_ACT = False
    same_bits(layer(NoFC(), w, b, act="relu")(x).detach(), ref["y"].to(F32), "backend without LINEAR_ACT")
    # fc_reg's shape (512 -> 4) and in % 64 != 0 are outside the coverage -> torch; fused=True raises
    g = torch.Generator().manual_seed(2)
    for inf, out in ((512, 4), (96, 8)):
        xs, ws, bs = (torch.randint(-8, 9, s, generator=g).float() for s in ((3, inf), (out, inf), (out,)))
        called.clear()
        ys = layer(spy, ws, bs)(xs)
        assert not called
        same_bits(ys.detach(), F.linear(xs, ws, bs), f"{inf} -> {out}")
        with pytest.raises(NotImplementedError):
            layer(spy, ws, bs, fused=True)(xs)
    with pytest.raises(NotImplementedError):
        layer(spy, w, b, fused=True)(x.to(torch.float16))


# ------------------------------------------------------------------------------------------------ the head
HEAD_KEYS = [
    "shared_convs.0.conv.weight", "shared_convs.0.bn.weight", "shared_convs.0.bn.bias", "shared_convs.0.bn.running_mean",
    "shared_convs.0.bn.running_var", "shared_convs.0.bn.num_batches_tracked",
    "shared_convs.1.conv.weight", "shared_convs.1.bn.weight", "shared_convs.1.bn.bias", "shared_convs.1.bn.running_mean",
    "shared_convs.1.bn.running_var", "shared_convs.1.bn.num_batches_tracked",
    "shared_fcs.0.weight", "shared_fcs.0.bias", "shared_fcs.1.weight", "shared_fcs.1.bias",
    "cls_fcs.0.weight", "cls_fcs.0.bias", "reg_fcs.0.weight", "reg_fcs.0.bias",
    "fc_cls.weight", "fc_cls.bias", "fc_reg.weight", "fc_reg.bias",
]


def _head(ops, fused, **kw):
    cfg = dict(type="FViTBBoxHead", in_channels=64, conv_out_channels=64, fc_out_channels=64, roi_feat_size=7, num_classes=5, reg_class_agnostic=True,
               norm_cfg=dict(type="SyncBN", requires_grad=True), num_shared_convs=2, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1,
               bbox_coder=dict(type="DeltaXYWHBBoxCoder"), loss_cls=dict(type="CustomCrossEntropyLoss"), loss_bbox=dict(type="L1Loss"),
               learned_temperature=50.0, vlm_temperature=50.0, alpha=0.1, beta=0.6, class_embed="x.pt", seen_classes="s.json",
               all_classes="a.json")
    cfg.update(kw)
    torch.manual_seed(11)
    return ConvFCBBoxHead(ops=ops, fused=fused, **cfg)


def test_head_key_names_and_shapes(ops):
    h = _head(ops, True)
    assert list(h.state_dict().keys()) == HEAD_KEYS
    sd = h.state_dict()
    assert tuple(sd["shared_fcs.0.weight"].shape) == (64, 64 * 49) and tuple(sd["fc_cls.weight"].shape) == (6, 64)
    assert tuple(sd["fc_reg.weight"].shape) == (4, 64) and tuple(sd["cls_fcs.0.weight"].shape) == (64, 64)
    assert h.shared_fcs[0].spatial == (64, 49) and h.shared_fcs[1].spatial is None and all(m.act == "relu" for m in h.shared_fcs)
    assert tuple(_head(ops, True, reg_class_agnostic=False).fc_reg.weight.shape) == (20, 64)
    other = _head(None, False)
    other.load_state_dict(sd, strict=True)
    assert float(sd["fc_reg.weight"].std()) < 0.002 and float(sd["fc_cls.weight"].std()) < 0.02 and float(sd["shared_fcs.1.bias"].abs().max()) == 0


def test_head_equals_the_same_stack_in_plain_torch(ops):
    """fvit_head.py:72-107 written with torch's modules on the same state, in float64, against the head on the reference backend: the
    convolution + batch norm trunk to its own tests' tolerance of a bf16 pipeline, and the torch route (fused=False) to fp32 rounding."""
    h = _head(ops, True)
    x = torch.randn(6, 64, 7, 7, generator=torch.Generator().manual_seed(5)).to(BF).to(F32)
    sd = {k: v.double() if v.is_floating_point() else v for k, v in h.state_dict().items()}

    def plain(x):
        x = x.double()
        for i in range(2):
            x = F.conv2d(x, sd[f"shared_convs.{i}.conv.weight"], None, padding=1)
            x = F.relu(F.batch_norm(x, None, None, sd[f"shared_convs.{i}.bn.weight"], sd[f"shared_convs.{i}.bn.bias"], True, 0.1, 1e-5))
        x = x.flatten(1)
        for i in range(2):
            x = F.relu(F.linear(x, sd[f"shared_fcs.{i}.weight"], sd[f"shared_fcs.{i}.bias"]))
        x_cls = F.relu(F.linear(x, sd["cls_fcs.0.weight"], sd["cls_fcs.0.bias"]))
        x_reg = F.relu(F.linear(x, sd["reg_fcs.0.weight"], sd["reg_fcs.0.bias"]))
        return x_cls, F.linear(x_reg, sd["fc_reg.weight"], sd["fc_reg.bias"])

    want_cls, want_reg = plain(x)
    torch_head = _head(None, False)
    torch_head.load_state_dict(h.state_dict(), strict=True)
    got_cls, got_reg = torch_head(x)
    assert got_cls.shape == (6, 64) and got_reg.shape == (6, 4)
    assert float((got_cls.double() - want_cls).abs().max()) <= 1e-4 * float(want_cls.abs().max())
    assert float((got_reg.double() - want_reg).abs().max()) <= 1e-4 * float(want_reg.abs().max())
    k_cls, k_reg = h(x)
    assert type(k_cls.grad_fn).__name__ == "_LinearActFnBackward"
    # five bf16 roundings of activations and four of weights in a row: 2^-8 each, relative to the largest value
    assert float((k_cls.double() - want_cls).abs().max()) <= 9 * 2.0 ** -8 * float(want_cls.abs().max())
    assert float((k_reg.double() - want_reg).abs().max()) <= 9 * 2.0 ** -8 * float(want_reg.abs().max())
    (k_cls.sum() + k_reg.sum()).backward()
    assert all(p.grad is not None for n, p in h.named_parameters() if not n.startswith("fc_cls"))
    assert h.fc_cls.weight.grad is None                                   # unused, as in FViTBBoxHead.forward


# ------------------------------------------------------------------------------------------------ the checks reject planted errors
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _rejected(m, shape, geom, keys, kinds=("exact", "random")):
    """Runs the flawed layer m on both kinds of operands; every named result must fail its exact check and its bound check."""
    for kind in kinds:
        x, w, b, dy, ref = case(shape, kind)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        y, dx, dw, db = run_layer(m, x, dy, F32, geom)
        got = dict(y=y, dx=dx, dw=dw, db=db)
        if kind == "random":
            ref = reference(x, w, b, dy, mask=y > 0)
        tol = bounds(ref, shape, splits=8)
        for k in keys:
            if kind == "exact":
                want = rne_bf16(ref["y"]).to(F32) if k == "y" else ref[k].to(F32)
                assert _fails(lambda: same_bits(got[k], want, k)), (kind, k)
            else:
                assert _fails(lambda: check_bound(k, got[k], ref[k], tol[k])), (kind, k)


def test_checks_reject_cp_and_pc_confused_in_the_packed_weights(ops, monkeypatch):
    shape, geom = CASES[1]
    monkeypatch.setattr(L, "pack_weights", lambda weight, spatial=None: pack_weights(weight, None))
    _rejected(LinearAct(shape[1], shape[2], act="relu", spatial=_spatial(geom), ops=ops, fused=True), shape, geom, ("y", "dx"))


def test_checks_reject_a_gate_taken_from_dy(ops, monkeypatch):
    shape, geom = CASES[0]
    monkeypatch.setattr(L, "relu_gate", lambda Y, dY: torch.where(dY > 0, dY, torch.zeros(())).to(BF))
    _rejected(LinearAct(shape[1], shape[2], act="relu", ops=ops, fused=True), shape, geom, ("dx", "dw", "db"))


def test_checks_reject_a_bias_added_once_per_slice():
    shape, geom = CASES[2]
    bad = RefOpsFC()
    bad.flaws = ("bias_per_slice",)
    _rejected(LinearAct(shape[1], shape[2], act="relu", spatial=_spatial(geom), ops=bad, fused=True, splits=2), shape, geom, ("y",))


def test_checks_reject_a_weight_gradient_left_in_pc_order(ops, monkeypatch):
    shape, geom = CASES[1]
    monkeypatch.setattr(L, "unpack_wgrad", lambda dWp, spatial=None: dWp)
    _rejected(LinearAct(shape[1], shape[2], act="relu", spatial=_spatial(geom), ops=ops, fused=True), shape, geom, ("dw",))


def test_checks_reject_untransposed_dgrad_weights(ops, monkeypatch):
    shape = (5, 64, 64)                                                  # square: the untransposed matrix fits the call

    def untransposed(weight, spatial=None):
        Wp, _ = pack_weights(weight, spatial)
        return Wp, Wp.clone()
    monkeypatch.setattr(L, "pack_weights", untransposed)
    _rejected(LinearAct(64, 64, act="relu", ops=ops, fused=True), shape, None, ("dx",))
