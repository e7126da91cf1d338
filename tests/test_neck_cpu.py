"""CPU: neck.Deconv2x2 -- ConvTranspose2d(k=2, s=2) as GEMMs on token rows -- and its wiring into the detector backbone, on the per-kernel
references (tests/_neck_ref.RefOpsNeck: fp32 accumulation of bf16 operands, as the kernels).  The comparisons with float64
F.conv_transpose2d use the derived per-element bounds of tests/_neck_ref.py; on exact operands they are bit for bit."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _backbone_ref import FIXTURES, OUT_INDICES, RefOpsBackbone, backbone_cfg, build_tower, load_fixture, rel_l2
from _neck_ref import (BF, F32, EXACT_CASES, KERNEL_SHAPES, ExactnessError, RefOpsNeck, bound, check_bound, exact_operands, exact_reference,
                       index_nchw_to_rows, index_rows_to_nchw, random_operands, reference, rne_bf16, to_rows)
from clipself_amd.neck import Deconv2x2, TokenRows


@pytest.fixture(scope="module")
def ops():
    return RefOpsNeck()


def _layer(ops, weight, bias):
    m = Deconv2x2(weight.shape[0], weight.shape[1], ops=ops)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    return m


def _run(m, x, dy, kind, off=1, out_dtype=F32):
    """forward + backward of the layer on an NCHW tensor (requires grad) or a TokenRows -> (y, dw, db, dx | None)."""
    m.zero_grad()
    if kind == "nchw":
        inp = x.clone().to(out_dtype).requires_grad_(True)
        y = m(inp)
    else:
        B, C, h, w = x.shape
        m.out_dtype = out_dtype
        inp = None
        y = m(TokenRows(to_rows(x, off), B, h, w, off))
    y.backward(dy.to(y.dtype))
    return y.detach(), m.weight.grad, m.bias.grad, None if inp is None else inp.grad


# ------------------------------------------------------------------------------------------------ the two maps
@pytest.mark.parametrize("B,h,w,C", KERNEL_SHAPES)
@pytest.mark.parametrize("s,off", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_the_two_maps_are_inverse_and_follow_the_definition(B, h, w, C, s, off):
    P, ld = h * w, s * s * C + 3
    rows = torch.randn(B * (P + off), ld, generator=torch.Generator().manual_seed(P + C)).to(BF)
    out = index_rows_to_nchw(rows, B, h, w, C, s, off, F32)
    b, c, i, j, di, dj = B - 1, C - 1, h - 1, w // 2, s - 1, 0
    assert out[b, c, s * i + di, s * j + dj] == rows[b * (P + off) + off + i * w + j, (di * s + dj) * C + c].float()
    back = torch.full_like(rows, 7.0)
    index_nchw_to_rows(out, B, h, w, C, s, off, back)
    body = back.view(B, P + off, ld)
    assert torch.equal(body[:, off:, :s * s * C], rows.view(B, P + off, ld)[:, off:, :s * s * C])
    assert bool((body[:, :, s * s * C:] == 7).all()) and (off == 0 or bool((body[:, 0, :s * s * C] == 0).all()))


# ------------------------------------------------------------------------------------------------ the layer
def test_state_dict_init_and_rng_are_those_of_conv_transpose2d():
    torch.manual_seed(11)
    a = nn.ConvTranspose2d(64, 32, kernel_size=2, stride=2)
    after_a = torch.rand(1)
    torch.manual_seed(11)
    b = Deconv2x2(64, 32, kernel_size=2, stride=2)
    after_b = torch.rand(1)
    assert isinstance(b, nn.ConvTranspose2d) and torch.equal(after_a, after_b)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == ["weight", "bias"] and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert tuple(sb["weight"].shape) == (64, 32, 2, 2) and tuple(sb["bias"].shape) == (32,)
    b.load_state_dict(sa, strict=True)
    for bad in (dict(kernel_size=3, stride=2), dict(kernel_size=2, stride=1), dict(padding=1), dict(output_padding=1), dict(groups=2), dict(dilation=2)):
        with pytest.raises(AssertionError):
            Deconv2x2(64, 32, **bad)


@pytest.mark.parametrize("kind", ["nchw", "rows0", "rows1"])
@pytest.mark.parametrize("Cin,Cout,h,w", EXACT_CASES)
def test_exact_operands_bit_for_bit(ops, Cin, Cout, h, w, kind):
    x, wt, bs, dy = exact_operands(2, Cin, Cout, h, w, seed=Cin + Cout + h)
    ref = exact_reference(x, wt, bs, dy)
    m = _layer(ops, wt, bs)
    y, dw, db, dx = _run(m, x, dy, kind[:4], off=int(kind[-1]) if kind != "nchw" else 0)
    assert y.dtype == F32 and torch.equal(y.double(), ref["y"])
    assert dw.dtype == F32 and tuple(dw.shape) == (Cin, Cout, 2, 2) and torch.equal(dw.double(), ref["dw"])
    assert torch.equal(db.double(), ref["db"])
    if kind == "nchw":
        assert torch.equal(dx.double(), ref["dx"])
    yb = _run(m, x, dy, kind[:4], off=int(kind[-1]) if kind != "nchw" else 0, out_dtype=BF)[0]
    assert yb.dtype == BF and torch.equal(yb, rne_bf16(ref["y"]))


def test_the_exact_reference_refuses_a_case_past_two_to_the_24():
    x, wt, bs, dy = exact_operands(1, 64, 16, 1, 1, seed=1)
    with pytest.raises(ExactnessError):
        exact_reference(x * 2.0 ** 20, wt, bs, dy)


@pytest.mark.parametrize("kind", ["nchw", "rows1"])
def test_random_operands_within_the_derived_bounds(ops, kind):
    B, Cin, Cout, h, w = 2, 128, 48, 5, 7
    x, wt, bs, dy = random_operands(B, Cin, Cout, h, w, seed=5)
    ref = reference(x, wt, bs, dy)
    m = _layer(ops, wt, bs)
    y, dw, db, dx = _run(m, x, dy, kind[:4], off=1)
    tokens = B * h * w
    check_bound("y", y, ref["y"], bound(ref["ay"], Cin))
    check_bound("dw", dw, ref["dw"], bound(ref["adw"], tokens))
    check_bound("db", db, ref["db"], bound(ref["adb"], 4 * tokens))
    if kind == "nchw":
        check_bound("dx", dx, ref["dx"], bound(ref["adx"], 4 * Cout))
    yb = _run(m, x, dy, kind[:4], off=1, out_dtype=BF)[0]
    check_bound("y bf16", yb, ref["y"], bound(ref["ay"], Cin, ref["y"], bf16_out=True))


def test_equals_torch_autograd_on_rounded_operands_and_falls_back_without_the_flag(ops):
    x, wt, bs, dy = random_operands(2, 64, 32, 4, 4, seed=9)
    fused, plain, nothing = _layer(ops, wt, bs), _layer(RefOpsBackbone(), wt, bs), _layer(None, wt, bs)
    xin = x.clone().requires_grad_(True)
    assert fused.fused(xin) and not plain.fused(xin) and not nothing.fused(xin)
    want = F.conv_transpose2d(xin, wt, bs, stride=2)
    for m in (plain, nothing):                                # torch's own convolution: the same bits as F.conv_transpose2d
        assert torch.equal(m(xin), want) and m(xin).grad_fn is not None and "Deconv" not in type(m(xin).grad_fn).__name__
        rows = TokenRows(to_rows(x, 1), 2, 4, 4, 1)           # a TokenRows input goes through its NCHW view
        assert torch.equal(m(rows), want)
    got = fused(xin)
    assert "Deconv" in type(got.grad_fn).__name__ and rel_l2(got, want) < 1e-6
    narrow = Deconv2x2(32, 16, ops=ops)                       # Cin % 64 != 0: torch
    assert not narrow.fused(torch.zeros(1, 32, 2, 2))
    with torch.no_grad():                                     # nothing is kept without grad
        y = fused(xin)
    assert y.grad_fn is None and not y.requires_grad


def test_the_gemm_weights_follow_the_parameter_version(ops):
    x, wt, bs, dy = exact_operands(1, 64, 16, 2, 2, seed=3)
    m = _layer(ops, wt, bs)
    Wg, WgT, b4 = m.gemm_weights()
    assert Wg.dtype == BF and tuple(Wg.shape) == (64, 64) and torch.equal(Wg.T.contiguous(), WgT) and torch.equal(b4, bs.repeat(4))
    assert Wg[(2 * 1 + 0) * 16 + 5, 7] == wt[7, 5, 1, 0]
    assert m.gemm_weights()[0] is Wg                          # unchanged parameters: the cached operand
    y0 = m(x)
    with torch.no_grad():
        m.weight.mul_(2.0)                                    # an optimiser step bumps the version counter
    assert m.gemm_weights()[0] is not Wg and torch.equal(m(x), 2 * (y0 - bs.view(1, -1, 1, 1)) + bs.view(1, -1, 1, 1))


# ------------------------------------------------------------------------------------------------ the backbone
@pytest.fixture()
def backbone_factory(monkeypatch, tmp_path):
    from clipself_amd import fvit
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import factory
    cfg = backbone_cfg()
    real = factory.get_tower_cfg
    monkeypatch.setattr(factory, "get_tower_cfg", lambda n: cfg if n == cfg.name else real(n))

    def make(seed, ops, **kw):
        ckpt = tmp_path / f"seed{seed}.pt"
        torch.save(seeded_visual_state(cfg, seed), ckpt)
        return fvit.EvaCLIPViT(cfg.name, str(ckpt), ops=ops, out_indices=OUT_INDICES, **kw)
    return make


@pytest.mark.parametrize("norm", [None, dict(type="BN", requires_grad=True)], ids=["nonorm", "BN"])
def test_fused_backbone_against_the_torch_neck(backbone_factory, ops, norm):
    images, taps, fmap, seed = load_fixture("tiny_fvit_backbone")
    torch.manual_seed(3)
    ref = backbone_factory(seed, ops, norm_cfg=norm, fused_neck=False)
    fused = backbone_factory(seed, ops, norm_cfg=norm, fused_neck=True)
    assert ref.fused_neck is False and fused.fused_neck is True
    assert list(ref.state_dict()) == list(fused.state_dict())
    fused.load_state_dict(ref.state_dict(), strict=True)      # a state dict of the torch neck loads strictly
    neck = [p for n, p in fused.named_parameters() if n.startswith("interpolate")]
    assert all(isinstance(l, Deconv2x2) for l in (fused.interpolate1[0], fused.interpolate1[3], fused.interpolate2[0]))
    for mode in (False, True):
        ref.train(mode), fused.train(mode)
        a, b = ref(images), fused(images)
        assert len(a) == len(b) == 5
        for i in range(4):
            assert a[i].shape == b[i].shape and b[i].dtype == F32
            r = rel_l2(b[i], a[i])
            print(f"train={mode} out{i}: rel-L2 fused vs torch {r:.3e}")
            assert r < (2e-2 if i < 2 else 1e-12)             # bf16 operands against fp32 ones: 2^-9 per rounding, the bound of test_backbone_cpu
        assert (a[4] is None and b[4] is None) if mode else torch.equal(a[4], b[4])
        assert b[0].requires_grad and b[1].requires_grad
    fused.zero_grad()
    (b[0].square().mean() + b[1].square().mean()).backward()
    ref.zero_grad()
    (a[0].square().mean() + a[1].square().mean()).backward()
    got, want = dict(fused.named_parameters()), dict(ref.named_parameters())
    for n in ("interpolate1.0.weight", "interpolate1.0.bias", "interpolate1.3.weight", "interpolate1.3.bias", "interpolate2.0.weight", "interpolate2.0.bias"):
        assert got[n].grad is not None and got[n].grad.shape == got[n].shape, n
        if norm is None:                                      # batch statistics of a 2-image batch amplify rounding: shapes only with BN
            assert rel_l2(got[n].grad, want[n].grad) < 5e-2, (n, rel_l2(got[n].grad, want[n].grad))
    assert all(p.grad is None and not p.requires_grad for p in fused.visual.parameters()) and len(neck) >= 6


def test_flag_handling_and_an_older_state_dict(backbone_factory, ops):
    _, _, _, seed = load_fixture("tiny_fvit_backbone")
    with pytest.raises(NotImplementedError, match="fused_neck"):
        backbone_factory(seed, RefOpsBackbone(), fused_neck=True)
    from clipself_amd import fvit
    auto = backbone_factory(seed, ops)
    assert auto.fused_neck is bool(fvit.FUSED_NECK_DEFAULT)
    assert backbone_factory(seed, RefOpsBackbone()).fused_neck is False
    # the neck as it was before: plain torch modules under the same names
    width = auto.width
    old = nn.ModuleDict(dict(
        interpolate1=nn.Sequential(nn.ConvTranspose2d(width, width, 2, 2), nn.Identity(), nn.GELU(), nn.ConvTranspose2d(width, width, 2, 2)),
        interpolate2=nn.Sequential(nn.ConvTranspose2d(width, width, 2, 2))))
    sd = {k: v for k, v in auto.state_dict().items() if not k.startswith("interpolate")}
    sd.update(old.state_dict())
    assert set(sd) == set(auto.state_dict())
    fused = backbone_factory(seed, ops, fused_neck=True)
    fused.load_state_dict(sd, strict=True)
    assert torch.equal(fused.interpolate1[3].weight, old["interpolate1"][3].weight)


def test_tap_rows_default_leaves_the_launch_list_alone_and_rows_are_the_cast_stream(ops):
    from test_backbone_cpu import _launches, _Recorder
    images, _, _, seed = load_fixture(FIXTURES[0])
    rec = _Recorder(ops)
    eng = build_tower(rec, seed).engine
    rec.calls.clear()
    _, g, maps = eng.encode_dense(images, taps=(0, 1, 2, 3))
    base = _launches(rec.calls)
    rec.calls.clear()
    _, _, maps0 = eng.encode_dense(images, taps=(0, 1, 2, 3), tap_rows=())
    assert _launches(rec.calls) == base and all(torch.equal(a, b) for a, b in zip(maps, maps0))
    rec.calls.clear()
    dense, _, mixed = eng.encode_dense(images, taps=(0, 1, 2, 3), tap_rows=(0, 1))
    got = _launches(rec.calls)
    assert got.count("cast_f32_bf16") == base.count("cast_f32_bf16") + 2 and got.count("tokens_to_nchw") == 2 and len(got) == len(base)
    for k in (0, 1):
        t = mixed[k]
        assert isinstance(t, TokenRows) and (t.B, t.h, t.w, t.off) == (2, g, g, 1) and t.rows.dtype == BF
        assert torch.equal(t.nchw(BF), maps[k].to(BF))        # one rounding of the fp32 tap
    assert torch.equal(mixed[2], maps[2]) and torch.equal(mixed[3], maps[3])
    with pytest.raises(ValueError):
        eng.encode_dense(images, taps=(0, 1), tap_rows=(2,))
    with pytest.raises(ValueError):
        eng.encode_dense(images, tap_rows=(0,))
