"""`-m gpu`: the detector neck's 2x2 transposed convolutions as GEMMs on token rows, on the MI355X.

Kernels alone (HipOps.rows_to_nchw / nchw_to_rows, forms 4 / 5 of cs_transpose_bf16): pure data movement, so bit for bit against the
indexing expressions of tests/_neck_ref.py, with NaN in everything they must not read, and inside the poisoned halos of tests/_extents.py.
Layer (neck.Deconv2x2 on HipOps): exact operands bit for bit against float64 autograd, random operands inside the derived per-element
bounds (tests/_neck_ref.py).  Backbone: EvaCLIPViT(fused_neck=True) against the fp32 reference neck evaluated in float64, at 3 x the worst
MI355X measurement (profiles/neck_parity.md), and end to end in both modes with and without a norm layer."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from _backbone_ref import FIXTURES, OUT_INDICES, backbone_cfg, load_fixture, rel_l2  # noqa: E402
from _extents import run_case  # noqa: E402
from _neck_ref import (BF, BOUND_NECK_GRAD_REL_L2, BOUND_NECK_OUT_REL_L2, EXACT_CASES, F32, KERNEL_SHAPES, bound, check_bound,  # noqa: E402
                       exact_operands, exact_reference, index_nchw_to_rows, index_rows_to_nchw, random_operands, reference, rne_bf16, to_rows)

S_OFF = [(1, 0), (1, 1), (2, 0), (2, 1)]
_INT = {BF: torch.int16, F32: torch.int32}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _lds(s, C):
    """Row strides: the natural one, and one that no 16-byte access can start on (an odd number of elements)."""
    return [s * s * C, s * s * C + 3]


def _rows_data(B, P, off, ld, seed):
    return torch.randn(B * (P + off), ld, generator=torch.Generator().manual_seed(seed))


def _same_bits(got, want, what):
    it = _INT[got.dtype]
    g, w = got.cpu().contiguous().view(it), want.contiguous().view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("s,off", S_OFF)
@pytest.mark.parametrize("B,h,w,C", KERNEL_SHAPES)
def test_rows_to_nchw_is_the_indexing_expression_bit_for_bit(hip, B, h, w, C, s, off):
    assert hip.DECONV_ROWS
    P = h * w
    for ld in _lds(s, C):
        for tin in (F32, BF):
            rows = _rows_data(B, P, off, ld, 100 + P + C).to(tin)
            poisoned = rows.clone()
            if off:
                poisoned.view(B, P + off, ld)[:, 0] = float("nan")                 # the CLS rows are never read
            poisoned[:, s * s * C:] = float("nan")                                 # nor the padding columns
            dev = poisoned.cuda()
            for tout in (F32, BF):
                out = torch.full((B, C, s * h, s * w), 0x7FA5 if tout == BF else 0x7FA5A5A5, dtype=_INT[tout], device="cuda").view(tout)
                hip.rows_to_nchw(dev[:, :s * s * C], B, h, w, C, s, off, out)
                _same_bits(out, index_rows_to_nchw(rows, B, h, w, C, s, off, tout), f"ld={ld} {tin}->{tout}")


@pytest.mark.parametrize("s,off", S_OFF)
@pytest.mark.parametrize("B,h,w,C", KERNEL_SHAPES)
def test_nchw_to_rows_is_the_indexing_expression_bit_for_bit(hip, B, h, w, C, s, off):
    P = h * w
    for ld in _lds(s, C):
        for tin in (F32, BF):
            x = torch.randn(B, C, s * h, s * w, generator=torch.Generator().manual_seed(200 + P + C)).to(tin)
            want = torch.full((B * (P + off), ld), 7.0, dtype=BF)                   # what the kernel leaves alone keeps the fill
            index_nchw_to_rows(x, B, h, w, C, s, off, want)
            rows = torch.full((B * (P + off), ld), 7.0, dtype=BF, device="cuda")
            hip.nchw_to_rows(x.cuda(), B, h, w, C, s, off, rows[:, :s * s * C])
            _same_bits(rows, want, f"ld={ld} {tin}->bf16")


def _halo_case(B, h, w, C, s, off, ld, tin, tout, to_rows_dir):
    P = h * w

    def fn(ops, a):
        if to_rows_dir:
            x = a.inp(torch.randn(B, C, s * h, s * w, generator=torch.Generator().manual_seed(300 + P + C)).to(tin))
            rows = a.out((B * (P + off), s * s * C), BF, ld=a.ld(ld))
            ops.nchw_to_rows(x, B, h, w, C, s, off, rows)
            return {"rows": rows}
        rows = a.inp(_rows_data(B, P, off, ld, 400 + P + C)[:, :s * s * C].to(tin), a.ld(ld))
        out = a.out((B, C, s * h, s * w), tout)
        ops.rows_to_nchw(rows, B, h, w, C, s, off, out)
        return {"out": out}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("s,off", S_OFF)
@pytest.mark.parametrize("B,h,w,C", KERNEL_SHAPES)
def test_kernels_stay_inside_their_extents(hip, B, h, w, C, s, off, pad):
    forms = [(tin, tout, False) for tin in (F32, BF) for tout in (F32, BF)] + [(F32, BF, True), (BF, BF, True)]
    for ld in _lds(s, C):
        for tin, tout, to_rows_dir in forms:
            key = f"{'nchw_to_rows' if to_rows_dir else 'rows_to_nchw'}[{B},{h},{w},{C},{s},{off},{ld},{tin},{tout}]"
            problems = run_case(hip, _halo_case(B, h, w, C, s, off, ld, tin, tout, to_rows_dir), "cuda", pad, key=key)
            assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_entry_point_refuses_bad_forms(hip):
    x = torch.zeros(2 * 5, 32, device="cuda", dtype=BF)
    out = torch.zeros(2, 8, 4, 4, device="cuda")
    p = lambda t: t.data_ptr()
    call = lambda form, ld_rows=32, R=4, C=8, batch=2: hip.lib.cs_transpose_bf16(p(x), ld_rows, p(out), ld_rows, R, C, form, batch, None)
    good = 4 | 1 << 8 | 1 << 9 | 1 << 10 | 2 << 12                                  # rows -> NCHW, s = 2, off = 1, bf16 rows, fp32 map, w = 2
    assert call(good) == 0
    torch.cuda.synchronize()
    assert call(3) == -1 and b"form 3" in hip.lib.cs_last_error()                  # still no such form
    assert call(6 | 2 << 12) == -1
    assert call(good, ld_rows=31) == -1 and b"stride" in hip.lib.cs_last_error()    # rows narrower than s*s*C
    assert call(4 | 1 << 8 | 1 << 10 | 3 << 12) == -1                               # h*w is no multiple of w
    assert call(4 | 1 << 10) == -1                                                  # w = 0
    assert call(5 | 1 << 8 | 2 << 12) == -1 and b"bf16 rows" in hip.lib.cs_last_error()      # NCHW -> rows writes bf16 only
    with pytest.raises(AssertionError):
        hip.rows_to_nchw(x, 2, 2, 2, 8, 2, 1, out.permute(0, 1, 3, 2))              # the map is contiguous
    with pytest.raises(AssertionError):
        hip.nchw_to_rows(out, 2, 2, 2, 8, 2, 1, x.float())                          # bf16 rows


# ------------------------------------------------------------------------------------------------ the layer
def _layer(hip, weight, bias):
    from clipself_amd.neck import Deconv2x2
    m = Deconv2x2(weight.shape[0], weight.shape[1], ops=hip)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    return m.cuda()


def _run(m, x, dy, kind, off=1, out_dtype=F32):
    from clipself_amd.neck import TokenRows
    m.zero_grad()
    if kind == "nchw":
        inp = x.cuda().to(out_dtype).requires_grad_(True)
        assert m.fused(inp)
        y = m(inp)
    else:
        B, C, h, w = x.shape
        m.out_dtype = out_dtype
        inp = None
        y = m(TokenRows(to_rows(x, off).cuda(), B, h, w, off))
    assert "Deconv" in type(y.grad_fn).__name__
    y.backward(dy.cuda().to(y.dtype))
    return y.detach(), m.weight.grad, m.bias.grad, None if inp is None else inp.grad


@pytest.mark.parametrize("kind", ["nchw", "rows0", "rows1"])
@pytest.mark.parametrize("Cin,Cout,h,w", EXACT_CASES)
def test_exact_operands_bit_for_bit(hip, Cin, Cout, h, w, kind):
    x, wt, bs, dy = exact_operands(2, Cin, Cout, h, w, seed=Cin + Cout + h)
    ref = exact_reference(x, wt, bs, dy)
    m = _layer(hip, wt, bs)
    off = 0 if kind == "nchw" else int(kind[-1])
    y, dw, db, dx = _run(m, x, dy, kind[:4], off)
    eq = lambda got, want, what: _same_bits(got, want.to(F32), what)
    assert y.dtype == F32 and dw.dtype == F32 and tuple(dw.shape) == (Cin, Cout, 2, 2)
    eq(y, ref["y"], "forward")
    eq(dw, ref["dw"], "weight gradient")
    eq(db, ref["db"], "bias gradient")
    if kind == "nchw":
        eq(dx, ref["dx"], "input gradient")
    yb = _run(m, x, dy, kind[:4], off, out_dtype=BF)[0]
    assert yb.dtype == BF
    _same_bits(yb, rne_bf16(ref["y"]), "bf16 forward")
    again = _run(m, x, dy, kind[:4], off)
    assert all(torch.equal(a, b) for a, b in zip((y, dw, db), again[:3]))            # the same inputs, the same bits


# one token tile and odd grid | several row tiles of the GEMMs, several channel tiles
@pytest.mark.parametrize("B,Cin,Cout,h,w", [(2, 128, 48, 5, 7), (3, 256, 64, 16, 16)])
@pytest.mark.parametrize("kind", ["nchw", "rows1"])
def test_random_operands_within_the_derived_bounds(hip, kind, B, Cin, Cout, h, w):
    x, wt, bs, dy = random_operands(B, Cin, Cout, h, w, seed=5)
    ref = reference(x, wt, bs, dy)
    m = _layer(hip, wt, bs)
    y, dw, db, dx = _run(m, x, dy, kind[:4], off=1)
    tokens = B * h * w
    check_bound("y", y, ref["y"], bound(ref["ay"], Cin))
    check_bound("dw", dw, ref["dw"], bound(ref["adw"], tokens))
    check_bound("db", db, ref["db"], bound(ref["adb"], 4 * tokens))
    if kind == "nchw":
        check_bound("dx", dx, ref["dx"], bound(ref["adx"], 4 * Cout))
    yb = _run(m, x, dy, kind[:4], off=1, out_dtype=BF)[0]
    check_bound("y bf16", yb, ref["y"], bound(ref["ay"], Cin, ref["y"], bf16_out=True))


# ------------------------------------------------------------------------------------------------ the backbone
@pytest.fixture()
def backbone_factory(monkeypatch, tmp_path):
    from clipself_amd import fvit
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import factory
    cfg = backbone_cfg()
    real = factory.get_tower_cfg
    monkeypatch.setattr(factory, "get_tower_cfg", lambda n: cfg if n == cfg.name else real(n))

    def make(seed, **kw):
        ckpt = tmp_path / f"seed{seed}.pt"
        torch.save(seeded_visual_state(cfg, seed), ckpt)
        return fvit.EvaCLIPViT(cfg.name, str(ckpt), out_indices=OUT_INDICES, **kw).cuda()
    return make


def _reference_neck(m):
    """The neck the reference runs -- nn.ConvTranspose2d modules on unrounded operands -- in float64 on the CPU, with m's parameters."""
    width = m.width
    ref = nn.ModuleDict(dict(
        interpolate1=nn.Sequential(nn.ConvTranspose2d(width, width, 2, 2), nn.Identity(), nn.GELU(), nn.ConvTranspose2d(width, width, 2, 2)),
        interpolate2=nn.Sequential(nn.ConvTranspose2d(width, width, 2, 2))))
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith("interpolate")}, strict=True)
    return ref.double()


@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_reference_neck(hip, backbone_factory, name):
    images, _, _, seed = load_fixture(name)
    torch.manual_seed(17)
    m = backbone_factory(seed, fused_neck=True).train()
    assert type(m.visual.engine.ops).__name__ == "HipOps" and m.fused_neck
    outs = m(images.cuda())
    gen = torch.Generator().manual_seed(23)
    g0, g1 = (torch.randn(o.shape, generator=gen) for o in outs[:2])
    (outs[0] * g0.cuda()).sum().backward(retain_graph=True)
    (outs[1] * g1.cuda()).sum().backward()
    taps, _ = m.visual.forward_intermediates(images.cuda(), OUT_INDICES, final_map=False)      # the fp32 taps of the same frozen pass
    ref = _reference_neck(m)
    r0, r1 = ref["interpolate1"](taps[0].cpu().double()), ref["interpolate2"](taps[1].cpu().double())
    ((r0 * g0.double()).sum() + (r1 * g1.double()).sum()).backward()
    worst_out = max(rel_l2(outs[0], r0), rel_l2(outs[1], r1))
    print(f"NECK PARITY {name} out0 rel-L2 {rel_l2(outs[0], r0):.4e} out1 rel-L2 {rel_l2(outs[1], r1):.4e}")
    worst_grad, got = 0.0, dict(m.named_parameters())
    for n, p in ref.named_parameters():
        r = rel_l2(got[n].grad, p.grad)
        worst_grad = max(worst_grad, r)
        print(f"NECK PARITY {name} grad {n} rel-L2 {r:.4e}")
    assert worst_out <= BOUND_NECK_OUT_REL_L2, (worst_out, BOUND_NECK_OUT_REL_L2)
    assert worst_grad <= BOUND_NECK_GRAD_REL_L2, (worst_grad, BOUND_NECK_GRAD_REL_L2)


@pytest.mark.parametrize("norm", [None, dict(type="BN", requires_grad=True)], ids=["nonorm", "BN"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_backbone_module_end_to_end(hip, backbone_factory, train, norm):
    images, _, _, seed = load_fixture(FIXTURES[1])
    m = backbone_factory(seed, fused_neck=True, norm_cfg=norm).train(train)
    outs = m(images.cuda())
    assert [tuple(o.shape) for o in outs[:4]] == [(2, 128, 24, 24), (2, 128, 12, 12), (2, 128, 6, 6), (2, 128, 3, 3)]
    assert (outs[4] is None) if train else tuple(outs[4].shape) == (2, 64, 6, 6)
    assert all(o.is_cuda and o.dtype == F32 for o in outs[:4])
    assert [o.requires_grad for o in outs[:4]] == [True, True, False, False]
    assert "Deconv" in type(outs[1].grad_fn).__name__
    (outs[0].square().mean() + outs[1].square().mean()).backward()
    p = dict(m.named_parameters())
    for n in ("interpolate1.0.weight", "interpolate1.0.bias", "interpolate1.3.weight", "interpolate1.3.bias", "interpolate2.0.weight", "interpolate2.0.bias"):
        assert p[n].grad is not None and p[n].grad.is_cuda and bool(torch.isfinite(p[n].grad).all()) and float(p[n].grad.abs().sum()) > 0, n
    assert all(q.grad is None for q in m.visual.parameters())
