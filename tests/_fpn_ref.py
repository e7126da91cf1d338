"""TEST INFRASTRUCTURE -- the detector's feature pyramid (clipself_amd/fpn.py, conv.Conv1x1, forms 7 / 8 of cs_transpose_bf16 in
include/clipself_hip.h).

* `RefOpsFPN`: the CPU backend of the other detector layers (tests/_fc_ref.RefOpsFC) plus `upsample2x_add` / `pool2x` restated from the
  header's text in np.float32, element by element through explicit row indices: fine row = b*4*h*w + (2i + di)*(2w) + 2j + dj, the pool's
  sum ((f00 + f01) + f10) + f11 in that order, one rounding at the output's type.  Conv1x1 runs on the inherited gemm_nt / gemm_wgrad_tn /
  colsum_bf16.  `flaws` plants the errors the checks must reject: "fine_width_w" (fine rows indexed with w instead of 2w), "pool_drops_tap",
  "ignores_accumulate".
* `TwinFPN`: mmdet 2.28's FPN.forward written with nn.Conv2d / nn.BatchNorm2d under the module's key names; the reference of every
  comparison, in float64 for the exact cases and in fp32 for the random one.
* `FlawedFPN`: the module with a planted error in its forward: "up_lateral" (level i receives up(lateral[i + 1]) instead of
  up(merged[i + 1])), "lateral_relu" (the laterals' ConvModule carries a ReLU), "extra_from_merged" (the extra level is taken from
  merged[3] instead of outs[3]).
* Exact operands: sparse small integers (`exact_case`), so that every intermediate of the float64 twin is an integer of magnitude <= 256
  (bf16 holds it: the kernel route rounds laterals, merged maps and gradients to bf16 GEMM operands) and every sum of |terms| -- bounded
  by running the twin on the operands' absolute values -- stays below 2^24, where fp32 accumulation in any order is exact.
  `assert_exact` checks that condition on the twin, not on the code under test.
* Random operands with norm: relative L2 per tensor against the fp32 twin.  Measured (profiles/fpn_parity.md; the CPU backend and the
  MI355X agree to four digits): 2.64e-3 worst over outputs and input gradients, 2.83e-3 over parameter gradients.  Twice those would
  pass the 3.4e-3 of profiles/neck_parity.md that the thresholds must not exceed, so PARITY_* sit at that cap; the profile says why the
  figures are where they are (one bf16 rounding of a GEMM operand is about 1.6e-3 rms; outputs see one, gradients two)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import _fc_ref
from _fc_ref import RefOpsFC
from _neck_ref import BF, F32, TWO24, ExactnessError

F64 = torch.float64
# The reference's neck, restated from F-ViT/configs/fvit_vitb16_upsample_fpn_bs64_3e_ovcoco_eva_original.py (`type` dropped: the registry key)
REFERENCE_NECK = dict(in_channels=[768, 768, 768, 768], out_channels=256, norm_cfg=dict(type="SyncBN", requires_grad=True), num_outs=5)
# (B, [(h, w) per level]) of the exact cases: levels 16 / 8 / 4 / 2, and three levels with h != w
EXACT_GEOMS = {"square4": (2, [(16, 16), (8, 8), (4, 4), (2, 2)]), "wide3": (2, [(12, 20), (6, 10), (3, 5)])}
# rel-L2 thresholds of the random case with norm: the cap, 3.4e-3 (2 x the measured 2.64e-3 / 2.83e-3 would exceed it: profiles/fpn_parity.md)
PARITY_OUT_REL_L2, PARITY_GRAD_REL_L2 = 3.4e-3, 3.4e-3


# ------------------------------------------------------------------------------------------------ the ops, from the header's text
def _np32(t):
    return t.detach().to(F32).numpy().astype(np.float32)


def _fine_rows(B, h, w, di, dj, fine_w):
    b, i, j = np.meshgrid(np.arange(B), np.arange(h), np.arange(w), indexing="ij")
    return (b * 4 * h * w + (2 * i + di) * fine_w + 2 * j + dj).reshape(-1)


class RefOpsFPN(RefOpsFC):
    name = "ref+taps+neck+conv+bn+fc+fpn"
    FPN_TOPDOWN = True

    def __init__(self, flaws=()):
        super().__init__()
        self.flaws = tuple(flaws)

    @staticmethod
    def _check(coarse, fine, B, h, w, C):
        if w <= 0 or min(B, h, C) <= 0 or B * h * w * C >= 1 << 31:
            raise RuntimeError("cs_transpose_bf16 (FPN top-down): w > 0, R a multiple of w, batch * R * C <= 2^31 - 1")
        for t, rows in ((coarse, B * h * w), (fine, 4 * B * h * w)):
            assert t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == rows and t.shape[1] == C and t.dtype in (F32, BF)
            if t.stride(0) < C:
                raise RuntimeError("cs_transpose_bf16 (FPN top-down): a row stride below C")

    def upsample2x_add(self, coarse, fine, B, h, w, C, accumulate=True):
        self._check(coarse, fine, B, h, w, C)
        c = _np32(coarse)
        acc = accumulate and "ignores_accumulate" not in self.flaws
        fw = w if "fine_width_w" in self.flaws else 2 * w
        for di in (0, 1):
            for dj in (0, 1):
                idx = torch.from_numpy(_fine_rows(B, h, w, di, dj, fw))
                v = (_np32(fine[idx]) + c) if acc else c
                fine[idx] = torch.from_numpy(v.astype(np.float32)).to(fine.dtype)

    def pool2x(self, fine, coarse, B, h, w, C, accumulate=False):
        self._check(coarse, fine, B, h, w, C)
        f = [_np32(fine[torch.from_numpy(_fine_rows(B, h, w, di, dj, 2 * w))]) for di in (0, 1) for dj in (0, 1)]
        s = (f[0] + f[1]) + f[2]
        if "pool_drops_tap" not in self.flaws:
            s = s + f[3]
        if accumulate:
            s = _np32(coarse) + s
        coarse.copy_(torch.from_numpy(s.astype(np.float32)).to(coarse.dtype))


# ------------------------------------------------------------------------------------------------ the twin
class TwinConvModule(nn.Module):
    def __init__(self, cin, cout, k, norm):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=not norm)
        if norm:
            self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        x = self.conv(x)
        return self.bn(x) if hasattr(self, "bn") else x


class TwinFPN(nn.Module):
    """mmdet/models/necks/fpn.py FPN.forward (add_extra_convs=False, upsample_cfg=dict(mode='nearest')).  forward keeps its intermediates
    (laterals, merged) for the exactness check."""

    def __init__(self, in_channels, out_channels, num_outs, norm_cfg=None, **_):
        super().__init__()
        norm = norm_cfg is not None
        self.num_outs = num_outs
        self.lateral_convs = nn.ModuleList(TwinConvModule(c, out_channels, 1, norm) for c in in_channels)
        self.fpn_convs = nn.ModuleList(TwinConvModule(out_channels, out_channels, 3, norm) for _ in in_channels)

    def forward(self, inputs):
        laterals = [m(x) for m, x in zip(self.lateral_convs, inputs)]
        self.laterals = list(laterals)
        for t in laterals:
            if t.requires_grad:
                t.retain_grad()
        for i in range(len(laterals) - 1, 0, -1):
            laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], size=laterals[i - 1].shape[2:], mode="nearest")
        self.merged = laterals
        for t in self.merged:
            if t.requires_grad:
                t.retain_grad()
        outs = [m(x) for m, x in zip(self.fpn_convs, laterals)]
        self.outs = list(outs)
        for t in outs:
            if t.requires_grad:
                t.retain_grad()
        for _ in range(self.num_outs - len(outs)):
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return tuple(outs)


def flawed_fpn(flaw, *args, **kw):
    """clipself_amd.fpn.FPN with one planted error in its forward."""
    from clipself_amd.fpn import FPN

    class FlawedFPN(FPN):
        def forward(self, inputs):
            lat = [conv(x) for conv, x in zip(self.lateral_convs, inputs)]
            if flaw == "lateral_relu":
                lat = [F.relu(t) for t in lat]
            merged = list(lat)
            for i in range(self.num_ins - 1, 0, -1):
                merged[i - 1] = self._merge(merged[i - 1], lat[i] if flaw == "up_lateral" else merged[i])
            outs = [conv(x) for conv, x in zip(self.fpn_convs, merged)]
            for _ in range(self.num_outs - self.num_ins):
                src = merged[-1] if flaw == "extra_from_merged" and len(outs) == self.num_ins else outs[-1]
                outs.append(F.max_pool2d(src, 1, stride=2))
            return tuple(outs)
    assert flaw in ("up_lateral", "lateral_relu", "extra_from_merged"), flaw
    return FlawedFPN(*args, **kw)


def copy_state(dst, src):
    """src's state dict into dst, strict, as fp32 (or dst's own dtype)."""
    dst.load_state_dict({k: v.detach().to(dst.state_dict()[k].dtype) for k, v in src.state_dict().items()}, strict=True)
    return dst


# ------------------------------------------------------------------------------------------------ exact operands
def _sparse_int(g, shape, lo, hi, keep):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F32)
    return v * (torch.rand(shape, generator=g) < keep).to(F32)


@functools.lru_cache(maxsize=None)
def exact_case(name, C=64, seed=0):
    """(twin in float64 with its gradients, inputs, upstream gradients, outs, input gradients) of EXACT_GEOMS[name]: in_channels = out_channels = C,
    norm_cfg=None, one extra level.  Computed once and shared read-only."""
    B, levels = EXACT_GEOMS[name]
    g = torch.Generator().manual_seed(1000 + seed + len(levels))
    n = len(levels)
    twin = TwinFPN([C] * n, C, n + 1).double()
    with torch.no_grad():
        for m in twin.lateral_convs:
            m.conv.weight.copy_(_sparse_int(g, m.conv.weight.shape, -1, 1, 1 / 8))
            m.conv.bias.copy_(_sparse_int(g, m.conv.bias.shape, -2, 2, 1 / 2))
        for m in twin.fpn_convs:
            m.conv.weight.copy_(_sparse_int(g, m.conv.weight.shape, -1, 1, 1 / 32))
            m.conv.bias.copy_(_sparse_int(g, m.conv.bias.shape, -2, 2, 1 / 2))
    xs = [_sparse_int(g, (B, C, h, w), -2, 2, 1 / 4) for h, w in levels]
    sizes = list(levels) + [((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2)]
    gs = [_sparse_int(g, (B, C, h, w), -2, 2, 1 / 16) for h, w in sizes]
    ins = [x.double().requires_grad_(True) for x in xs]
    outs = twin(ins)
    torch.autograd.backward(outs, [t.double() for t in gs])
    assert_exact(twin, ins, gs, outs)
    return twin, xs, gs, [o.detach() for o in outs], [t.grad for t in ins]


def assert_exact(twin, ins, gs, outs):
    """The condition the exact comparison rests on, checked on the float64 twin: every intermediate a bf16 operand is made of is an integer of
    magnitude <= 256, every result an integer fp32 holds, and every sum of |terms| (the twin run on absolute values) is below 2^24."""
    def ints(t, what, limit):
        if not (torch.equal(t, t.round()) and float(t.abs().max()) <= limit):
            raise ExactnessError(f"{what}: max |v| {float(t.abs().max())} (limit {limit}) or a non-integer: the case, not a kernel, is wrong")
    for i, (lat, mer) in enumerate(zip(twin.laterals, twin.merged)):
        ints(lat.detach(), f"lateral {i}", 256)
        ints(mer.detach(), f"merged {i}", 256)
        ints(mer.grad, f"gradient of merged {i}", 256)
    for i, t in enumerate(gs):
        ints(t, f"upstream gradient {i}", 256)
    for i, t in enumerate(ins):
        ints(t.detach(), f"input {i}", 256)
    results = [o.detach() for o in outs] + [t.grad for t in ins] + [p.grad for p in twin.parameters()]
    for t in results:
        ints(t, "a result", TWO24 - 1)
    # sums of |terms|: the same graph on absolute values bounds every accumulation, forward and backward
    mag = TwinFPN([ins[0].shape[1]] * len(ins), outs[0].shape[1], len(outs)).double()
    mag.load_state_dict({k: v.abs() for k, v in twin.state_dict().items()})
    ains = [t.detach().abs().requires_grad_(True) for t in ins]
    aouts = mag(ains)
    torch.autograd.backward(aouts, [t.double().abs() for t in gs])
    worst = max(float(t.max()) for t in [o.detach() for o in aouts] + [t.grad for t in ains] + [p.grad for p in mag.parameters()])
    if not worst < TWO24:
        raise ExactnessError(f"a sum of |terms| reaches {worst} >= 2^24: fp32 accumulation is not exact for this case")


def run_module(m, xs, gs, dtype=F32, device="cpu", channels_last=False):
    """One forward + backward of an FPN-like module -> (outs, input gradients, {parameter name: gradient})."""
    m.zero_grad()
    ins = []
    for x in xs:
        t = x.detach().to(device).to(dtype).clone()
        if channels_last:
            t = t.contiguous(memory_format=torch.channels_last)
        ins.append(t.requires_grad_(True))
    outs = m(tuple(ins))
    torch.autograd.backward(outs, [t.to(device).to(o.dtype) for t, o in zip(gs, outs)])
    return [o.detach() for o in outs], [t.grad for t in ins], {n: p.grad for n, p in m.named_parameters()}


def same_bits(got, want, what):
    """got (any strides, any device) has exactly the bits of want cast to got's dtype.  The sign of a zero is not compared (x + 0.0 maps
    -0 to +0 and nothing else): a gradient accumulated into a zeroed buffer is +0 where float64 autograd writes a lone product -0."""
    it = {BF: torch.int16, F32: torch.int32}[got.dtype]
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    g, w = (got.detach().cpu().contiguous() + 0.0).view(it), (want.detach().to(got.dtype).contiguous() + 0.0).view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


def check_exact(make, name, device="cpu"):
    """make(in_channels, out_channels, num_outs) -> the module under test; its five outputs, input gradients and parameter gradients on
    the exact case `name` must have the float64 twin's bits."""
    twin, xs, gs, outs, dxs = exact_case(name)
    C, n = xs[0].shape[1], len(xs)
    m = copy_state(make([C] * n, C, n + 1), twin).to(device)
    got_outs, got_dx, got_dp = run_module(m, xs, gs, device=device)
    assert len(got_outs) == n + 1
    for i, (a, b) in enumerate(zip(got_outs, outs)):
        same_bits(a, b, f"{name}: output {i}")
    for i, (a, b) in enumerate(zip(got_dx, dxs)):
        same_bits(a, b, f"{name}: gradient of input {i}")
    want = {k: p.grad for k, p in twin.named_parameters()}
    assert sorted(got_dp) == sorted(want)
    for k in want:
        same_bits(got_dp[k], want[k], f"{name}: gradient of {k}")


# ------------------------------------------------------------------------------------------------ random operands, with norm
def _bf(t):
    return t.to(BF).to(F32)


@functools.lru_cache(maxsize=None)
def random_case(seed=7, C=64, Cout=64, B=2):
    """The fp32 twin in training mode with norm on levels 16 / 8 / 4 / 2 and its results: (state dict, xs, gs, outs, dx, parameter
    gradients, {bn.bias name: per-channel sum of |terms| of that gradient}).  Inputs, convolution weights and upstream gradients are fp32
    values that bf16 holds exactly (the convention of tests/_neck_ref.random_operands): what is measured is the route, not the rounding
    of its operands."""
    levels = EXACT_GEOMS["square4"][1]
    torch.manual_seed(seed)
    twin = TwinFPN([C] * 4, Cout, 5, norm_cfg=dict(type="BN")).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in twin.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(_bf(m.weight))
    state = {k: v.clone() for k, v in twin.state_dict().items()}
    xs = [_bf(torch.randn(B, C, h, w, generator=g)) for h, w in levels]
    gs = [_bf(torch.randn(B, Cout, h, w, generator=g)) for h, w in list(levels) + [(1, 1)]]
    outs, dx, dp = run_module(twin, xs, gs)
    terms = {}
    for i in range(4):
        terms[f"lateral_convs.{i}.bn.bias"] = twin.laterals[i].grad.abs().sum((0, 2, 3))
        terms[f"fpn_convs.{i}.bn.bias"] = twin.outs[i].grad.abs().sum((0, 2, 3))
    return state, xs, gs, outs, dx, dp, terms


def rel_l2(got, want, scale=None):
    """|got - want| / |want| in L2; with `scale`, |got - want| / |scale|."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / (want if scale is None else scale.double()).norm().clamp_min(1e-300))


def parity(make, device="cpu", tag="CPU backend"):
    """(worst rel-L2 over outputs and input gradients, worst rel-L2 over parameter gradients) of the module against the fp32 twin on the
    random case; every figure is printed.  A bn.bias gradient is a plain sum over the pixels, and the laterals' is a sum that cancels
    (the batch norm behind the output convolution returns a gradient whose sum over the pixels is zero, so only the convolution's border
    terms survive): its error is measured against the sum of |terms|, the scale a sum's rounding error has."""
    state, xs, gs, outs, dx, dp, terms = random_case()
    m = make([64] * 4, 64, 5, norm_cfg=dict(type="BN")).train()
    m.load_state_dict(state, strict=True)
    m = m.to(device)
    got_outs, got_dx, got_dp = run_module(m, xs, gs, device=device)
    worst_out = worst_grad = 0.0
    for i, (a, b) in enumerate(zip(got_outs, outs)):
        r = rel_l2(a, b)
        worst_out = max(worst_out, r)
        print(f"FPN PARITY [{tag}] output {i} rel-L2 {r:.4e}")
    for i, (a, b) in enumerate(zip(got_dx, dx)):
        r = rel_l2(a, b)
        worst_out = max(worst_out, r)
        print(f"FPN PARITY [{tag}] input gradient {i} rel-L2 {r:.4e}")
    assert sorted(got_dp) == sorted(dp)
    for k in dp:
        r = rel_l2(got_dp[k], dp[k], terms.get(k))
        worst_grad = max(worst_grad, r)
        print(f"FPN PARITY [{tag}] grad {k} rel-L2 {r:.4e}" + (" (against the sum of |terms|)" if k in terms else ""))
    return worst_out, worst_grad


# ------------------------------------------------------------------------------------------------ Conv1x1 alone
# (M rows, Cin, Cout) -> (N, H, W) with N*H*W == M: one row | a ragged row count, two K tiles, Cout % 64 != 0 (padded dgrad) | three K tiles
CONV1X1_SHAPES = {(1, 64, 8): (1, 1, 1), (130, 128, 72): (2, 5, 13), (300, 192, 256): (3, 10, 10)}
LAYOUTS = [("nchw", F32), ("channel_last", F32), ("channel_last", BF)]


def conv1x1_layer(ops, weight, bias, device="cpu"):
    from clipself_amd.conv import Conv1x1
    m = Conv1x1(weight.shape[1], weight.shape[0], ops=ops, fused=True)
    with torch.no_grad():
        m.weight.copy_(weight.view_as(m.weight))
        m.bias.copy_(bias)
    return m.to(device)


def run_conv1x1(m, x, dy, geom, layout, dtype):
    """x [M, Cin], dy [M, Cout] rows -> (y rows, dx rows, dw [Cout, Cin], db) of one forward + backward on the map of that layout."""
    N, H, W = geom
    dev = m.weight.device
    m.zero_grad()
    inp = x.to(dev).to(dtype).view(N, H, W, -1).permute(0, 3, 1, 2)
    if layout == "nchw":
        inp = inp.contiguous()
    inp = inp.detach().requires_grad_(True)
    y = m(inp)
    assert y.dtype == dtype and y.permute(0, 2, 3, 1).is_contiguous() and "Conv1x1" in type(y.grad_fn).__name__
    y.backward(dy.to(dev).to(dtype).view(N, H, W, -1).permute(0, 3, 1, 2).contiguous())
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N * H * W, -1)
    return rows(y.detach()), rows(inp.grad), m.weight.grad.view(m.out_channels, m.in_channels), m.bias.grad


def check_conv1x1(ops, shape, layout, dtype, kind, device="cpu"):
    x, w, b, dy, ref = _fc_ref.case(shape, kind, act=None)
    M, Cin, Cout = shape
    y, dx, dw, db = run_conv1x1(conv1x1_layer(ops, w, b, device), x, dy, CONV1X1_SHAPES[shape], layout, dtype)
    assert dx.dtype == dtype and dw.dtype == F32 and db.dtype == F32
    if kind == "exact":
        for got, key in ((y, "y"), (dx, "dx"), (dw, "dw"), (db, "db")):
            same_bits(got, ref[key], f"{shape} {layout} {dtype}: {key}")
        return
    bf = dtype == BF
    _fc_ref.check_bound("y", y, ref["y"], _fc_ref.bound(ref["ay"], Cin, 1, ref["y"], bf))
    _fc_ref.check_bound("dx", dx, ref["dx"], _fc_ref.bound(ref["adx"], Cout, 1, ref["dx"], bf))
    _fc_ref.check_bound("dw", dw, ref["dw"], _fc_ref.bound(ref["adw"], M))
    _fc_ref.check_bound("db", db, ref["db"], _fc_ref.bound(ref["adb"], M))
