"""TEST INFRASTRUCTURE -- the thin 1 x 1 convolutions and the two head assemblies built on them (conv.Conv1x1Thin, conv.thin_heads,
clipself_amd/rpn_head.py, clipself_amd/mask_head.py, epilogues 10 / 11 of cs_gemm_nt in include/clipself_hip.h).

* `RefOpsThin`: the CPU backend of the other detector layers (tests/_fpn_ref.RefOpsFPN) plus `thin_fwd` / `thin_dgrad` restated from the
  header's text in np.float32, every element placed through its explicit index: rows T[m * ld + n]; planes P1[((m / R) * s + n) * R + m % R]
  and P2[((m / R) * (N - s) + (n - s)) * R + m % R] with P2 = P1 + M * s in the forward.  It is a host backend that serves host tensors.
  `flaws` plants the errors the checks must reject: "split_off_by_one", "plane_index_swapped" (m % R and m / R exchanged),
  "bias_second_block_only", "gate_lt" (the gate tested as < 0), "dy_not_rounded", "second_block_ignored".
* The twins: mmdet 2.28's RPNHead.forward_single (dense_heads/rpn_head.py, with F-ViT/models/custom_rpn_head.py's _init_layers) and
  FCNMaskHead.forward (roi_heads/mask_heads/fcn_mask_head.py) written with nn.Conv2d / nn.BatchNorm2d / nn.ConvTranspose2d under the
  modules' key names.  Parity-unpinned: mmdet is cited, not run; the layers themselves are torch's own F.conv2d / F.conv_transpose2d under
  float64 autograd, the reference of every comparison.
* Exact operands: sparse small integers, so that every intermediate of the float64 twin that the kernel route rounds to a bf16 operand is
  an integer of magnitude <= 256 and every sum of |terms| -- bounded by running the twin on absolute values, where every ReLU passes --
  stays below 2^24, where fp32 accumulation in any order is exact.  `assert_exact` checks that on the twin, not on the code under test.
* Random operands (Conv1x1Thin / thin_heads alone): the bounds of tests/_fc_ref.bound, 2 * (K + 2) * 2^-24 * sum|terms| per element for the
  fp32 results plus 2^-8 * (|ref| + bound) where the result is bf16.  Derived, not measured.
* The module with norm on random operands: relative L2 against the fp32 twin; the threshold is the 3.4e-3 of profiles/neck_parity.md and
  profiles/fpn_parity.md (the same bf16 operand roundings), the measured values are in profiles/thin_heads_parity.md."""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import _fc_ref
from _fpn_ref import RefOpsFPN, _sparse_int, copy_state, rel_l2, same_bits  # noqa: F401
from _neck_ref import BF, F32, TWO24, ExactnessError

F64 = torch.float64
PARITY_REL_L2 = 3.4e-3
FLAWS = ("split_off_by_one", "plane_index_swapped", "bias_second_block_only", "gate_lt", "dy_not_rounded", "second_block_ignored")
# The reference's heads, restated from F-ViT/configs/ov_lvis/fvit_vitb16_upsample_fpn_bs64_4x_ovlvis_eva_original.py (norm_cfg and
# head_norm_cfg are that file's dict(type='SyncBN', requires_grad=True))
REFERENCE_RPN_HEAD = dict(
    type="CustomRPNHead", in_channels=256, feat_channels=256,
    anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
    bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[0.0, 0.0, 0.0, 0.0], target_stds=[1.0, 1.0, 1.0, 1.0]),
    loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
    num_convs=2, norm_cfg=dict(type="SyncBN", requires_grad=True))
REFERENCE_MASK_HEAD = dict(
    type="FCNMaskHead", num_convs=4, in_channels=256, conv_out_channels=256, num_classes=1203,
    loss_mask=dict(type="CrossEntropyLoss", use_mask=True, loss_weight=1.0), class_agnostic=True,
    norm_cfg=dict(type="SyncBN", requires_grad=True))


# ------------------------------------------------------------------------------------------------ the ops, from the header's text
def _np32(t):
    return t.detach().to(F32).numpy().astype(np.float32)


class RefOpsThin(RefOpsFPN):
    name = "ref+taps+neck+conv+bn+fc+fpn+thin"
    THIN_HEADS = True

    def __init__(self, flaws=()):
        super().__init__()
        self.flaws = tuple(flaws)
        assert all(f in FLAWS for f in self.flaws), self.flaws

    def _plane_offsets(self, M, N, R, s):
        """offs [M, N] (element offsets) and second [N] (column lives in P2) of the planes form."""
        if "split_off_by_one" in self.flaws and s < N:
            s = s + 1
        m = np.arange(M, dtype=np.int64)[:, None]
        n = np.arange(N, dtype=np.int64)[None, :]
        img, pix = m // R, m % R
        if "plane_index_swapped" in self.flaws:
            img, pix = m % (M // R), m // (M // R)
        first = n < s
        offs = np.where(first, (img * s + n) * R + pix, (img * (N - s) + (n - s)) * R + pix)
        return offs, ~first[0], s

    @staticmethod
    def _check_thin(krows, W, M, N, K, R, s):
        if N > 16 or N < 1 or K % 64 or K <= 0 or M <= 0:
            raise RuntimeError("cs_gemm_nt (thin): 1 <= N <= 16, K a positive multiple of 64")
        if R < 0 or (R and M % R):
            raise RuntimeError("cs_gemm_nt (thin): group is 0 or a divisor of M")
        if R and not 1 <= s <= N:
            raise RuntimeError("cs_gemm_nt (thin): split outside [1, N]")
        assert krows.dim() == 2 and krows.stride(1) == 1 and krows.dtype in (F32, BF) and tuple(krows.shape) == (M, K)
        assert W.dtype == BF and tuple(W.shape) == (N, K) and W.stride(1) == 1
        if M > 1 and krows.stride(0) < K:
            raise RuntimeError("cs_gemm_nt (thin): a row stride below K")

    def thin_fwd(self, X, W, bias, out, R=0, split=None):
        M, K = X.shape
        N = W.shape[0]
        s = N if split is None else int(split)
        self._check_thin(X, W, M, N, K, R, s)
        assert out.dtype == F32 and (bias is None or (bias.dtype == F32 and bias.numel() == N))
        acc = _np32(X.to(BF)) @ _np32(W).T                               # fp32 rows are rounded to bf16 (RNE) first
        if bias is not None:
            b = _np32(bias).copy()
            if "bias_second_block_only" in self.flaws and R and s < N:
                b[:s] = 0
            acc = acc + b[None, :]
        acc = torch.from_numpy(acc.astype(np.float32))
        if R == 0:
            assert tuple(out.shape) == (M, N) and out.stride(1) == 1
            out.copy_(acc)
            return
        assert out.is_contiguous() and out.numel() == M * N
        offs, second, s_used = self._plane_offsets(M, N, R, s)
        offs = offs + np.where(second, M * s_used, 0)[None, :]
        out.view(-1)[torch.from_numpy(offs.reshape(-1))] = acc.reshape(-1)

    def thin_dgrad(self, dY, W, dX, R=0, dY2=None, gate=None):
        M, K = dX.shape
        N = W.shape[0]
        assert dY.dtype == F32
        if R == 0:
            assert dY2 is None and tuple(dY.shape) == (M, N) and dY.stride(1) == 1
            s = N
            self._check_thin(dX, W, M, N, K, R, s)
            dy = _np32(dY)
        else:
            s = dY.numel() // M
            self._check_thin(dX, W, M, N, K, R, s)
            assert dY.is_contiguous() and dY.numel() == M * s and (dY2 is None) == (s == N)
            assert dY2 is None or (dY2.dtype == F32 and dY2.is_contiguous() and dY2.numel() == M * (N - s))
            offs, second, s_used = self._plane_offsets(M, N, R, s)
            p1 = _np32(dY).reshape(-1)
            p2 = _np32(dY2).reshape(-1) if dY2 is not None else np.zeros(1, np.float32)
            dy = np.zeros((M, N), np.float32)
            for n in range(N):
                src = p2 if second[n] else p1
                dy[:, n] = src[np.minimum(offs[:, n], src.size - 1)]
                if second[n] and "second_block_ignored" in self.flaws:
                    dy[:, n] = 0
        if "dy_not_rounded" not in self.flaws:
            dy = _np32(torch.from_numpy(dy).to(BF))
        acc = dy @ _np32(W)
        if gate is not None:
            assert gate.dtype == BF and tuple(gate.shape) == (M, K) and gate.stride(1) == 1 and (M == 1 or gate.stride(0) == dX.stride(0))
            g = _np32(gate)
            acc = np.where((g < 0) if "gate_lt" in self.flaws else (g <= 0), np.float32(0), acc)      # a NaN gate passes
        dX.copy_(torch.from_numpy(acc.astype(np.float32)).to(dX.dtype))


# ------------------------------------------------------------------------------------------------ the twins
class _GatedReLU(torch.autograd.Function):
    """relu(x) whose backward multiplies by a gate that is handed in (see `parity`)."""

    @staticmethod
    def forward(ctx, x, gate):
        ctx.save_for_backward(gate)
        return x.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _relu(x, gate):
    return F.relu(x) if gate is None else _GatedReLU.apply(x, gate.to(x.dtype))


class TwinConvModule(nn.Module):
    """mmcv ConvModule(cin, cout, 3, padding=1, norm_cfg=..., act_cfg=dict(type='ReLU')): conv -> bn -> ReLU."""

    def __init__(self, cin, cout, norm):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1, bias=not norm)
        if norm:
            self.bn = nn.BatchNorm2d(cout)
        self.gate = None                                              # a bool map: the ReLU's backward gate, handed in

    def forward(self, x):
        x = self.conv(x)
        return _relu(self.bn(x) if hasattr(self, "bn") else x, self.gate)


class TwinRPNHead(nn.Module):
    def __init__(self, in_channels, feat_channels, anchor_generator=None, num_convs=1, norm_cfg=None, **_):
        super().__init__()
        A = len(anchor_generator["scales"]) * len(anchor_generator["ratios"])
        if num_convs > 1:
            self.rpn_conv = nn.Sequential(*(TwinConvModule(in_channels if i == 0 else feat_channels, feat_channels, norm_cfg is not None)
                                            for i in range(num_convs)))
        else:
            self.rpn_conv = nn.Conv2d(in_channels, feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(feat_channels, A, 1)
        self.rpn_reg = nn.Conv2d(feat_channels, 4 * A, 1)

    def forward(self, feats):
        cls, reg = [], []
        last = self.rpn_conv[-1].gate if isinstance(self.rpn_conv, nn.Sequential) else None
        for x in feats:                                               # RPNHead.forward_single; a gate handed to the stack's last ReLU
            x = _relu(self.rpn_conv(x), last)                         # is this (forward-identical) ReLU's gate too
            cls.append(self.rpn_cls(x))
            reg.append(self.rpn_reg(x))
        return cls, reg


class TwinMaskHead(nn.Module):
    def __init__(self, num_convs=4, in_channels=256, conv_out_channels=256, num_classes=80, class_agnostic=False, norm_cfg=None, **_):
        super().__init__()
        self.convs = nn.ModuleList(TwinConvModule(in_channels if i == 0 else conv_out_channels, conv_out_channels, norm_cfg is not None)
                                   for i in range(num_convs))
        self.upsample = nn.ConvTranspose2d(conv_out_channels if num_convs else in_channels, conv_out_channels, 2, stride=2)
        self.conv_logits = nn.Conv2d(conv_out_channels, 1 if class_agnostic else num_classes, 1)
        self.gate = None                                              # the gate of the ReLU behind `upsample`, handed in

    def forward(self, x):
        for conv in self.convs:
            x = conv(x)
        return self.conv_logits(_relu(self.upsample(x), self.gate))


ANCHORS = dict(scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16])
KINDS = {
    # name -> (twin class, constructor arguments without norm_cfg, [input shapes])
    "rpn2": (TwinRPNHead, dict(in_channels=64, feat_channels=64, anchor_generator=ANCHORS, num_convs=2), [(2, 64, 8, 8), (2, 64, 4, 4), (2, 64, 2, 2)]),
    "rpn1": (TwinRPNHead, dict(in_channels=64, feat_channels=64, anchor_generator=ANCHORS, num_convs=1), [(2, 64, 5, 7), (1, 64, 3, 3)]),
    "mask": (TwinMaskHead, dict(num_convs=2, in_channels=64, conv_out_channels=64, num_classes=3, class_agnostic=True), [(5, 64, 14, 14)]),
    # the form with norm: one ConvModule, so that two bf16 operand roundings sit in series behind the exact input (the tail's X and the
    # activation), as many as in the cases of profiles/neck_parity.md and profiles/fpn_parity.md that justify the threshold
    "mask1": (TwinMaskHead, dict(num_convs=1, in_channels=64, conv_out_channels=64, num_classes=3, class_agnostic=True), [(5, 64, 14, 14)]),
}


def call(m, ins):
    """The module's outputs as one flat list: an RPN head's cls_scores + bbox_preds, a mask head's logits."""
    out = m(ins) if isinstance(m, TwinRPNHead) or type(m).__name__ == "RPNHead" else m(ins[0])
    if isinstance(out, tuple):
        return list(out[0]) + list(out[1])
    return [out]


def make_twin(kind, norm_cfg=None):
    cls, kw, shapes = KINDS[kind]
    return cls(**kw, norm_cfg=norm_cfg), shapes


def make_module(kind, ops, fused=True, norm_cfg=None, **extra):
    from clipself_amd.mask_head import FCNMaskHead
    from clipself_amd.rpn_head import RPNHead
    cls, kw, _ = KINDS[kind]
    return (RPNHead if cls is TwinRPNHead else FCNMaskHead)(**kw, norm_cfg=norm_cfg, ops=ops, fused=fused, **extra)


# ------------------------------------------------------------------------------------------------ exact operands
def _watch(twin):
    """Forward hooks that keep every leaf layer's output (with its gradient): the tensors the kernel route rounds to bf16 operands."""
    seen = []

    def hook(mod, inp, out):
        if out.requires_grad:
            out.retain_grad()
        seen.append((type(mod).__name__, out))
    hs = [m.register_forward_hook(hook) for m in twin.modules() if not list(m.children())]
    return seen, hs


@functools.lru_cache(maxsize=None)
def exact_case(kind, seed=0):
    """(twin in float64 with its gradients, inputs, upstream gradients, outputs, input gradients), computed once and shared read-only."""
    twin, shapes = make_twin(kind)
    twin = twin.double()
    g = torch.Generator().manual_seed(4000 + seed + len(kind))
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if p.dim() == 4 and p.shape[-1] == 3:
                p.copy_(_sparse_int(g, p.shape, -1, 1, 1 / 48))
            elif p.dim() == 4:
                p.copy_(_sparse_int(g, p.shape, -1, 1, 1 / 8))
            else:
                p.copy_(_sparse_int(g, p.shape, -2, 2, 1 / 2))
    xs = [_sparse_int(g, s, -2, 2, 1 / 4) for s in shapes]
    ins = [x.double().requires_grad_(True) for x in xs]
    seen, hs = _watch(twin)
    outs = call(twin, ins)
    gs = [_sparse_int(g, o.shape, -2, 2, 1 / 8) for o in outs]
    torch.autograd.backward(outs, [t.double() for t in gs])
    for h in hs:
        h.remove()
    assert_exact(kind, twin, ins, gs, outs, seen)
    return twin, xs, gs, [o.detach() for o in outs], [t.grad for t in ins]


def assert_exact(kind, twin, ins, gs, outs, seen):
    def ints(t, what, limit):
        if not (torch.equal(t, t.round()) and float(t.abs().max()) <= limit):
            raise ExactnessError(f"{what}: max |v| {float(t.abs().max())} (limit {limit}) or a non-integer: the case, not a kernel, is wrong")
    finals = {id(o) for o in outs}
    for name, t in seen:
        ints(t.detach(), f"output of a {name}", TWO24 - 1 if id(t) in finals else 256)
        if t.grad is not None:
            ints(t.grad, f"gradient at the output of a {name}", 256)
    for t in list(gs) + [t.detach() for t in ins]:
        ints(t, "an input or upstream gradient", 256)
    for t in [o.detach() for o in outs] + [t.grad for t in ins] + [p.grad for p in twin.parameters()]:
        ints(t, "a result", TWO24 - 1)
    mag, _ = make_twin(kind)                                              # sums of |terms|: the same graph on absolute values
    mag = mag.double()
    mag.load_state_dict({k: v.abs() for k, v in twin.state_dict().items()})
    ains = [t.detach().abs().requires_grad_(True) for t in ins]
    aouts = call(mag, ains)
    torch.autograd.backward(aouts, [t.double().abs() for t in gs])
    worst = max(float(t.max()) for t in [o.detach() for o in aouts] + [t.grad for t in ains] + [p.grad for p in mag.parameters()])
    if not worst < TWO24:
        raise ExactnessError(f"a sum of |terms| reaches {worst} >= 2^24: fp32 accumulation is not exact for this case")


def run_module(m, xs, gs, dtype=F32, device="cpu", channels_last=False):
    """One forward + backward -> (outs, input gradients, {parameter name: gradient})."""
    m.zero_grad()
    ins = []
    for x in xs:
        t = x.detach().to(device).to(dtype).clone()
        if channels_last:
            t = t.contiguous(memory_format=torch.channels_last)
        ins.append(t.requires_grad_(True))
    outs = call(m, ins)
    torch.autograd.backward(outs, [t.to(device).to(o.dtype) for t, o in zip(gs, outs)])
    return [o.detach() for o in outs], [t.grad for t in ins], {n: p.grad for n, p in m.named_parameters()}


def check_exact(kind, ops, device="cpu", **extra):
    """The module on `ops` against the float64 twin on the exact case: outputs, input gradients and parameter gradients bit for bit."""
    twin, xs, gs, outs, dxs = exact_case(kind)
    m = copy_state(make_module(kind, ops, **extra), twin).to(device)
    got_outs, got_dx, got_dp = run_module(m, xs, gs, device=device)
    assert len(got_outs) == len(outs)
    for i, (a, b) in enumerate(zip(got_outs, outs)):
        assert a.dtype == F32
        same_bits(a, b, f"{kind}: output {i}")
    for i, (a, b) in enumerate(zip(got_dx, dxs)):
        same_bits(a, b, f"{kind}: gradient of input {i}")
    want = {k: p.grad for k, p in twin.named_parameters()}
    assert sorted(got_dp) == sorted(want)
    for k in want:
        same_bits(got_dp[k], want[k], f"{kind}: gradient of {k}")
    return got_outs


# ------------------------------------------------------------------------------------------------ random operands, with norm
@functools.lru_cache(maxsize=None)
def random_case(kind, seed=11):
    """The fp32 twin with norm in training mode and its results on operands bf16 holds exactly."""
    torch.manual_seed(seed)
    twin, shapes = make_twin(kind, norm_cfg=dict(type="BN"))
    twin.train()
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(BF).to(F32)
    with torch.no_grad():
        for m in twin.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                m.weight.copy_(bf(m.weight))
    state = {k: v.clone() for k, v in twin.state_dict().items()}
    xs = [bf(torch.randn(s, generator=g)) for s in shapes]
    with torch.no_grad():
        shapes_out = [o.shape for o in call(twin, xs)]
    twin.load_state_dict(state)
    gs = [bf(torch.randn(s, generator=g)) for s in shapes_out]
    outs, dx, dp = run_module(twin, xs, gs)
    return state, xs, gs, outs, dx, dp


def _module_gates(m, ins):
    """One forward of the module under test -> the gates of its ReLUs, in the twin's order: a ConvModule's output > 0, and for a mask head
    the gate of the ReLU behind `upsample`, recomputed in float64 from the map that enters the tail rounded to bf16 and the bf16 weights
    (what the kernel route contracts; its fp32 accumulation moves a pre-activation by 1e-7 of its scale, the bf16 operands the twin does
    not have by 1e-3)."""
    from clipself_amd.norm_act import ConvModule
    seen = []
    hs = [c.register_forward_hook(lambda mod, inp, out: seen.append(out.detach())) for c in m.modules() if isinstance(c, ConvModule)]
    with torch.no_grad():
        call(m, ins)
    for h in hs:
        h.remove()
    gates = [(t > 0).cpu() for t in seen]
    tail = None
    if hasattr(m, "upsample"):
        up = m.upsample
        pre = F.conv_transpose2d(seen[-1].to(BF).double().cpu(), up.weight.detach().to(BF).double().cpu(), up.bias.detach().double().cpu(), stride=2)
        tail = pre > 0
    return gates, tail


def parity(kind, ops, device="cpu", tag="CPU backend"):
    """Worst rel-L2 of the module with norm against the fp32 twin on random operands: (outputs, input gradients, parameter gradients);
    every figure is printed.  The outputs are compared with the plain twin.  A ReLU's gradient is discontinuous: a pre-activation that
    the route's bf16 operand roundings move across zero (about one element in a thousand) flips a gate, and two correct backward passes
    then differ by 2e-2 to 7e-2 in L2.  So the gradients are compared with the twin whose ReLU GATES are the module's own (as
    profiles/fc_parity.md does for Linear + ReLU); the gates themselves are pinned bit for bit by the exact cases."""
    state, xs, gs, outs, _, _ = random_case(kind)
    m = make_module(kind, ops, norm_cfg=dict(type="BN")).train()
    m.load_state_dict(state, strict=True)
    m = m.to(device)
    gates, tail = _module_gates(m, [x.to(device) for x in xs])
    m.load_state_dict(state, strict=True)                                # the running statistics back to where they were
    got_outs, got_dx, got_dp = run_module(m, xs, gs, device=device)
    twin, _ = make_twin(kind, norm_cfg=dict(type="BN"))
    twin.train().load_state_dict(state, strict=True)
    mods = [c for c in twin.modules() if isinstance(c, TwinConvModule)]
    n = len(mods)
    assert len(gates) % n == 0                                           # an RPN head runs its stack once per level
    twin.gate = tail
    dx, dp = [], None
    if isinstance(twin, TwinRPNHead):                                    # level by level: each level has its own gates
        twin.zero_grad()
        L = len(xs)
        for i, x in enumerate(xs):
            for j, c in enumerate(mods):
                c.gate = gates[i * n + j]
            t = x.clone().requires_grad_(True)
            cls, reg = twin([t])
            torch.autograd.backward([cls[0], reg[0]], [gs[i], gs[L + i]])
            dx.append(t.grad)
        dp = {k: p.grad for k, p in twin.named_parameters()}
    else:
        for c, g in zip(mods, gates):
            c.gate = g
        _, dx, dp = run_module(twin, xs, gs)
    worst_out = worst_dx = worst_grad = 0.0
    for i, (a, b) in enumerate(zip(got_outs, outs)):
        r = rel_l2(a, b)
        worst_out = max(worst_out, r)
        print(f"THIN PARITY [{tag}] {kind} output {i} rel-L2 {r:.4e}")
    for i, (a, b) in enumerate(zip(got_dx, dx)):
        r = rel_l2(a, b)
        worst_dx = max(worst_dx, r)
        print(f"THIN PARITY [{tag}] {kind} input gradient {i} rel-L2 {r:.4e} (gates handed in)")
    assert sorted(got_dp) == sorted(dp)
    for layer in sorted({k.rsplit(".", 1)[0] for k in dp}):             # a layer's weight and bias gradients as one vector
        ks = [k for k in dp if k.rsplit(".", 1)[0] == layer]
        a = torch.cat([got_dp[k].detach().double().cpu().reshape(-1) for k in ks])
        b = torch.cat([dp[k].detach().double().reshape(-1) for k in ks])
        r = float((a - b).norm() / b.norm().clamp_min(1e-300))
        worst_grad = max(worst_grad, r)
        print(f"THIN PARITY [{tag}] {kind} grad {layer}.* rel-L2 {r:.4e} (gates handed in)")
    return worst_out, worst_dx, worst_grad


# ------------------------------------------------------------------------------------------------ Conv1x1Thin / thin_heads alone
# (M rows, Cin, Cout) -> (B, H, W) with B*H*W == M.  M = 105 is no multiple of 16 and R = 35 no multiple of 4; one pixel; two K tiles
# and N = 16; five K tiles (K % 256 != 0) with R % 4 == 0
LAYER_SHAPES = {(105, 64, 15): (3, 5, 7), (1, 64, 1): (1, 1, 1), (32, 256, 16): (2, 4, 4), (256, 320, 12): (2, 16, 8), (105, 256, 3): (3, 5, 7)}
LAYOUTS = [("nchw", F32), ("channel_last", F32), ("channel_last", BF)]


def thin_layers(ops, weight, bias, widths, device="cpu", fused=True):
    from clipself_amd.conv import Conv1x1Thin
    mods, c0 = [], 0
    for n in widths:
        m = Conv1x1Thin(weight.shape[1], n, ops=ops, fused=fused)
        with torch.no_grad():
            m.weight.copy_(weight[c0:c0 + n].view_as(m.weight))
            m.bias.copy_(bias[c0:c0 + n])
        mods.append(m.to(device))
        c0 += n
    return mods


def run_thin(mods, x, dy, geom, layout, dtype):
    """x [M, Cin], dy [M, sum N] rows -> (y rows [M, sum N], dx rows, dw [sum N, Cin], db [sum N]) of one forward + backward through
    thin_heads (two modules) or the module itself (one)."""
    from clipself_amd.conv import thin_heads
    B, H, W = geom
    dev = mods[0].weight.device
    for m in mods:
        m.zero_grad()
    inp = x.to(dev).to(dtype).view(B, H, W, -1).permute(0, 3, 1, 2)
    if layout == "nchw":
        inp = inp.contiguous()
    inp = inp.detach().requires_grad_(True)
    ys = thin_heads(inp, mods) if len(mods) > 1 else (mods[0](inp),)
    gs, c0 = [], 0
    for y, m in zip(ys, mods):
        assert y.dtype == F32 and y.is_contiguous() and tuple(y.shape) == (B, m.out_channels, H, W) and "Thin" in type(y.grad_fn).__name__
        gs.append(dy[:, c0:c0 + m.out_channels].to(dev).view(B, H, W, -1).permute(0, 3, 1, 2).contiguous())
        c0 += m.out_channels
    torch.autograd.backward(ys, gs)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    assert inp.grad.dtype == dtype
    return (torch.cat([rows(y.detach()) for y in ys], 1), rows(inp.grad), torch.cat([m.weight.grad.view(m.out_channels, -1) for m in mods]),
            torch.cat([m.bias.grad for m in mods]))


def check_thin(ops, shape, layout, dtype, kind, widths=None, device="cpu"):
    x, w, b, dy, ref = _fc_ref.case(shape, kind, act=None)
    M, Cin, Cout = shape
    mods = thin_layers(ops, w, b, widths or [Cout], device)
    y, dx, dw, db = run_thin(mods, x, dy, LAYER_SHAPES[shape], layout, dtype)
    assert dx.dtype == dtype and dw.dtype == F32 and db.dtype == F32
    if kind == "exact":
        for got, key in ((y, "y"), (dx, "dx"), (dw, "dw"), (db, "db")):
            same_bits(got, ref[key], f"{shape} {layout} {dtype} {widths}: {key}")
        return
    _fc_ref.check_bound("y", y, ref["y"], _fc_ref.bound(ref["ay"], Cin, 1))
    _fc_ref.check_bound("dx", dx, ref["dx"], _fc_ref.bound(ref["adx"], Cout, 1, ref["dx"], dtype == BF))
    _fc_ref.check_bound("dw", dw, ref["dw"], _fc_ref.bound(ref["adw"], M))
    _fc_ref.check_bound("db", db, ref["db"], _fc_ref.bound(ref["adb"], M))


def check_dy_rounding(ops, device="cpu"):
    """The input gradient rounds dY to bf16: an upstream gradient of integers that bf16 does NOT hold (257, 1027, ...) must give the
    float64 result of its round-to-nearest-even image, bit for bit (all operands stay integers, every sum below 2^24)."""
    shape = (105, 64, 15)
    x, w, b, _, _ = _fc_ref.case(shape, "exact", act=None)
    g = torch.Generator().manual_seed(99)
    dy = (torch.randint(0, 2, (105, 15), generator=g) * 2 - 1).to(F32) * torch.tensor([257.0, 1027.0, 515.0, 3.0, 2049.0])[torch.randint(0, 5, (105, 15), generator=g)]
    assert not torch.equal(dy.to(BF).to(F32), dy)
    want = (dy.to(BF).double() @ w.double())
    assert float((dy.to(BF).double().abs() @ w.double().abs()).max()) < TWO24
    mods = thin_layers(ops, w, b, [3, 12], device)
    _, dx, _, _ = run_thin(mods, x, dy, LAYER_SHAPES[shape], "channel_last", F32)
    same_bits(dx, want, "dx of a gradient that bf16 does not hold")
