"""TEST INFRASTRUCTURE -- the box head's Linear (+ ReLU) layers as split-K GEMMs (clipself_amd/linear.py, clipself_amd/bbox_head.py, the
cs_gemm_nt block of include/clipself_hip.h).

* `RefOpsFC`: the CPU backend of the other detector layers (tests/_bn_ref.RefOpsBN, a subclass of the unchanged oracle.ops_ref.RefOps)
  plus `gemm_nt` restated from the header's text for epilogue 9 and for `splits` on epilogues 0 / 9: contiguous slices of
  ceil(K/64/splits) K tiles, fp32 partials [splits, M, N] in `extra`, added in ascending order, the bias once, v < 0 ? 0 : v, one
  rounding to bf16 -- and the header's rejections.  `flaws=("bias_per_slice",)` plants an error the checks must reject.
* The reference is torch's own layer: F.linear (+ F.relu) under autograd in float64, on x.flatten(1) for the `spatial` form.  With
  `mask` the ReLU's gate is handed in (the device's own saved Y > 0), so that a pre-activation next to zero cannot make two correct
  backward passes differ.
* Bounds, the derivation of tests/_neck_ref.bound: an fp32 accumulation of K exact bf16 x bf16 products summed in S slices, plus the
  bias, is K + S + 1 roundings at the most, each at most 2^-24 of the running sum, which sum|terms| bounds; the factor 2 covers the
  second-order terms:  2 * (K + S + 1) * 2^-24 * sum|terms|.  A bf16 output adds 2^-8 * (|reference| + bound).  ReLU is 1-Lipschitz and
  adds nothing.  K = in_features for y, out_features for dx, rows for dw and db (S = 1 for the gradients: any summation order of K terms
  is inside the bound).  Derived, not measured.
* Exact operands are integers in [-8, 8]: every sum of |terms| is asserted below 2^24, so fp32 accumulation in any order and in any
  number of slices is exact, fp32 results equal the float64 ones bit for bit and bf16 results their round-to-nearest-even image."""
import functools

import torch
import torch.nn.functional as F

from _bn_ref import RefOpsBN
from _neck_ref import BF, F32, TWO24, U, ExactnessError, check_bound, rne_bf16  # noqa: F401

EPI_BF16, EPI_F32, EPI_ATOMIC_F32, EPI_RELU_BF16 = 0, 1, 4, 9
REF_CUS = 256                                   # the CU count the CPU backend states the automatic rule with (MI355X)


# ------------------------------------------------------------------------------------------------ the op, from the header's text
def auto_splits(M, N, K, cus=REF_CUS):
    """clipself_hip.h: s = 1; while (s < 8 && ceil(M/256) * ceil(N/256) * 2s <= compute units && (K/64) / (2s) >= 16) s *= 2."""
    tiles = -(-M // 256) * -(-N // 256)
    s = 1
    while s < 8 and tiles * 2 * s <= cus and (K // 64) // (2 * s) >= 16:
        s *= 2
    return s


class RefOpsFC(RefOpsBN):
    name = "ref+taps+neck+conv+bn+fc"
    LINEAR_ACT = True
    flaws = ()

    def gemm_nt_splits(self, M, N, K):
        return auto_splits(M, N, K)

    def gemm_nt(self, A, B, C, bias=None, extra=None, epi=EPI_BF16, splits=1, group=0, flags=0):
        if epi not in (EPI_BF16, EPI_RELU_BF16):
            if splits != 1 and epi != EPI_ATOMIC_F32:
                raise RuntimeError(f"cs_gemm_nt: split-K exists for epilogues 0, 9 and 4, not {epi}")
            return super().gemm_nt(A, B, C, bias, extra, epi=epi, splits=splits, group=group, flags=flags)
        M, K = A.shape
        N = B.shape[0]
        assert K % 64 == 0 and N % 4 == 0 and A.dtype == BF and B.dtype == BF and C.dtype == BF and tuple(C.shape) == (M, N)
        kt = K // 64
        s = splits if splits > 0 else self.gemm_nt_splits(M, N, K)
        if s > kt:
            raise RuntimeError(f"cs_gemm_nt: splits={s} exceeds the {kt} K tiles")
        if s > 1:
            if extra is None or extra.dtype != F32 or extra.data_ptr() % 16 or extra.numel() < s * M * N:
                raise RuntimeError("cs_gemm_nt: split-K needs a 16-byte aligned fp32 workspace of splits*M*N floats in `extra`")
            ws = extra.reshape(-1)[:s * M * N].view(s, M, N)
            per = -(-kt // s)
            for y in range(s):
                k0, k1 = y * per * 64, min((y + 1) * per, kt) * 64
                ws[y] = A[:, k0:k1].float() @ B[:, k0:k1].float().T if k1 > k0 else 0.0
            acc = ws[0].clone()
            for y in range(1, s):
                acc += ws[y]
        else:
            acc = A.float() @ B.float().T
        if bias is not None:
            acc = acc + (bias * s if "bias_per_slice" in self.flaws else bias)
        if epi == EPI_RELU_BF16:
            acc = torch.where(acc < 0, torch.zeros(()), acc)
        C.copy_(acc.to(BF))


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_operands(rows, inf, out, seed):
    """x [rows, in], weight [out, in], bias [out], dy [rows, out]: fp32 values that bf16 holds exactly, weights at Xavier's scale."""
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).to(F32)
    return r(rows, inf), (r(out, inf) * inf ** -0.5).to(BF).to(F32), r(out), r(rows, out)


def exact_operands(rows, inf, out, seed):
    g = _gen(seed)
    r = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)
    return r(rows, inf), r(out, inf), r(out), r(rows, out)


# ------------------------------------------------------------------------------------------------ references
def reference(x, weight, bias, dy, act="relu", mask=None):
    """float64 F.linear (+ F.relu) under autograd -> dict(y, dx, dw, db) and the per-element sums of |terms| (ay, adx, adw, adb).
    x [rows, in] (the flattened input).  mask [rows, out] bool: the gate of the ReLU's backward, handed in instead of taken from the
    float64 pre-activation."""
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, weight, bias))
    pre = F.linear(x64, w64, b64)
    y = F.relu(pre) if act == "relu" else pre
    if act == "relu" and mask is not None:
        dz = dy.double() * mask.double()
        pre.backward(dz)
    else:
        y.backward(dy.double())
        dz = dy.double() * (pre.detach() > 0).double() if act == "relu" else dy.double()
    with torch.no_grad():
        ax, aw, adz = x.double().abs(), weight.double().abs(), dz.abs()
        out = dict(y=y.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad, dz=dz,
                   ay=ax @ aw.T + bias.double().abs(), adx=adz @ aw, adw=adz.T @ ax, adb=adz.sum(0))
    return out


def assert_exact(ref):
    """The sums of |terms| of an exact case stay below 2^24 and the results are integers fp32 holds (else the case, not a kernel, is wrong)."""
    for k in ("ay", "adx", "adw", "adb"):
        if not float(ref[k].max()) < TWO24:
            raise ExactnessError(f"{k}: sum of |terms| {float(ref[k].max())} reaches 2^24: fp32 accumulation is not exact for this case")
    for k in ("y", "dx", "dw", "db"):
        assert torch.equal(ref[k], ref[k].round()) and torch.equal(ref[k].to(F32).double(), ref[k])
    return ref


@functools.lru_cache(maxsize=None)
def case(shape, kind, act="relu", seed=0):
    """(x, weight, bias, dy, reference) of (rows, in, out), computed once and shared (read-only) by the tests that need it."""
    rows, inf, out = shape
    ops = (exact_operands if kind == "exact" else random_operands)(rows, inf, out, seed + rows + inf + out)
    ref = reference(*ops, act=act)
    return ops + (assert_exact(ref) if kind == "exact" else ref,)


def bound(abs_terms, K, S=1, reference_value=None, bf16_out=False):
    """2 * (K + S + 1) * 2^-24 * sum|terms|  (+ 2^-8 * (|reference| + bound) for a bf16 output)."""
    b = 2.0 * (K + S + 1) * U * abs_terms
    if bf16_out:
        b = b + 2.0 ** -8 * (reference_value.abs() + b)
    return b


def bounds(ref, shape, splits=1, bf16_dx=False):
    """Per-element bounds of y (always a bf16 value), dx (x's dtype), dw, db (fp32) for (rows, in, out)."""
    rows, inf, out = shape
    return dict(y=bound(ref["ay"], inf, splits, ref["y"], True), dx=bound(ref["adx"], out, 1, ref["dx"], bf16_dx),
                dw=bound(ref["adw"], rows), db=bound(ref["adb"], rows))


def same_bits(got, want, what):
    it = {BF: torch.int16, F32: torch.int32}[got.dtype]
    assert want.dtype == got.dtype and tuple(want.shape) == tuple(got.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().contiguous().view(it), want.contiguous().view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ the layer
def to_map(x, C, h, w):
    """x [rows, C*h*w] in nn.Linear's (c, p) order -> the map [rows, C, h, w] whose flatten(1) it is."""
    return x.view(x.shape[0], C, h, w)


def layer(ops, weight, bias, device="cpu", **kw):
    from clipself_amd.linear import LinearAct
    m = LinearAct(weight.shape[1], weight.shape[0], ops=ops, **kw)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    return m.to(device)


def run_layer(m, x, dy, dtype=F32, geom=None, channel_last=True):
    """One forward + backward of the layer on x [rows, in] (cast to `dtype`; with geom=(C, h, w) handed in as the map, channel-last or
    NCHW-contiguous) -> (y, dx [rows, in] in (c, p) order, dw, db)."""
    dev = m.weight.device
    m.zero_grad()
    inp = x.detach().to(dev).to(dtype).clone()
    if geom is not None:
        inp = to_map(inp, *geom)
        if channel_last:
            inp = inp.contiguous(memory_format=torch.channels_last)
    inp.requires_grad_(True)
    y = m(inp)
    y.backward(dy.to(dev).to(y.dtype))
    return y.detach(), inp.grad.reshape(x.shape), m.weight.grad, m.bias.grad
