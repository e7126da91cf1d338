"""TEST INFRASTRUCTURE -- the detector heads' 3 x 3 convolutions as implicit GEMMs (clipself_amd/conv.py, include/clipself_conv.h).

* `RefOpsConv`: tests/_neck_ref.RefOpsNeck plus conv3x3 / im2col3x3 as torch index expressions written from the header's definition, and
  the CONV3X3 flag -- the CPU backend Conv3x3's kernel route and its autograd function run on without a GPU.
* `index_im2col` / `index_conv3x3`: those expressions; `flaws=` plants one error in a copy (what the checks must reject).
* Seeded operand generators: random (bf16-representable) and exact (integers in [-8, 8]).
* The float64 reference (F.conv2d(padding=1) under autograd) and the bounds, the derivation of tests/_neck_ref.bound:

  exact operands -- with |x|, |w|, |b|, |dy| <= 8 integers a forward sum is at most 64 * 9*Cin + 8, an input-gradient sum 64 * 9*Cout and a
  weight- or bias-gradient sum 64 * N*H*W (8 * N*H*W): `exact_reference` asserts that each stays below 2^24 (the largest case gives
  64 * 9 * 192 + 8 = 110 600), so fp32 accumulation in any order is exact and fp32 results must equal the float64 ones bit for bit, bf16
  outputs their round-to-nearest-even image.

  random operands -- fp32 accumulation of K exact bf16 x bf16 products in any order: `2 * K * 2^-24 * sum|terms|` with K = 9*Cin + 1 for y
  (the bias is one more term), K = 9*Cout for dx, K = N*H*W for dw and db; a bf16 output adds 2^-8 * (|reference| + bound).  Derived,
  not measured."""
import functools

import torch
import torch.nn.functional as F

from _neck_ref import BF, F32, F64, TWO24, ExactnessError, RefOpsNeck, bound, check_bound, rne_bf16  # noqa: F401

# (N, H, W, Cin, Cout): eight of nine taps out of range, one K tile per tap, the smallest N | non-square, an H / W swap shows | 147 rows:
# images straddle an M tile, three K tiles per tap, a partial N tile | 294 rows, three M tiles, dgrad on the implicit route | the mask
# head's tile, Cout % 64 != 0: dgrad takes the im2col route | a map rather than tiles, a full N tile
SHAPES = [(1, 1, 1, 64, 8), (2, 3, 5, 64, 16), (3, 7, 7, 192, 48), (6, 7, 7, 64, 64), (2, 14, 14, 128, 72), (1, 33, 17, 64, 256)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
ROUTES = ("implicit", "im2col")


# ------------------------------------------------------------------------------------------------ the ops, from the header's definition
def index_im2col(x, N, H, W, row0, rows, flaws=()):
    """cols[r, t*C + c] = x[(row0 + r) shifted by tap t, c], t = ky*3 + kx reading pixel (y + ky - 1, x + kx - 1) of the same image, zero
    outside it.  x [N*H*W, >= C] rows.  flaws: 'swap' (ky / kx exchanged), 'no_x' (no x-range check: a tap wraps to the neighbouring
    row), 'no_image' (no y-range check inside the image: a tap bleeds into image n +- 1)."""
    M, C = N * H * W, x.shape[1]
    p = torch.arange(row0, row0 + rows)
    pix = p % (H * W)
    y, xx = pix // W, pix % W
    cols = torch.zeros(rows, 9 * C, dtype=x.dtype)
    for t in range(9):
        ky, kx = t // 3, t % 3
        if "swap" in flaws:
            ky, kx = kx, ky
        yy, xs = y + ky - 1, xx + kx - 1
        src = p + (ky - 1) * W + (kx - 1)
        ok_x = (xs >= 0) & (xs < W)
        ok_y = (yy >= 0) & (yy < H)
        if "no_x" in flaws:
            ok_x = torch.ones_like(ok_x)
        if "no_image" in flaws:
            ok_y = torch.ones_like(ok_y)
        ok = ok_x & ok_y & (src >= 0) & (src < M)                       # the map's own extent holds in every copy
        cols[:, t * C:(t + 1) * C] = torch.where(ok[:, None], x[src.clamp(0, M - 1)], torch.zeros((), dtype=x.dtype))
    return cols


def index_conv3x3(x, Wg, bias, N, H, W, dtype, flaws=()):
    """y[p, co] = bias[co] + sum_{t, ci} x[p shifted by t, ci] * Wg[co, t*Cin + ci]: fp32 accumulation, one rounding at `dtype`."""
    acc = index_im2col(x, N, H, W, 0, N * H * W, flaws).float() @ Wg.float().T
    if bias is not None:
        acc = acc + bias
    return acc.to(dtype)


class RefOpsConv(RefOpsNeck):
    name = "ref+taps+neck+conv"
    CONV3X3 = True
    flaws = ()

    def conv3x3(self, x, Wg, y, bias, N, H, W):
        Cin, Cout = x.shape[1], Wg.shape[0]
        assert x.dtype == BF and Wg.dtype == BF and tuple(x.shape) == (N * H * W, Cin) and tuple(Wg.shape) == (Cout, 9 * Cin)
        assert Cin % 64 == 0 and Cout % 8 == 0 and tuple(y.shape) == (N * H * W, Cout) and y.dtype in (F32, BF)
        y.copy_(index_conv3x3(x, Wg, bias, N, H, W, y.dtype, self.flaws))

    def im2col3x3(self, x, cols, N, H, W, row0=0):
        Cin = x.shape[1]
        assert x.dtype == BF and cols.dtype == BF and tuple(x.shape) == (N * H * W, Cin) and cols.shape[1] == 9 * Cin and Cin % 8 == 0
        assert 0 <= row0 and row0 + cols.shape[0] <= N * H * W
        cols.copy_(index_im2col(x, N, H, W, row0, cols.shape[0], self.flaws))


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_operands(N, H, W, Cin, Cout, seed):
    """x [N, Cin, H, W], weight [Cout, Cin, 3, 3], bias [Cout], dy [N, Cout, H, W]: fp32 values that bf16 holds exactly."""
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).to(F32)
    return r(N, Cin, H, W), (r(Cout, Cin, 3, 3) * (9 * Cin) ** -0.5).to(BF).to(F32), r(Cout), r(N, Cout, H, W)


def exact_operands(N, H, W, Cin, Cout, seed):
    """The same four tensors holding integers in [-8, 8]."""
    g = _gen(seed)
    r = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)
    return r(N, Cin, H, W), r(Cout, Cin, 3, 3), r(Cout), r(N, Cout, H, W)


def rows_of(t, dtype=BF):
    """[N, C, H, W] -> the channel-last rows [N*H*W, C]."""
    N, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(N * H * W, C).to(dtype).contiguous()


def map_of(rows, N, H, W):
    """The inverse: rows [N*H*W, C] -> [N, C, H, W]."""
    return rows.reshape(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ references
def reference(x, weight, bias, dy):
    """float64 F.conv2d(padding=1) under autograd -> dict(y, dx, dw, db) and the per-element sums of |terms| (ay, adx, adw, adb): the same
    graph on the operands' absolute values."""
    out = {}
    for tag, f in (("", lambda t: t.double()), ("a", lambda t: t.double().abs())):
        x64, w64, b64 = (f(t).requires_grad_(True) for t in (x, weight, bias))
        y = F.conv2d(x64, w64, b64, padding=1)
        y.backward(f(dy))
        out.update({tag + "y": y.detach(), tag + "dx": x64.grad, tag + "dw": w64.grad, tag + "db": b64.grad})
    return out


def exact_reference(x, weight, bias, dy):
    """reference() on exact operands; asserts that every sum of |terms| stays below 2^24 (else the case, not a kernel, is wrong)."""
    ref = reference(x, weight, bias, dy)
    for k in ("ay", "adx", "adw", "adb"):
        if not float(ref[k].max()) < TWO24:
            raise ExactnessError(f"{k}: sum of |terms| {float(ref[k].max())} reaches 2^24: fp32 accumulation is not exact for this case")
    for k in ("y", "dx", "dw", "db"):
        assert torch.equal(ref[k], ref[k].round()) and torch.equal(ref[k].to(F32).double(), ref[k])
    return ref


@functools.lru_cache(maxsize=None)
def case(shape, kind, seed=0):
    """(x, weight, bias, dy, reference) of a shape, computed once and shared (read-only) by the tests that need it."""
    N, H, W, Cin, Cout = shape
    ops = (exact_operands if kind == "exact" else random_operands)(N, H, W, Cin, Cout, seed + Cin + Cout + H)
    return ops + ((exact_reference if kind == "exact" else reference)(*ops),)


def bounds(ref, shape, bf16_out=False):
    """The per-element bounds of y, dx, dw, db for a shape; bf16_out widens y and dx (the outputs that take the input's dtype)."""
    N, H, W, Cin, Cout = shape
    return dict(y=bound(ref["ay"], 9 * Cin + 1, ref["y"], bf16_out), dx=bound(ref["adx"], 9 * Cout, ref["dx"], bf16_out),
                dw=bound(ref["adw"], N * H * W), db=bound(ref["adb"], N * H * W))


def same_bits(got, want, what):
    it = {BF: torch.int16, F32: torch.int32}[got.dtype]
    assert want.dtype == got.dtype and tuple(want.shape) == tuple(got.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().contiguous().view(it), want.contiguous().view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


def layer(ops, weight, bias, device="cpu", **kw):
    from clipself_amd.conv import Conv3x3
    m = Conv3x3(weight.shape[1], weight.shape[0], ops=ops, **kw)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    return m.to(device)


def run_layer(m, x, dy, dtype=F32, channel_last=True):
    """One forward + backward of the layer on x (cast to `dtype`, channel-last or NCHW-contiguous) -> (y, dx, dw, db)."""
    dev = m.weight.device
    m.zero_grad()
    inp = x.detach().to(dev).to(dtype).clone()            # the shared operands stay as they are
    if channel_last:
        inp = inp.contiguous(memory_format=torch.channels_last)
    inp.requires_grad_(True)
    y = m(inp)
    y.backward(dy.to(dev).to(y.dtype))
    return y.detach(), inp.grad, m.weight.grad, m.bias.grad
