"""TEST INFRASTRUCTURE -- the detector neck's 2x2 transposed convolutions as GEMMs on token rows (clipself_amd/neck.py).

* `RefOpsNeck`: tests/_backbone_ref.RefOpsBackbone plus rows_to_nchw / nchw_to_rows (forms 4 / 5 of cs_transpose_bf16) as torch indexing
  expressions, and the DECONV_ROWS flag -- the CPU backend Deconv2x2's GEMM path runs on without a GPU.
* `index_rows_to_nchw` / `index_nchw_to_rows`: the same two maps written element by element from the definition in
  include/clipself_hip.h; what the kernels are compared with bit for bit.
* Seeded operand generators: random (bf16-representable) and exact (integers in [-8, 8]).
* The float64 reference (F.conv_transpose2d under autograd) and the bounds:

  exact operands -- with |x|, |w|, |b|, |dy| <= 8 integers a forward sum is at most 64*Cin + 8, an input-gradient sum 64 * 4*Cout and a
  weight-gradient sum 64 * tokens: `exact_reference` asserts that each stays below 2^24, so fp32 accumulation in any order is exact and
  the fp32 results must equal the float64 ones bit for bit, bf16 outputs their round-to-nearest-even image.

  random operands -- fp32 accumulation of K exact bf16 x bf16 products in any order errs by at most (K - 1) * u * sum|terms| to first
  order, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, §3.1; K + 1 terms with the bias); `2 * K * 2^-24 *
  sum|terms|` covers the higher orders and the bias.  A bf16 output adds half an ulp of the rounded value v: ulp = 2^(e-7) for |v| in
  [2^e, 2^(e+1)), so half of it is at most 2^-8 * |v| <= 2^-8 * (|reference| + accumulation bound).  The bias gradient sums the
  bf16-rounded dY in fp32 over `tokens` terms per position, then four positions: K = 4 * tokens.  Derived, not measured."""
import torch
import torch.nn.functional as F

from _backbone_ref import RefOpsBackbone

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TWO24 = float(1 << 24)
U = 2.0 ** -24

# (B, h, w, C): smallest | ragged, non-square (an h / w swap shows) | the miniature | unaligned C, scalar tail | a full 64-token tile,
# 16-byte accesses both ways | several images, a channel tile and a fragment
KERNEL_SHAPES = [(1, 1, 1, 2), (2, 3, 5, 24), (2, 6, 6, 128), (1, 9, 7, 100), (1, 16, 16, 64), (3, 8, 8, 72)]
# (Cin, Cout, h, w) of the exact-operand cases, B = 2: one and three K tiles of the forward GEMM, 64 and 192 output columns, a ragged
# non-square grid and the miniature's
EXACT_CASES = [(Cin, Cout, h, w) for Cin in (64, 192) for Cout in (16, 48) for h, w in ((3, 5), (6, 6))]

# rel-L2 against the fp32 reference neck (nn.ConvTranspose2d on unrounded operands, evaluated in float64): 3 x the worst MI355X measurement
# over both backbone fixtures (profiles/neck_parity.md: outputs 2.3387e-3, parameter gradients 3.4052e-3, both on tiny_fvit_backbone_g6)
BOUND_NECK_OUT_REL_L2, BOUND_NECK_GRAD_REL_L2 = 7.02e-3, 1.03e-2


def index_rows_to_nchw(rows, B, h, w, C, s, off, dtype):
    """out[b, c, s*i + di, s*j + dj] = rows[b*(P + off) + off + i*w + j, (di*s + dj)*C + c], one rounding at `dtype`."""
    P = h * w
    r = rows[:, :s * s * C].reshape(B, P + off, s, s, C)[:, off:].reshape(B, h, w, s, s, C)        # b i j di dj c
    return r.permute(0, 5, 1, 3, 2, 4).reshape(B, C, s * h, s * w).contiguous().to(dtype)


def index_nchw_to_rows(x, B, h, w, C, s, off, rows):
    """The inverse into `rows` (bf16, RNE): columns past s*s*C untouched, the CLS rows (off = 1) zero in [0, s*s*C)."""
    P = h * w
    v = x.reshape(B, C, h, s, w, s).permute(0, 2, 4, 3, 5, 1).reshape(B, P, s * s * C).to(rows.dtype)
    for b in range(B):
        if off:
            rows[b * (P + off), :s * s * C] = 0
        rows[b * (P + off) + off:(b + 1) * (P + off), :s * s * C] = v[b]


class RefOpsNeck(RefOpsBackbone):
    name = "ref+taps+neck"
    DECONV_ROWS = True

    def rows_to_nchw(self, rows, B, h, w, C, s, off, out):
        assert rows.dim() == 2 and rows.shape[0] == B * (h * w + off) and rows.shape[1] >= s * s * C and rows.dtype in (F32, BF)
        assert out.is_contiguous() and tuple(out.shape) == (B, C, s * h, s * w) and out.dtype in (F32, BF)
        out.copy_(index_rows_to_nchw(rows, B, h, w, C, s, off, out.dtype))

    def nchw_to_rows(self, x, B, h, w, C, s, off, rows):
        assert rows.dim() == 2 and rows.shape[0] == B * (h * w + off) and rows.shape[1] >= s * s * C and rows.dtype == BF
        assert x.is_contiguous() and tuple(x.shape) == (B, C, s * h, s * w) and x.dtype in (F32, BF)
        index_nchw_to_rows(x, B, h, w, C, s, off, rows)


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_operands(B, Cin, Cout, h, w, seed):
    """x [B, Cin, h, w], weight [Cin, Cout, 2, 2], bias [Cout], dy [B, Cout, 2h, 2w]: fp32 values that bf16 holds exactly."""
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).to(F32)
    return r(B, Cin, h, w), (r(Cin, Cout, 2, 2) * Cin ** -0.5).to(BF).to(F32), r(Cout), r(B, Cout, 2 * h, 2 * w)


def exact_operands(B, Cin, Cout, h, w, seed):
    """The same four tensors holding integers in [-8, 8]."""
    g = _gen(seed)
    r = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)
    return r(B, Cin, h, w), r(Cin, Cout, 2, 2), r(Cout), r(B, Cout, 2 * h, 2 * w)


def to_rows(x, off):
    """NCHW fp32 -> the tower's stream form: bf16 [B*(h*w + off), C] with NaN-free, non-zero CLS rows (they must not reach any result
    but the discarded CLS rows of Y)."""
    B, C, h, w = x.shape
    rows = torch.full((B, h * w + off, C), 3.0)
    rows[:, off:] = x.reshape(B, C, h * w).permute(0, 2, 1)
    return rows.reshape(B * (h * w + off), C).to(BF)


# ------------------------------------------------------------------------------------------------ references
def reference(x, weight, bias, dy, need_dx=True):
    """float64 F.conv_transpose2d under autograd -> dict(y, dw, db, dx) and the per-element sums of |terms| (ay, adw, adb, adx) the
    accumulation bounds are made of."""
    x64, w64, b64, dy64 = (t.double() for t in (x, weight, bias, dy))
    x64.requires_grad_(need_dx)
    w64.requires_grad_(True)
    b64.requires_grad_(True)
    y = F.conv_transpose2d(x64, w64, b64, stride=2)
    y.backward(dy64)
    with torch.no_grad():
        ay = F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
        # dw[ci, co, di, dj] = sum_{b,i,j} x[b, ci, i, j] * dy[b, co, 2i + di, 2j + dj];  dx[b, ci, i, j] = sum_{co,di,dj} dy * w
        B, Cout, H2, W2 = dy.shape
        dyq = dy64.abs().reshape(B, Cout, H2 // 2, 2, W2 // 2, 2)
        adw = torch.einsum("bcij,bdiejf->cdef", x64.detach().abs(), dyq)
        adx = torch.einsum("bdiejf,cdef->bcij", dyq, w64.detach().abs())
        adb = dy64.abs().sum((0, 2, 3))
    return dict(y=y.detach(), dw=w64.grad, db=b64.grad, dx=x64.grad if need_dx else None, ay=ay, adw=adw, adb=adb, adx=adx)


class ExactnessError(AssertionError):
    pass


def exact_reference(x, weight, bias, dy, need_dx=True):
    """reference() on exact operands; asserts that every sum of |terms| stays below 2^24 (else the case, not a kernel, is wrong)."""
    ref = reference(x, weight, bias, dy, need_dx)
    for k in ("ay", "adw", "adb", "adx"):
        if not float(ref[k].max()) < TWO24:
            raise ExactnessError(f"{k}: sum of |terms| {float(ref[k].max())} reaches 2^24: fp32 accumulation is not exact for this case")
    for k in ("y", "dw", "db", "dx"):
        if ref[k] is not None:
            assert torch.equal(ref[k], ref[k].round()) and torch.equal(ref[k].to(F32).double(), ref[k])
    return ref


def bound(abs_terms, K, reference_value=None, bf16_out=False):
    """Per-element bound of an fp32 accumulation of K terms whose absolute values sum to abs_terms (+ half a bf16 ulp of the result)."""
    b = 2.0 * K * U * abs_terms
    if bf16_out:
        b = b + 2.0 ** -8 * (reference_value.abs() + b)
    return b


def check_bound(name, got, want, tol):
    err = (got.detach().double().cpu() - want).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= tol).all()), f"{name}: {int((err > tol).sum())} of {err.numel()} elements past the bound, worst ratio {worst:.3f}"


def rne_bf16(x64):
    """Round-to-nearest-even bf16 image of exactly fp32-representable float64 values."""
    return x64.to(F32).to(BF)
