"""Float64 statements, element-wise bounds, cases and the comparator for the point-wise, column-sum, L2-norm and loss kernels
(cs_gelu_fwd/bwd, cs_swiglu_fwd/bwd/bwd_q8/bwd_colsum, cs_cast_f32_bf16, cs_colsum_bf16, cs_l2norm_fwd/bwd, cs_cosine_loss_fwd/bwd,
cs_fed_bce_fwd/bwd).  tests/test_pointwise_ref_cpu.py checks this module against fp32 restatements and planted errors on the CPU;
tests/test_gpu_pointwise.py runs the kernels against it.  Nothing here imports the code under test.

Bounds.  u = 2^-24 is the fp32 unit roundoff: one rounded operation errs by at most u |result|.  expf, logf and log1pf are documented at
1 ulp (relative 2u).  FLOOR = 2^-126 is the smallest normal of fp32 and bf16: what the device exp and the bf16 conversion do below it is
not documented, so every bound carries FLOOR once for its output.

  Fast sigmoid forms (SiLU, QuickGELU; c = 1 or 1.702), e = exp2(fl(-c x log2 e)), s = 1 / (1 + e).  The figures are the ones of
    _exact_gemm.act_case:  REL = 2^-17 |want| covers exp2 and the reciprocal at 1 ulp, the three roundings of the exponent's argument
    (the product c x, the constant, the product with log2 e) amplified by |c x| ln 2 <= 27 at |x| <= 16, and a few roundings.  That was
    stated for |x| <= 16; the amplification grows linearly in |x|, so here REL(x) = 2^-17 max(1, |x| / 16).  It stops growing at
    |x| = 128 (REL <= 2^-14): beyond it |c x| log2 e > 184, exp2 returns exactly 0 or inf and s is exactly 1 or 0.
  Intermediates below FLOOR.  e, s, s (1 - s) and their products with x are fp32 values of their own: each may be flushed when it is below
    FLOOR (an e that overflows to inf is the same event: then s < 2^-128 becomes 0), and each is afterwards multiplied by at most
    c |x| <= 2 |x| or by 1.  At most four such intermediates:      FLINT(x) = 8 FLOOR max(1, min(|x|, 128)).
    Beyond |x| = 128 a flushed intermediate loses at most its own true value, which is below exp(-|x|) there, and
    2 |x| exp(-|x|) <= 256 exp(-128) < FLOOR: the factor stops growing with REL's.
  x * sigmoid(c x):                      E = REL(x) |want| + FLINT
  GELU (erf) forward 0.5 x (1 + erf(x / sqrt 2)):  2^-22 |x| covers erf (4 ulp) under the cancellation of 1 + erf, as in act_case:
                                         E = REL(x) |want| + 2^-22 |x| + FLINT
  GELU (erf) gradient PHI + x phi, PHI = 0.5 (1 + erf), phi = exp(-x^2/2) / sqrt(2 pi):  PHI: erf at 4 ulp is 4u absolute, one rounding u.
    x phi: the exponent's argument x^2/2 carries 3u, amplified to 1.5 x^2 u; exp2, two products and the constant 6u:
    (1.5 x^2 + 6) u |x| phi <= 0.7u + 1.5u (maxima of x^3 exp(-x^2/2) and x exp(-x^2/2)).  The sum: u |want| <= 1.2u.  Together < 16u:
                                         E = 2^-20 + FLINT
  Sigmoid gradients g = s + T, T = c x s (1 - s):  s and T each within REL(x) of themselves, but they cancel near c x (1 - s) = -1, so
    REL applies to s + |T|.  1 - s is exact given the computed s, which errs by 3u s absolutely (the sum 1 + e and the reciprocal) however
    small 1 - s is; T inherits c |x| s 3u s <= 8u |x| s^2 (CANCEL, a term the project's figures do not hold: they were stated for the
    forward).  CANCEL applies up to |x| = 128 only: beyond it e is exactly 0 or inf, the sum 1 + e is 1 or inf and its reciprocal
    (a division, or a reciprocal instruction: both return 1 for 1 and 0 for inf) is exactly 1 or 0, so 1 - s, T and g carry no
    error at all and the bound there is REL(x) g + FLINT beside the bf16 rounding: a wrong finite gradient on the largest
    inputs is rejected.
                                         E = REL(x) (s + |T|) + 8u |x| s^2 [|x| <= 128] + FLINT
  Products with the companions (dy; x2 and dh of SwiGLU; values exactly representable in bf16): the unary bound times |companion|, plus
    one u |want| per product and one of slack.  A bf16 output adds half a bf16 spacing at the float64 value, and FLOOR.
  ACT_MAX_SHARE: beside the bound, at most 1 % of the elements of a case of >= 1024 elements may differ from bf16(float64 value) at all.
    It is a condition, not a measurement: a plain fp32 evaluation differs on 0.03 % (QuickGELU, SiLU) to 0.3 % (GELU) of the inputs,
    all of them flushed subnormals or the cancelling negative tail.

  Cast: bit-equal to round-to-nearest-even of the fp32 bits; a NaN gives a NaN.
  Column sums: integer inputs in [-8, 8] and integer starting values, every partial sum below 2^24: any fp32 order gives the one
    integer result, compared bit for bit.

  L2 norm, row of C fp32 entries.  ss = sum x^2: C products and C - 1 sums in any order, relative (C + 1) u.  sqrt and the reciprocal at
    2u each (correctly rounded gives u; one of slack):      r = ((C + 1) / 2 + 5) u,  |inv - INV| <= r INV,  |y - Y| <= (r + 2u) |Y| + FLOOR.
    A clamped row (norm < eps, never within 4 r of eps in a case) has inv = fl(1 / eps): r = 2u.
    Backward, from the fp32-rounded y and inv of the statement (so it does not inherit the forward's error):  dot = sum y dy errs by
    EDOT = (C + 1) u sum |y dy|;  dx = fl(fl(dy - fl(y dot)) inv):
      |dx - DX| <= inv (|y| EDOT + u |y dot| + u |dy - y dot|) + 2u |DX| + half a bf16 spacing + FLOOR.   (An fma only removes a rounding.)
    Rows of +-2^k entries with C a power of four: norm, inverse, y, dot and dy - y dot are exact; dx is one bf16 rounding of an exact
    value.  Bit for bit.

  Cosine loss, rows of E entries.  is = 1 / max(|s|, eps), it likewise: relative r(E) as above.  st = sum s t errs by
    EST = (E + 1) u sum |s t|.  cos = fl(fl(st is) it):      |cos - COS| <= EST IS IT + (2 r + 3u) |COS|.
    loss = weight (1 - sum cos / K), K terms in any order:
      |loss - LOSS| <= weight (sum ECOS / K + u sum |COS| + u |MEAN| + u |1 - MEAN|) + 2u |LOSS|.
    Backward from the fp32-rounded stats; coef = fl(fl(-weight grad_scale) / K) is host arithmetic, the same number on both sides; times
    upstream: u.  ds = coef fl(fl(t it) - fl(fl(cos s) is)) is:
      |ds - DS| <= |coef| is (u |t it| + 2u |cos s is| + u |t it - cos s is|) + 4u |DS| + FLOOR.
    Rows of +-1 at E = 4 or 256 (norms 2 or 16, cosines multiples of 1/E), K a power of two and dyadic weights: all exact, bit for bit.

  Federated BCE.  z = fl(logit temp): u |z|.  a = max(z, 0) - z t is exact given z (it is z, -z or 0).  e = expf(-|z|): (4 |z| + 2) u
    (its own 2u, the argument's u |z| and the 3u |z| of the exp2 form).  l = log1pf(e): the true log1p moves by at most the relative
    change of e, plus 2u: RL = (4 |z| + 4) u.  Two sums.      |term - TERM| <= u |z| [a != 0] + RL L + 2u (|a| + L)
    row: ns terms in any order: sum of the term bounds + ns u ROW + ns FLOOR.  loss = weight sum rows / K:
      |loss - LOSS| <= weight (sum row bounds + K u sum ROW) / K + 3u |LOSS|.
    dz = fl(fl(coef temp) (sig - t)), coef = fl(weight / K) on the host (the same number on both sides), times upstream u.  sig errs by
    sig (1 - sig) (4 |z| + 2) u + 3u sig; sig - t adds u |sig - t| (on the target column sig - 1 cancels: the 3u sig stays):
      |dz - DZ| <= |coef temp| (DSIG + u |SIG - t|) + 4u |DZ| + half a bf16 spacing + FLOOR.
    Logits 0 with dyadic coef and temp: expf(0) = 1, sig = 0.5, dz = coef temp (0.5 - t) bit for bit.  Padding columns are zero.

The comparator reports the number of elements outside the bound, the first of them (row, column, input, got, want, bound) and the worst
err / bound of the case.  Cases are generated from seeds; nothing is read from outside the repository."""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -126
ACT_MAX_SHARE = 0.01
SHARE_MIN_ELEMENTS = 1024          # a smaller case (the q8 cases at Hd = 8) cannot spend a 1 % share: it is compared element by element only
F32 = np.float32
F64 = np.float64
QUICK_C = 1.702
L2_EPS = float(F32(1e-12))
COLSUM_ROWS = 64                   # rows per block of cs_colsum_bf16 (include/clipself_hip.h: cs_colsum_workspace)


# ================================================================================================ number formats
def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def f32_bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def rne_bits(x32):
    """fp32 -> bf16 bits, round to nearest even on the bit pattern; NaN keeps its sign and top mantissa bits, quieted."""
    b = f32_bits(x32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x32, F32)), ((b >> 16) | 0x40).astype(np.uint16), r)


def trunc_bits(x32):
    return (f32_bits(x32) >> 16).astype(np.uint16)


def bits_of(v):
    """bf16 bits of values that are exactly representable (asserted)."""
    v32 = np.asarray(v, F64).astype(F32)
    b = rne_bits(v32)
    assert np.array_equal(bf16_to_f32(b).astype(F64), np.asarray(v, F64)), "value is not a bf16 number"
    return b


def bf16_spacing(w):
    """Distance between neighbouring bf16 numbers at |w| (2^-133 in the subnormal range and at 0)."""
    w = np.asarray(w, F64)
    _, e = np.frexp(np.abs(w))
    e = np.where(w == 0, -125, np.maximum(e, -125))
    return np.ldexp(1.0, e - 8)


BF16_MAX = float(bf16_to_f32(np.uint16(0x7F7F)))


def bf16_round64(w):
    """Round-to-nearest-even bf16 image of float64 values, as float64 (no double rounding through fp32)."""
    w = np.asarray(w, F64)
    s = bf16_spacing(w)
    q = np.rint(w / s) * s
    return np.where(np.abs(q) > BF16_MAX, np.copysign(np.inf, w), q)


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ================================================================================================ comparator
def compare(name, got, want, bound, inputs=None):
    """-> (message or None, worst err / bound).  got / want / bound broadcast to want's shape (rows x columns, or a vector); inputs: an
    array of want's shape (or a dict of them) printed for the first offender."""
    want = np.asarray(want, F64)
    got = np.asarray(got, F64).reshape(want.shape)
    bound = np.broadcast_to(np.asarray(bound, F64), want.shape)

    def where(mask):
        idx = np.unravel_index(int(np.argmax(mask)), want.shape)
        row, col = (idx + (0,))[:2] if want.ndim >= 2 else (0, idx[0] if idx else 0)
        ins = inputs if isinstance(inputs, dict) else ({} if inputs is None else {"input": inputs})
        shown = ", ".join(f"{k} {float(np.asarray(v).reshape(want.shape)[idx])!r}" for k, v in ins.items())
        return idx, f"row {int(row)} column {int(col)}" + (f" ({shown})" if shown else "")

    bad = ~np.isfinite(got)
    if bad.any():
        _, at = where(bad)
        return f"{name}: {int(bad.sum())} non-finite outputs (a NaN may be the prefill: not written), first at {at}", float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    over = err > bound
    if over.any():
        idx, at = where(over)
        return (f"{name}: {int(over.sum())} of {over.size} elements outside the bound, first at {at}: got {float(got[idx])!r} want "
                f"{float(want[idx])!r} bound {float(bound[idx]):.3e}; worst err / bound {worst:.3g}"), worst
    return None, worst


def share_differing(got, want):
    """Share of the elements that are not the bf16 image of the float64 value (signed zeros count as equal)."""
    got = np.asarray(got, F64).reshape(np.shape(want))
    return float(np.mean(got != bf16_round64(want)))


def share_message(name, share, n):
    if n >= SHARE_MIN_ELEMENTS and share > ACT_MAX_SHARE:
        return f"{name}: {share:.2%} of the elements differ from bf16(float64 value), more than {ACT_MAX_SHARE:.0%}"
    return None


# ================================================================================================ unary activations: the table
PATTERNS = np.arange(65536, dtype=np.uint32).astype(np.uint16)
X32 = bf16_to_f32(PATTERNS)
FINITE = np.isfinite(X32)
X64 = np.where(FINITE, X32, 0).astype(F64)
UNARY = ("gelu", "quick", "silu", "gelu_grad", "quick_grad", "silu_grad")


def _sig(z):
    """(sigmoid(z), sigmoid(-z)), neither by cancellation."""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(z >= 0, big, small), np.where(z >= 0, small, big)


def _erfc(a):
    return torch.erfc(torch.from_numpy(np.ascontiguousarray(a, F64))).numpy()


def unary64(kind, x):
    """-> (float64 value, evaluation bound E of the docstring) of one of UNARY at the float64 points x."""
    x = np.asarray(x, F64)
    ax = np.abs(x)
    rel = 2.0 ** -17 * np.clip(ax / 16.0, 1.0, 8.0)
    flint = 8.0 * FLOOR * np.clip(ax, 1.0, 128.0)
    with np.errstate(over="ignore", under="ignore"):
        if kind == "gelu":
            w = x * (0.5 * _erfc(-x / math.sqrt(2.0)))
            return w, rel * np.abs(w) + 2.0 ** -22 * ax + flint
        if kind == "gelu_grad":
            w = 0.5 * _erfc(-x / math.sqrt(2.0)) + x * (np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))
            return w, 2.0 ** -20 + flint
        c = QUICK_C if kind.startswith("quick") else 1.0
        s, q = _sig(c * x)
        if kind in ("quick", "silu"):
            w = x * s
            return w, rel * np.abs(w) + flint
        assert kind in ("quick_grad", "silu_grad"), kind
        t = (c * x) * (s * q)
        return s + t, rel * (s + np.abs(t)) + 8.0 * U * ax * s * s * (ax <= 128.0) + flint


_TABLE = {}


def table(kind):
    """pattern -> (float64 value, evaluation bound); the non-finite patterns hold the entry of 0."""
    if kind not in _TABLE:
        _TABLE[kind] = unary64(kind, X64)
    return _TABLE[kind]


def _half(w):
    return 0.5 * bf16_spacing(w)


COMPANIONS = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 7.5, -3.28125, 1.3828125, -0.08642578125, 0.0035400390625, -5.84375])
SMALL_COMPANIONS = COMPANIONS[:5]        # for |x| >= 2^120, where a factor above 1 would overflow


def patterns(M, N, offset=0):
    """[M, N] uint16: element (r, c) holds pattern (r N + c + offset) mod 65536; the non-finite ones are replaced by 0."""
    p = ((np.arange(M * N, dtype=np.int64) + offset) % 65536).astype(np.uint16)
    return np.where(FINITE[p], p, np.uint16(0)).reshape(M, N)


def companions(pat, salt, ones=False):
    """Float64 companion values (bf16 numbers) for the pattern matrix: the fixed set cycled with period 11 (coprime to 65536), the
    five of magnitude <= 1 where |x| >= 2^120, so every product of the kernels stays finite.  ones: all 1."""
    if ones:
        return np.ones(pat.shape)
    i = np.arange(pat.size, dtype=np.int64) + salt
    big = np.abs(X64[pat.ravel()]) >= 2.0 ** 120
    return np.where(big, SMALL_COMPANIONS[i % 5], COMPANIONS[i % 11]).reshape(pat.shape)


def expect_act_fwd(kind, pat):
    w, e = table(kind)
    W = w[pat]
    return W, _half(W) + e[pat] + FLOOR


def expect_act_bwd(kind, pat, dy):
    w, e = table(kind + "_grad")
    W = dy * w[pat]
    return W, _half(W) + np.abs(dy) * e[pat] + 2 * U * np.abs(W) + FLOOR


def expect_swiglu_fwd(pat, x2):
    w, e = table("silu")
    W = w[pat] * x2
    return W, _half(W) + np.abs(x2) * e[pat] + 2 * U * np.abs(W) + FLOOR


def expect_swiglu_bwd(pat, x2, dh):
    """-> (want [M, 2 Hd], bound) of dx12 = [dh x2 g(x1) | dh silu(x1)]."""
    g, eg = table("silu_grad")
    s, es = table("silu")
    W1, W2 = dh * x2 * g[pat], dh * s[pat]
    b1 = _half(W1) + np.abs(dh * x2) * eg[pat] + 3 * U * np.abs(W1) + FLOOR
    b2 = _half(W2) + np.abs(dh) * es[pat] + 3 * U * np.abs(W2) + FLOOR
    return np.concatenate([W1, W2], 1), np.concatenate([b1, b2], 1)


# (name, M, N, padding columns of the row stride, companions all 1)
ACT_SHAPES = [("32x2048", 32, 2048, 0, True), ("8192x8", 8192, 8, 8, False), ("128x512", 128, 512, 64, False)]
Q8_SHAPES = [(M, Hd) for Hd in (8, 2048, 2056, 3072, 3080, 4096) for M in (1, 3, 4, 5)]
WRAP_ROWS, WRAP_COLS, WRAP_CAST = 4100, 2048, 8396800        # just over 4096 workgroups x 256 threads x 8 elements
GRID_CAP_VECTORS = 4096 * 256


def q8_offsets():
    """Pattern offset of each q8 case: the running element count, so the cases together walk the whole domain."""
    out, off = {}, 0
    for M, Hd in Q8_SHAPES:
        out[(M, Hd)] = off
        off += M * Hd
    return out


# ---- fp32 restatements (numpy) of the kernels' expressions, with the planted variants --------------------------------------------
LOG2E32 = F32(1.4426950408889634)


def _exp32(x):
    with np.errstate(all="ignore"):
        return np.exp2((np.asarray(x, F32) * LOG2E32).astype(F32)).astype(F32)


def _erf32(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, F32))).numpy()


def unary32(kind, x, c=1.702, form="fixed", tanh=False):
    """One of UNARY in fp32 as the kernels write it.  c: the QuickGELU constant (planted: 1.7); form "parent": the QuickGELU gradient
    s (1 + c x (1 - s)) of the parent commit; tanh: the tanh approximation in the place of erf (planted)."""
    x = np.asarray(x, F32)
    one, half = F32(1), F32(0.5)
    with np.errstate(all="ignore"):
        if kind == "gelu":
            if tanh:
                return half * x * (one + np.tanh(F32(0.7978845608) * (x + F32(0.044715) * x * x * x)))
            return half * x * (one + _erf32(x * F32(0.70710678118654752)))
        if kind == "gelu_grad":
            return half * (one + _erf32(x * F32(0.70710678118654752))) + x * F32(0.3989422804014327) * _exp32(F32(-0.5) * x * x)
        c = F32(c) if kind.startswith("quick") else one
        e = _exp32(-c * x)
        if kind in ("quick", "silu"):
            return x / (one + e)
        s = one / (one + e)
        if kind == "silu_grad":
            return s + x * s * (one - s)
        if form == "parent":
            return s * (one + c * x * (one - s))
        return s + c * (x * (s * (one - s)))


# ================================================================================================ cast
def cast_inputs():
    """fp32 bit patterns: for each of the 65 536 upper halves (every bf16 value, +-0, +-inf, NaNs, the subnormals), the lower halves
    0 (the value itself), 1, 0x7FFF, 0x8000 (the midpoint to the next bf16 number, for both parities of the lower neighbour), 0x8001
    and 0xFFFF: the ties +-1 fp32 ulp, the smallest fp32 subnormals, and the largest fp32 values on both sides of 0x7F7F8000, where
    bf16 rounds to infinity."""
    hi = PATTERNS.astype(np.uint32) << 16
    low = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)
    return (hi[:, None] | low[None, :]).reshape(-1)


def cast_mismatch(name, in_bits, got_bits):
    x = in_bits.view(F32)
    want = rne_bits(x)
    got_bits = np.asarray(got_bits, np.uint16).reshape(want.shape)
    nan = np.isnan(x)
    got_nan = ((got_bits & 0x7F80) == 0x7F80) & ((got_bits & 0x7F) != 0)
    bad = np.where(nan, ~got_nan, got_bits != want)
    if bad.any():
        i = int(np.argmax(bad))
        return (f"{name}: {int(bad.sum())} of {bad.size} elements are not round-to-nearest-even, first at {i}: input bits "
                f"{int(in_bits[i]):#010x} ({float(x[i])!r}) got {int(got_bits[i]):#06x} want {int(want[i]):#06x}")
    return None


# ================================================================================================ column sums
COLSUM_M = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 333, 2119)
COLSUM_N = (8, 504, 512, 520, 770, 7)
# name -> (M, N, row stride, element offset of the pointer)
# the row stride is a multiple of 8 on an aligned pointer throughout, so with N % 8 != 0 only the thread of the ragged last vector takes
# the scalar branch, beside vector threads of the same workgroup; the all-scalar launches are the two cases added below
COLSUM_CASES = {f"M{M}-N{N}": (M, N, (N + 7) // 8 * 8 + (8 if N % 8 == 0 else 0), 0) for N in COLSUM_N for M in COLSUM_M}
COLSUM_CASES["M333-N512-ld515"] = (333, 512, 515, 0)
COLSUM_CASES["M333-N512-offset1"] = (333, 512, 520, 1)
FUSED_COLSUM_SHAPES = [(M, Hd) for Hd in (8, 504, 520) for M in (1, 3, 4, 5, 63, 64, 65)]


def colsum_case(name):
    """-> dict(M, N, ld, offset, flat [offset + M ld] float64 integers (100 = padding, never to be read), x [M, N] view, start [N], want [N])."""
    M, N, ld, off = COLSUM_CASES[name]
    rng = np.random.default_rng(1000 * M + N + ld + off)
    flat = np.full(off + M * ld, 100.0)
    rows = flat[off:].reshape(M, ld)
    rows[:, :N] = rng.integers(-8, 9, (M, N))
    start = rng.integers(-100, 101, N).astype(F64)
    x = rows[:, :N]
    want = start + x.sum(0)
    assert float(np.abs(start).max() + np.abs(x).sum(0).max()) < 2 ** 24, "a partial sum can leave the exact integers of fp32"
    return dict(M=M, N=N, ld=ld, offset=off, flat=flat, x=x, start=start, want=want)


def colsum_restated(x, start, drop=None):
    """The kernel's structure on exact integers: row blocks of COLSUM_ROWS, then their sum.  drop = (block, column): that block forgets
    its last row in that column (planted)."""
    M, N = x.shape
    out = start.copy()
    for b in range((M + COLSUM_ROWS - 1) // COLSUM_ROWS):
        blk = x[b * COLSUM_ROWS:min(M, (b + 1) * COLSUM_ROWS)]
        part = blk.sum(0)
        if drop is not None and drop[0] == b:
            part[drop[1]] -= blk[-1, drop[1]]
        out += part
    return out


# ================================================================================================ L2 norm
L2_C = (4, 252, 256, 260, 1028)
L2_M = (1, 3, 4, 5, 9)
L2_KINDS = ("zero", "tiny", "dominant", "seeded")
L2_CASES = {f"M{M}-C{C}": (M, C, iM + iC, False) for iM, M in enumerate(L2_M) for iC, C in enumerate(L2_C)}
L2_CASES.update({f"exact-M{M}-C{C}": (M, C, 0, True) for M in L2_M for C in (4, 256)})


def _r_norm(C):
    return ((C + 1) / 2.0 + 5.0) * U


def l2_case(name):
    """-> dict(x, dy fp32 [M, C], kinds, exact, and l2_ref's outputs).  Row r of a mixed case has kind L2_KINDS[(r + shift) % 4]."""
    M, C, shift, exact = L2_CASES[name]
    rng = np.random.default_rng(7000 + 10 * M + C)
    if exact:
        k, j = rng.integers(-8, 9, (M, 1)), rng.integers(-4, 5, (M, 1))
        x = np.ldexp(rng.choice([-1.0, 1.0], (M, C)), k).astype(F32)
        dy = np.ldexp(rng.choice([-1.0, 1.0], (M, C)), j).astype(F32)
        kinds = ["pow2"] * M
    else:
        kinds = [L2_KINDS[(r + shift) % 4] for r in range(M)]
        x, dy = rng.normal(0, 1, (M, C)).astype(F32), rng.normal(0, 1, (M, C)).astype(F32)
        for r, kind in enumerate(kinds):
            if kind == "zero":
                x[r] = 0
            elif kind == "tiny":
                x[r] *= F32(1e-14)
            elif kind == "dominant":
                x[r] *= F32(1e-3)
                x[r, (3 * r + 1) % C] = F32(-1e3 if r % 2 else 1e3)
    c = dict(M=M, C=C, x=x, dy=dy, kinds=kinds, exact=exact)
    c.update(l2_ref(x, dy, exact))
    return c


def l2_ref(x, dy, exact=False, clamp=True):
    X, G = x.astype(F64), dy.astype(F64)
    C = X.shape[1]
    norm = np.sqrt((X * X).sum(1))
    r = _r_norm(C)
    clamped = norm < L2_EPS
    assert np.all(np.abs(norm - L2_EPS) > 4 * r * L2_EPS), "a row's norm sits on the eps clamp"
    with np.errstate(divide="ignore", invalid="ignore"):
        INV = 1.0 / (np.maximum(norm, L2_EPS) if clamp else norm)
        rr = np.where(clamped, 2 * U, r)
        Y = X * INV[:, None]
        y32, inv32 = Y.astype(F32), INV.astype(F32)                       # the backward's inputs: the rounded statement
        Yq, Iq = y32.astype(F64), inv32.astype(F64)[:, None]
        dot = (Yq * G).sum(1)[:, None]
        edot = (C + 1) * U * np.abs(Yq * G).sum(1)[:, None]
        ad = Yq * dot
        diff = G - ad
        DX = diff * Iq
        ev = Iq * (np.abs(Yq) * edot + U * np.abs(ad) + U * np.abs(diff)) + 2 * U * np.abs(DX)
    out = dict(inv=INV, inv_b=rr * INV, y=Y, y_b=(rr + 2 * U)[:, None] * np.abs(Y) + FLOOR, y32=y32, inv32=inv32, clamped=clamped,
               dx=DX, dx_b=_half(DX) + ev + FLOOR)
    if exact:
        assert np.array_equal(Yq, Y) and np.array_equal(Iq[:, 0], INV), "an exact case is not exact"
        out.update(inv_b=np.zeros_like(INV), y_b=np.zeros_like(Y), dx=bf16_round64(DX), dx_b=np.zeros_like(DX))
    return out


def l2_restated(x, dy, y32, inv32, clamp=True):
    """fp32 restatement: (inv, y, dx bf16 values); the backward from the given y32 / inv32.  clamp=False drops max(., eps) (planted)."""
    with np.errstate(all="ignore"):
        ss = (x * x).sum(1, dtype=F32)
        n = np.sqrt(ss)
        inv = (F32(1) / (np.maximum(n, F32(L2_EPS)) if clamp else n)).astype(F32)
        y = x * inv[:, None]
        dot = (y32 * dy).sum(1, dtype=F32)[:, None]
        dx = (dy - y32 * dot) * inv32[:, None]
    return inv, y, bf16_to_f32(rne_bits(dx)).astype(F64)


# ================================================================================================ cosine loss
COS_K = (1, 3, 4, 5, 255, 256, 257, 600)
COS_E = (4, 252, 260, 512)
# name -> (K, E, exact)
COS_CASES = {f"K{K}-E{E}": (K, E, False) for K in COS_K for E in COS_E}
COS_CASES.update({f"exact-K{K}-E{E}": (K, E, True) for K in (1, 4, 256) for E in (4, 256)})
COS_UPSTREAM = 0.25


def cos_case(name):
    """-> dict(s, t fp32 [K, E], weight, grad_scale, exact, kinds and cos_ref's outputs).  Exact rows cycle through s = t, s = -t,
    orthogonal (half of the signs flipped) and random signs; a seeded case of K >= 3 has a zero student row (the eps clamp)."""
    K, E, exact = COS_CASES[name]
    rng = np.random.default_rng(9000 + 10 * K + E)
    if exact:
        t = rng.choice([-1.0, 1.0], (K, E)).astype(F32)
        s = rng.choice([-1.0, 1.0], (K, E)).astype(F32)
        kinds = [("same", "opposite", "orthogonal", "random")[k % 4] for k in range(K)]
        for k, kind in enumerate(kinds):
            if kind == "same":
                s[k] = t[k]
            elif kind == "opposite":
                s[k] = -t[k]
            elif kind == "orthogonal":
                s[k] = t[k]
                s[k, :E // 2] *= -1
        weight, gs = 0.5, 2.0
    else:
        s, t = (0.3 * rng.normal(0, 1, (K, E))).astype(F32), (2.0 * rng.normal(0, 1, (K, E))).astype(F32)
        kinds = ["seeded"] * K
        if K >= 3:
            s[1] = 0
            kinds[1] = "zero"
        weight, gs = 0.7, 1.5
    c = dict(K=K, E=E, s=s, t=t, weight=weight, grad_scale=gs, exact=exact, kinds=kinds)
    c.update(cos_ref(s, t, weight, gs, exact))
    return c


def cos_coef(weight, gs, K):
    return float((-F32(weight) * F32(gs)) / F32(K))


def cos_ref(s, t, weight, gs, exact=False):
    """stats / loss with bounds, and ds (without and with upstream = COS_UPSTREAM) from the fp32-rounded stats."""
    S, T = s.astype(F64), t.astype(F64)
    K, E = S.shape
    w = float(F32(weight))
    r = _r_norm(E)

    def inv_norm(A):
        n = np.sqrt((A * A).sum(1))
        assert np.all(np.abs(n - L2_EPS) > 4 * r * L2_EPS)
        return 1.0 / np.maximum(n, L2_EPS), np.where(n < L2_EPS, 2 * U, r)

    IS, rs = inv_norm(S)
    IT, rt = inv_norm(T)
    ST = (S * T).sum(1)
    COS = ST * IS * IT
    ecos = (E + 1) * U * np.abs(S * T).sum(1) * IS * IT + (rs + rt + 3 * U) * np.abs(COS)
    stats = np.stack([COS, IS, IT], 1)
    stats_b = np.stack([ecos, rs * IS, rt * IT], 1)
    mean = COS.sum() / K
    LOSS = w * (1.0 - mean)
    loss_b = w * (ecos.sum() / K + U * np.abs(COS).sum() + U * abs(mean) + U * abs(1 - mean)) + 2 * U * abs(LOSS)
    st32 = stats.astype(F32)
    q = st32.astype(F64)
    coef = cos_coef(weight, gs, K)
    a, b = T * q[:, 2:3], q[:, 0:1] * S * q[:, 1:2]
    core = (a - b) * q[:, 1:2]
    ecore = q[:, 1:2] * (U * np.abs(a) + 2 * U * np.abs(b) + U * np.abs(a - b))
    out = dict(stats=stats, stats_b=stats_b, loss=LOSS, loss_b=loss_b, stats32=st32, coef=coef)
    for key, up in (("ds", 1.0), ("ds_up", COS_UPSTREAM)):
        DS = coef * up * core
        out[key], out[key + "_b"] = DS, abs(coef * up) * ecore + 4 * U * np.abs(DS) + FLOOR
    if exact:
        assert np.array_equal(q, stats) and float(F32(LOSS)) == LOSS, "an exact case is not exact"
        for key in ("ds", "ds_up"):
            assert np.array_equal(out[key].astype(F32).astype(F64), out[key])
            out[key + "_b"] = np.zeros_like(out[key])
        out.update(stats_b=np.zeros_like(stats), loss_b=0.0)
    return out


def cos_restated(s, t, stats32, weight, gs, upstream=None, final_is=True):
    """fp32 restatement -> (stats, loss, ds); the backward from stats32.  final_is=False drops the last `* is` (planted)."""
    K, E = s.shape
    ss, tt, st = (s * s).sum(1, dtype=F32), (t * t).sum(1, dtype=F32), (s * t).sum(1, dtype=F32)
    i_s, i_t = F32(1) / np.maximum(np.sqrt(ss), F32(L2_EPS)), F32(1) / np.maximum(np.sqrt(tt), F32(L2_EPS))
    stats = np.stack([st * i_s * i_t, i_s, i_t], 1).astype(F32)
    loss = F32(weight) * (F32(1) - stats[:, 0].sum(dtype=F32) / F32(K))
    coef = F32(cos_coef(weight, gs, K)) * (F32(1) if upstream is None else F32(upstream))
    q = stats32
    ds = coef * (t * q[:, 2:3] - q[:, 0:1] * s * q[:, 1:2])
    if final_is:
        ds = ds * q[:, 1:2]
    return stats, loss, ds.astype(F32)


# ================================================================================================ federated BCE
BCE_K = (1, 3, 5, 257)
BCE_NS = (1, 63, 64, 65, 100)
# name -> (K, ns, ldz, ldd, zero logits)
BCE_CASES = {}
for _iK, _K in enumerate(BCE_K):
    for _ns in BCE_NS:
        for _zero in (False, True):
            BCE_CASES[f"{'zero' if _zero else 'seeded'}-K{_K}-ns{_ns}"] = (_K, _ns, _ns + (3, 1, 7, 5)[_iK], _ns + (5, 2, 8, 3)[_iK], _zero)
BCE_UPSTREAM = 0.5


def bce_case(name):
    """-> dict(logits fp32 [K, ldz] (NaN in the padding), tgt int32 [K] (-1, 0, ns - 1, then seeded; K = 1: one of them), temp, weight and bce_ref's
    outputs).  Seeded logits reach |z| = 60.  Zero cases: temp 16, weight K / 8, so coef = 1 / 8 exactly."""
    K, ns, ldz, ldd, zero = BCE_CASES[name]
    rng = np.random.default_rng(11000 + 10 * K + ns)
    temp, weight = (16.0, K / 8.0) if zero else (14.3, 1.3)
    logits = np.full((K, ldz), np.nan, F32)
    logits[:, :ns] = 0 if zero else rng.uniform(-60 / 14.3, 60 / 14.3, (K, ns)).astype(F32)
    tgt = rng.integers(-1, ns, K).astype(np.int32)
    if K == 1:                                                    # the single row's target changes with ns: -1, 0, ns - 1, -1, 0
        tgt[0] = (-1, 0, ns - 1)[BCE_NS.index(ns) % 3]
    for k, v in enumerate((-1, 0, ns - 1)[:K if K >= 3 else 0]):
        tgt[(k + ns) % K] = v
    c = dict(K=K, ns=ns, ldz=ldz, ldd=ldd, zero=zero, logits=logits, tgt=tgt, temp=temp, weight=weight)
    c.update(bce_ref(logits[:, :ns], tgt, ldd, temp, weight, zero))
    return c


def bce_ref(logits, tgt, ldd, temp, weight, exact_dz=False, shift=0):
    """shift: the target column moved by that many columns (planted)."""
    K, ns = logits.shape
    tp, w = float(F32(temp)), float(F32(weight))
    Z = logits.astype(F64) * tp
    t = (np.arange(ns)[None, :] == (tgt[:, None] + shift)) & (tgt[:, None] >= 0)
    az = np.abs(Z)
    a = np.maximum(Z, 0) - np.where(t, Z, 0)
    L = np.log1p(np.exp(-az))
    TERM = a + L
    eterm = U * az * (a != 0) + (4 * az + 4) * U * L + 2 * U * (np.abs(a) + L)
    ROW = TERM.sum(1)
    row_b = eterm.sum(1) + ns * U * ROW + ns * FLOOR
    LOSS = w * ROW.sum() / K
    loss_b = w * (row_b.sum() + K * U * ROW.sum()) / K + 3 * U * abs(LOSS)
    coef = float(F32(weight) / F32(K))
    SIG, NSIG = _sig(Z)
    dsig = SIG * NSIG * (4 * az + 2) * U + 3 * U * SIG
    D = np.where(t, -NSIG, SIG)                                            # sigmoid - 1 without cancellation
    out = dict(row=ROW, row_b=row_b, loss=LOSS, loss_b=loss_b, coef=coef)
    for key, up in (("dz", 1.0), ("dz_up", BCE_UPSTREAM)):
        DZ = np.zeros((K, ldd))
        DZ[:, :ns] = coef * up * tp * D
        b = np.zeros((K, ldd))
        b[:, :ns] = abs(coef * up * tp) * (dsig + U * np.abs(D)) + 4 * U * np.abs(DZ[:, :ns]) + _half(DZ[:, :ns]) + FLOOR
        if exact_dz:
            assert np.array_equal(bf16_round64(DZ), DZ), "the zero-logit gradient is not a bf16 number"
            b[:] = 0
        out[key], out[key + "_b"] = DZ, b
    return out


def bce_restated(logits, tgt, ldd, temp, weight, upstream=None):
    """fp32 restatement -> (rowloss, loss, dz bf16 values [K, ldd])."""
    K, ns = logits.shape
    z = logits * F32(temp)
    t = (np.arange(ns)[None, :] == tgt[:, None])
    with np.errstate(all="ignore"):
        term = (np.maximum(z, F32(0)) - np.where(t, z, F32(0))) + np.log1p(_exp32(-np.abs(z))).astype(F32)
        row = term.sum(1, dtype=F32)
        loss = F32(weight) * row.sum(dtype=F32) / F32(K)
        coef = F32(weight) / F32(K) * (F32(1) if upstream is None else F32(upstream))
        v = coef * F32(temp) * (F32(1) / (F32(1) + _exp32(-z)) - t.astype(F32))
    dz = np.zeros((K, ldd))
    dz[:, :ns] = bf16_to_f32(rne_bits(v.astype(F32)))
    return row, loss, dz
