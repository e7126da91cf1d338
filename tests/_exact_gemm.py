"""TEST INFRASTRUCTURE -- GEMM tests on exactly representable operands.

If A, B, bias, residual, ln_mean, ln_rstd and ln_colsum hold small integers or powers of two and every partial sum, counted in units of
the smallest step `q` that any term can have, stays below 2^24, then fp32 accumulation is exact IN ANY ORDER: whatever the schedule, tile
shape, split count or K-slice order, there is one correct fp32 result, and it is known from float64 / integer arithmetic.  Every linear
epilogue must reproduce it bit for bit and every bf16 output must be its round-to-nearest-even image, ties included.

This module holds the seeded operand generators, the reference (float64, never through the code under test; it asserts its own 2^24
precondition and raises ExactnessError when a case violates it -- that is a bug of the test, not of a kernel), the expected outputs, the
shapes / schedules the GPU module runs, and the localising comparator.  tests/test_exact_gemm_cpu.py checks all of it without a GPU.
"""
from __future__ import annotations

import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TWO24 = float(1 << 24)
from test_gpu_ops import _LOG as LOG          # the metrics file that check() of the per-kernel tests appends to

# flags of cs_gemm_nt: heuristic, register staging, forced 128x128 / 256x128 / 256x256 (+ register staging), split rings (+ register
# staging, + burst DMA), persistent, streaming (+ slab epilogue) -- every reachable schedule (bits 4-7: 1, 2, 3, 7, 9, 11)
FLAGS = [0, 1, 0x10, 0x20, 0x30, 0x31, 0x70, 0x71, 0x8070, 0x90, 0xB0, 0x10B0]
TILE_OF_FLAGS = {0x10: (128, 128), 0x20: (256, 128)}         # everything else runs 256x256 tiles (the heuristic may pick a smaller one)

M_VALUES = [1, 7, 127, 128, 129, 191, 192, 193, 255, 256, 257, 449]
N_VALUES = [4, 12, 60, 64, 68, 124, 132, 252, 256, 260, 516]
K_VALUES = [64, 128, 192, 256, 448]                          # 1, 2, 3, 4, 7 K tiles: fewer than the ring stages, odd, more than the stages


def m_class(M):
    """Against the smallest row tile (128): below one tile, exactly one, one plus a fragment, several."""
    return 0 if M < 128 else 1 if M == 128 else 2 if M < 256 else 3


def n_class(N):
    """Against a wave's 64 output columns (also the width of a statistics slice)."""
    return 0 if N < 64 else 1 if N == 64 else 2 if N < 128 else 3


# The fixed selection: every value of M_VALUES / N_VALUES / K_VALUES and every (M class, N class) pair at least once
# (test_exact_gemm_cpu.py::test_the_selection_covers_every_value_and_every_pair_of_edge_classes).
TRIPLES = [
    (1, 4, 64), (7, 12, 192), (127, 60, 448), (7, 64, 128), (1, 68, 256), (127, 124, 64), (1, 516, 128), (7, 132, 448), (127, 256, 192),
    (128, 4, 256), (128, 64, 64), (128, 124, 192), (128, 260, 448),
    (129, 12, 128), (255, 60, 64), (191, 64, 448), (192, 68, 192), (193, 124, 256),
    (129, 252, 64), (191, 256, 128), (192, 132, 256), (193, 516, 64), (255, 260, 192),
    (256, 4, 448), (449, 60, 128), (257, 64, 256), (256, 68, 128), (449, 124, 448),
    (256, 256, 64), (257, 132, 192), (449, 516, 256), (257, 252, 128),
]
# cs_gemm_nt_ln_split and cs_gemm_nt_f8 need N % 32 == 0: the M edges against N below / at / past one wave's columns and several tiles
TRIPLES_N32 = [(1, 32, 64), (127, 64, 192), (128, 96, 128), (129, 256, 448), (192, 288, 64), (257, 64, 256), (449, 96, 128), (255, 32, 448),
               (7, 288, 256), (256, 256, 192), (193, 64, 128), (191, 96, 64)]
F8_SHAPES = [(1, 32, 128), (127, 64, 256), (128, 96, 384), (129, 256, 128), (192, 288, 256), (257, 64, 384), (449, 96, 128), (255, 32, 256),
             (7, 288, 384), (256, 256, 128), (193, 64, 256), (191, 96, 384)]
WGRAD_SHAPES = [(128, 64, 64), (300, 192, 128), (257, 260, 192), (64, 132, 832), (256, 256, 832), (129, 4, 128)]      # (M, N, contraction): 1, 2, 3, 13 K tiles
WGRAD_TN_SHAPES = [(1, 8, 264), (7, 24, 248), (63, 248, 8), (64, 256, 256), (65, 264, 24), (200, 256, 264), (200, 8, 8), (64, 24, 256),
                   (65, 248, 248), (7, 264, 256), (63, 256, 24), (1, 248, 264)]                                        # (tokens, N, K)
BM192_SHAPES = [(192, 64, 128), (193, 288, 64), (383, 96, 192), (385, 64, 448), (449, 288, 256)]


class ExactnessError(AssertionError):
    """The case does not meet the precondition under which fp32 arithmetic is order independent: a bug of the test."""


def _require(cond, msg):
    if not cond:
        raise ExactnessError(msg)


# ------------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lim, seed, zeros=1.0 / 3.0):
    """Integers in [-lim, lim], both signs, about `zeros` of them zero (float64)."""
    g = _gen(seed)
    mag = torch.randint(1, lim + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    keep = (torch.rand(shape, generator=g) >= zeros).double()
    return mag * sign * keep + 0.0                  # + 0.0: no negative zeros


def int_bf16(shape, lim, seed, step=1.0):
    """bf16 multiples of `step` (a power of two) in [-lim * step, lim * step], about one third zeros: exactly representable."""
    t = (_ints(shape, lim, seed) * step).to(BF)
    return t


def int_f32(shape, lim, seed, step=1.0):
    """fp32 multiples of `step` in [-lim * step, lim * step], no forced zeros (bias, residual, ln_mean, ln_colsum)."""
    return (_ints(shape, lim, seed, zeros=0.0) * step).float()


def rstd_f32(n, seed):
    """ln_rstd in {0.5, 1, 2}."""
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=_gen(seed))].contiguous()


def pow2_f32(n, seed, lo=-1, hi=1):
    """Power-of-two scales 2^lo .. 2^hi (fp8 row / column scales)."""
    return (2.0 ** torch.randint(lo, hi + 1, (n,), generator=_gen(seed)).double()).float()


def e4m3_codes(shape, lim, seed):
    """uint8 e4m3 codes of integers in [-lim, lim] (lim <= 16: exactly representable in e4m3)."""
    v = _ints(shape, lim, seed).float()
    q = v.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), v)
    return q.view(torch.uint8)


def fp8_quant_case(M, K, seed):
    """Rows for cs_quant_rows_fp8 whose amax is 448 * 2^k: the scale 2^k is exact and the codes are the integers themselves.  Returns
    (x bf16 [M, K], codes uint8 [M, K rounded up to 128] with zero padding, scale fp32 [M])."""
    c = _ints((M, K), 3, seed).float()
    c[torch.arange(M), torch.randint(0, K, (M,), generator=_gen(seed + 1))] = 448.0
    c[0, 0] = -448.0                                              # a negative amax too
    scale = pow2_f32(M, seed + 2, -3, 3)
    x = (c * scale[:, None]).to(BF)
    assert torch.equal(x.float(), c * scale[:, None])
    codes = torch.zeros(M, (K + 127) // 128 * 128, dtype=torch.uint8)
    codes[:, :K] = c.to(torch.float8_e4m3fn).view(torch.uint8)
    return x, codes, scale


def operands(M, N, K, seed, profile="wide", rows_b=None, bias_hi=7):
    """The operands of one case.  Profiles:
      wide   A in [-3, 3], B in [-2, 2], bias / residual integers in [-1000, 1000]: most bf16 outputs lie above 256 and need rounding, the odd
             ones in (256, 512) are exact ties;
      stats  the same with bias / residual in [-150, 150]: the 64-column sums of squares of the outputs stay below 2^24 steps;
      act    B in multiples of 2^-4 / 2^-5, bias in multiples of 1/8 in [-1, bias_hi]: pre-activations within [-16, 16] with many distinct values,
             few of them below -3.5 where 1 + erf(x / sqrt 2) cancels.
    rows_b: rows of B (default N; 2 N for the SwiGLU epilogue)."""
    nb = rows_b or N
    if profile in ("act", "act_ln"):
        step = (2.0 ** -4 if K <= 128 else 2.0 ** -5) * (0.5 if profile == "act_ln" else 1.0)
        A, B = int_bf16((M, K), 2 if profile == "act_ln" else 3, seed), int_bf16((nb, K), 2, seed + 1, step)
        bias = (torch.randint(-8, 8 * bias_hi + 1, (nb,), generator=_gen(seed + 2)).double() / 8).float()
        res = int_f32((M, N), 8, seed + 3, 0.125)
    else:
        lim = 1000 if profile == "wide" else 150
        A, B = int_bf16((M, K), 3, seed), int_bf16((nb, K), 2, seed + 1)
        bias, res = int_f32((nb,), lim, seed + 2), int_f32((M, N), lim, seed + 3)
    return dict(A=A, B=B, bias=bias, res=res, mean=int_f32((M,), 2, seed + 4), rstd=rstd_f32(M, seed + 5), colsum=int_f32((nb,), 8, seed + 6))


def act_ln_operands(M, N, K, seed, rows_b, bias_hi=7):
    """The act profile with a fold that keeps the pre-activations inside [-16, 16] under rstd = 2: A in [-2, 2], B in steps half as large,
    mean in [-1, 1], column sums in multiples of 1/8 in [-1, 1]."""
    a = operands(M, N, K, seed=seed, profile="act_ln", rows_b=rows_b, bias_hi=bias_hi)
    a["mean"], a["colsum"] = int_f32((M,), 1, seed + 7), int_f32((rows_b,), 8, seed + 8, 0.125)
    return a


# ------------------------------------------------------------------------------------------------ reference
def quantum(*tensors):
    """The largest power of two 2^-s (s = 0 .. 16) of which every entry of every tensor is a multiple."""
    for s in range(17):
        q = 2.0 ** -s
        if all(torch.equal(t.double() / q, (t.double() / q).round()) for t in tensors if t is not None):
            return q
    raise ExactnessError("operands are not multiples of 2^-16")


def _f64(t):
    if t is None:
        return None
    if t.dtype == torch.uint8:
        t = t.view(torch.float8_e4m3fn)
    return t.float().double() if t.dtype in (torch.float8_e4m3fn, BF) else t.double()


def exact_gemm(A, B, bias=None, extra=None, ln=None, scales=None):
    """float64 value of   extra + [rstd * ((row_scale * col_scale) A.B^T - mean * colsum)] + bias   and the proof that fp32 computes the
    same in any order: with q the common step of all terms, max over the elements of  (sum_k |a||b| (+ |mean||colsum|) scaled) + |bias| +
    |extra|  < 2^24 q.  Every partial sum of every summation order is then a multiple of q below 2^24 q, i.e. an fp32 number."""
    a, b = _f64(A), _f64(B)
    acc, bound, q = a @ b.T, a.abs() @ b.abs().T, quantum(a) * quantum(b)
    if scales is not None:
        rs, cs = _f64(scales[0]), _f64(scales[1])
        f = rs[:, None] * cs[None, :]
        acc, bound, q = acc * f, bound * f.abs(), q * quantum(rs) * quantum(cs)
    if ln is not None:
        mean, rstd, colsum = (_f64(t) for t in ln)
        acc = rstd[:, None] * (acc - mean[:, None] * colsum[None, :])
        bound = rstd.abs()[:, None] * (bound + mean.abs()[:, None] * colsum.abs()[None, :])
        q = min(q, quantum(mean) * quantum(colsum)) * quantum(rstd)
    if bias is not None:
        acc, bound, q = acc + _f64(bias), bound + _f64(bias).abs(), min(q, quantum(bias))
    if extra is not None:
        acc, bound, q = acc + _f64(extra), bound + _f64(extra).abs(), min(q, quantum(extra))
    worst = float(bound.max()) / q
    _require(worst < TWO24, f"sum of magnitudes {worst:.3e} steps of {q} >= 2^24: fp32 is not order independent here")
    _require(torch.equal(acc.float().double(), acc), "the exact value is not an fp32 number")
    return acc


def exact_stats(v, width):
    """stats_part of the fp32 outputs v (float64 [M, N]): per `width`-column slice (sum, sum of squares) [S, M, 2] -- exact in fp32 in any
    order because sum |v| and sum v^2, in steps of q resp. q^2, stay below 2^24."""
    M, N = v.shape
    S = (N + width - 1) // width
    q = quantum(v)
    out = torch.zeros(S, M, 2, dtype=F64)
    for s in range(S):
        blk = v[:, width * s:width * (s + 1)]
        _require(float(blk.abs().sum(-1).max()) / q < TWO24 and float((blk * blk).sum(-1).max()) / (q * q) < TWO24,
                 f"statistics slice {s}: sums of |v| / v^2 in steps of {q} / {q * q} reach 2^24")
        out[s, :, 0], out[s, :, 1] = blk.sum(-1), (blk * blk).sum(-1)
    _require(torch.equal(out.float().double(), out), "the exact statistics are not fp32 numbers")
    return out.float()


def want_f32(v):
    return v.float()


def want_bf16(v):
    """bf16 of the exact fp32 value: torch's conversion is round-to-nearest-even."""
    return v.float().to(BF)


def rounding_census(v):
    """(ties, share of rounded elements) of the bf16 image of the exact values v: a tie has the dropped 16 bits equal to 0x8000."""
    low = v.float().contiguous().view(torch.int32) & 0xFFFF
    return int((low == 0x8000).sum()), float((low != 0).double().mean())


CENSUS_MIN_ELEMENTS = 1024        # a case of fewer elements cannot be asked for 10 ties (they occur at a rate of ~10 %); it is still compared


def assert_rounding_is_tested(name, v):
    """A bf16 case claims to test round-to-nearest-even: it must hold >= 10 exact ties and >= 1 % rounded elements."""
    if v.numel() < CENSUS_MIN_ELEMENTS:
        return
    ties, share = rounding_census(v)
    _require(ties >= 10 and share >= 0.01, f"{name}: {ties} ties, {share:.2%} rounded elements -- the rounding claim is not tested")


# ------------------------------------------------------------------------------------------------ non-linear epilogues
def act64(pre, epi, group=0):
    """float64 value of the non-linear epilogues on the exact pre-activation: 3 silu(x1) * x2, 7 GELU (erf), 8 QuickGELU."""
    if epi == 3:
        x1, x2 = pre[:, :group], pre[:, group:]
        return x1 * torch.sigmoid(x1) * x2
    if epi == 7:
        return 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    assert epi == 8
    return pre * torch.sigmoid(1.702 * pre)


def act32(pre, epi, group=0):
    """The same three formulas in plain fp32 (what a correct kernel computes, up to its own choice of exp / erf)."""
    p = pre.float()
    if epi == 3:
        x1, x2 = p[:, :group], p[:, group:]
        return x1 / (1.0 + torch.exp(-x1)) * x2
    if epi == 7:
        return 0.5 * p * (1.0 + torch.erf(p * 0.70710678118654752))
    return p / (1.0 + torch.exp(-1.702 * p))


def bf16_spacing(w):
    """Distance between neighbouring bf16 numbers at |w| (float64 tensor); 0 at w == 0."""
    _, e = torch.frexp(w.abs().clamp_min(2.0 ** -126))
    return torch.where(w == 0, torch.zeros_like(w), torch.ldexp(torch.ones_like(w), e - 8))


ACT_MAX_SHARE = 0.01


def flip_margin(w):
    """Distance of the float64 values w to the nearest point where their bf16 rounding changes (the midpoints between neighbouring bf16
    numbers; below a power of two the neighbours are half as far apart)."""
    b = w.float().to(BF).double()
    s = bf16_spacing(b)
    m, _ = torch.frexp(b.abs())
    below_pow2 = (m == 0.5) & (w.abs() < b.abs())
    half = torch.where(below_pow2, s / 4, s / 2)
    return torch.where(w == 0, torch.full_like(w, float("inf")), torch.where(b == 0, w.abs(), half - (w - b).abs()))      # act(0) = 0 in any precision


def act_case(M, N, K, seed, epi, fold=False):
    """Operands and exact pre-activations of one non-linear case: profile `act` (behind a folded LayerNorm with fold=True: key "pre_ln").
    A case of fewer than 100 elements cannot spend any of the 1 % of elements that may differ from bf16(float64 activation), so its seed
    advances (by 1000) until every element is robust: farther from a change of its bf16 rounding than any fp32 evaluation errs --
    2^-17 |want| (exp2 and rcp at 1 ulp, the 27-fold amplified rounding of the exponent's argument, a few roundings) + 2^-22 |pre| (erf at
    2 ulp under the cancellation of 1 + erf)."""
    nb = 2 * N if epi == 3 else N
    for attempt in range(64):
        hi = 7 if M * N >= 100 else 3             # small cases stay below ~4.4, where a pre-activation on a bf16 tie meets GELU(x) = x - tiny
        a = act_ln_operands(M, N, K, seed + 1000 * attempt, nb, hi) if fold else operands(M, N, K, seed + 1000 * attempt, "act", nb, hi)
        a["pre"] = exact_gemm(a["A"], a["B"], a["bias"])
        pres = [a["pre"]]
        if fold:
            a["pre_ln"] = exact_gemm(a["A"], a["B"], a["bias"], ln=(a["mean"], a["rstd"], a["colsum"]))
            pres.append(a["pre_ln"])
        if M * N >= 100:
            return a
        ok = True
        for pre in pres:
            w = act64(pre, epi, N)
            x = torch.maximum(pre[:, :N].abs(), pre[:, N:].abs()) if epi == 3 else pre.abs()
            ok = ok and bool((flip_margin(w) > 2.0 ** -17 * w.abs() + 2.0 ** -22 * x).all())
        if ok:
            return a
    raise ExactnessError(f"no robust small case found for [{M},{N},{K}] epilogue {epi}")


def activation_mismatch(name, got, pre, epi, group=0):
    """Per-element check of a non-linear epilogue; None when it holds, else the message.  The pre-activation is exact, so what is left is
    the activation's fp32 arithmetic and one rounding:  |got - want64| <= one bf16 spacing at |want64| + 8 * 2^-23 * max |pre|  (the second
    term covers the cancellation in 1 + erf(x) for negative x), and at most 1 % of the elements may differ from bf16(want64) at all.
    Returns (message or None, share of differing elements)."""
    _require(float(pre.abs().max()) <= 16.0, f"{name}: pre-activations leave [-16, 16]")
    want = act64(pre, epi, group)
    g = got.detach().cpu()
    if not torch.isfinite(g.float()).all():
        bad = ~torch.isfinite(g.float())
        r, c = (int(x) for x in bad.nonzero()[0])
        return f"{name}: {int(bad.sum())} non-finite outputs (NaN prefill = not written), first at ({r}, {c})", 1.0
    tol = bf16_spacing(want) + 8 * 2.0 ** -23 * float(pre.abs().max())
    err = (g.double() - want).abs()
    share = float((g.view(torch.int16) != want.float().to(BF).view(torch.int16)).double().mean())
    over = err > tol
    if over.any():
        r, c = (int(x) for x in over.nonzero()[0])
        return (f"{name}: {int(over.sum())} elements outside the bound, first ({r}, {c}) got {float(g[r, c])!r} want {float(want[r, c])!r} "
                f"(pre {float(pre[r, c])!r}, bound {float(tol[r, c]):.3e})"), share
    if share > ACT_MAX_SHARE:
        return f"{name}: {share:.2%} of the elements differ from bf16(float64 activation), more than {ACT_MAX_SHARE:.0%}", share
    return None, share


# ------------------------------------------------------------------------------------------------ comparator
def _int_view(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def bits_mismatch(name, got, want, tile=(256, 256)):
    """None when got and want agree in every bit, else a message that localises the fault: number of wrong elements, the first few (row,
    col, got, want), the (row // bm, col // bn) tiles that contain errors, whether they lie only in the last partial row / column tile, and
    whether a wrong element is untouched NaN prefill ("tile not written")."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    gi, wi = _int_view(got), _int_view(want)
    if torch.equal(gi, wi):
        return None
    if gi.dim() == 1:
        gi, wi, got, want = gi[None], wi[None], got[None], want[None]
    gi, wi = gi.reshape(-1, gi.shape[-1]), wi.reshape(-1, wi.shape[-1])
    g2, w2 = got.detach().cpu().reshape(gi.shape), want.detach().cpu().reshape(wi.shape)
    bad = gi != wi
    idx = bad.nonzero()
    bm, bn = tile
    R, C = gi.shape
    tiles = sorted({(int(r) // bm, int(c) // bn) for r, c in idx.tolist()})
    first = ", ".join(f"({int(r)}, {int(c)}): got {float(g2[r, c])!r} want {float(w2[r, c])!r}" for r, c in idx[:4].tolist())
    last_tm, last_tn = (R - 1) // bm, (C - 1) // bn
    where = []
    if R % bm and all(t[0] == last_tm for t in tiles):
        where.append("only in the last partial row tile")
    if C % bn and all(t[1] == last_tn for t in tiles):
        where.append("only in the last partial column tile")
    unwritten = int((bad & torch.isnan(g2.float()) & ~torch.isnan(w2.float())).sum()) if g2.is_floating_point() else 0
    msg = (f"{name}: {int(bad.sum())} of {bad.numel()} elements differ in bits; first {first}; tiles {bm}x{bn} with errors: "
           f"{tiles[:12]}{' ...' if len(tiles) > 12 else ''}; {', '.join(where) if where else 'not confined to the ragged edge tiles'}")
    if unwritten:
        msg += f"; {unwritten} of them are untouched NaN prefill: tile not written"
    return msg


def log_line(line):
    try:
        LOG.parent.mkdir(exist_ok=True)
        with open(LOG, "a") as f:
            f.write(line + "\n")
    except OSError:                 # a read-only tree: the message is still raised
        pass


def assert_bits_equal(name, got, want, tile=(256, 256)):
    msg = bits_mismatch(name, got, want, tile)
    if msg is not None:
        log_line("EXACT MISMATCH " + msg)
        raise AssertionError(msg)


class Failures:
    """Collects every failing combination of a test's inner loop (schedules x epilogues) before asserting."""

    def __init__(self):
        self.msgs = []

    def bits(self, name, got, want, tile=(256, 256)):
        msg = bits_mismatch(name, got, want, tile)
        if msg is not None:
            log_line("EXACT MISMATCH " + msg)
            self.msgs.append(msg)
        return msg is None

    def add(self, msg):
        if msg is not None:
            log_line("EXACT MISMATCH " + msg)
            self.msgs.append(msg)

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} failing combinations:\n" + "\n".join(self.msgs[:20])


# ------------------------------------------------------------------------------------------------ expected outputs of the epilogues
def patch_rows(M, group):
    """Output row of every GEMM row under the patch-embed epilogue (5): row + row // group + 1; rows img * (group + 1) stay untouched."""
    r = torch.arange(M)
    return r + r // group + 1, r % group + 1


def patch_group(M):
    """A tokens-per-image count that divides no row tile (128 / 192 / 256)."""
    return 37 if M > 37 else 5


def split_chain(o, M, N):
    """The exact fp32 residual stream after each of the three chained folded GEMMs of the split-stream test (x += rstd (A.B^T - mean colsum)
    + bias, the same operands three times), float64."""
    xs, x = [], _f64(o["res"])
    for _ in range(3):
        x = exact_gemm(o["A"], o["B"], o["bias"], x, ln=(o["mean"], o["rstd"], o["colsum"]))
        xs.append(x)
    return xs

