"""Inputs, fp64 references and derived error bounds for the LayerNorm / row-statistics family (tests/test_ln_cond_cpu.py,
tests/test_gpu_ln_cond.py; figures in profiles/ln_conditioning.md).

The op-level tests of tests/test_gpu_ops.py draw `randn * s + small offset`: every row of a launch has the same statistics, so a kernel
that hands one row's (mean, rstd) to another, or drops a term that only matters when |mean| >> sigma, stays under their whole-tensor
tolerance.  Here every row of one launch gets its own prescribed |mean| / sigma and scale, every check is per row or per element, and
every bound is derived from the number formats and the kernels' summation depths (u = 2^-24), never from what a kernel returned.

Imports without a GPU.  torch (CPU, float64 / float32) is the only dependency; the fp32 emulations perform one IEEE single operation
per statement, in the kernels' order.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24                         # unit round-off of fp32
RATIOS = (0.0, 1.0, 2.0, 5.0, 20.0, 100.0, 1000.0)
SCALES = (2.0 ** -10, 1.0, 2.0 ** 10, 1.0)       # period 4: coprime to the 7 ratios and to the every-third-row outliers; neighbours always differ
OUTLIER = 150.0
EPS = 1e-6
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

# activation Lipschitz constants (sup |f'|): GELU 1.129, SiLU 1.0998, QuickGELU x * sigmoid(1.702 x) 1.0998 -- rounded up
LIP = {"gelu": 1.13, "silu": 1.13, "qgelu": 1.1}


# ------------------------------------------------------------------------------------------------ inputs
def _stats64(x):
    x = x.double()
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, var


def _ulp_of_max(x, dtype):
    bits = 7 if dtype == BF else 23
    return 2.0 ** (torch.floor(torch.log2(x.abs().amax(-1).clamp_min(1e-300))) - bits)


def skewed_rows(M, C, seed, dtype, ratios=RATIOS, scales=SCALES, outliers=True):
    """[M, C] rows with prescribed, row-wise different statistics, and their descriptors.

    Row i: |mean| / sigma = ratios[i % len(ratios)], sign of the mean (-1)^i, sigma = scales[i % len(scales)]; with `outliers`, rows
    i % 3 == 2 carry three channels (first, middle, last column) at OUTLIER times the others before standardisation.  Each row is
    standardised exactly in fp64 (mean 0, biased variance 1), then x = scale * (sign * ratio + g * z) is rounded to `dtype`.
    Rounding changes sigma where the grid is coarse against it (bf16 at ratio >= 100: one ulp of the mean is 0.4 .. 4 sigma), so the
    gain g is iterated on the STORED values, and what is left is trimmed by moving the whole row a few ulps of its largest element
    towards zero (exactly representable: every element stays a multiple of its own ulp).  The descriptors are recomputed in fp64 from
    the values as stored -- those are the kernels' inputs:
      ratio0 (prescribed), ratio (achieved), scale, sign, outlier, mean, var, sigma, rstd (1 / sqrt(var + EPS))."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g, dtype=F64)
    idx = torch.arange(M)
    ratio0 = torch.tensor(ratios, dtype=F64)[idx % len(ratios)]
    scale = torch.tensor(scales, dtype=F64)[idx % len(scales)]
    sign = torch.where(idx % 2 == 0, 1.0, -1.0).double()
    out = (idx % 3 == 2) if outliers else torch.zeros(M, dtype=torch.bool)
    for c in (0, C // 2, C - 1):
        z[out, c] = OUTLIER * torch.sign(z[out, c]) * z[out, c].abs().clamp_min(0.5)      # never a near-zero draw: it would be no outlier
    for _ in range(2):                                              # twice: the second pass removes the first one's rounding
        z = z - z.mean(-1, keepdim=True)
        z = z / z.pow(2).mean(-1, keepdim=True).sqrt()

    def store(gain):
        return (scale[:, None] * (sign[:, None] * ratio0[:, None] + gain[:, None] * z)).to(dtype)

    def err_of(xs):
        mean, var = _stats64(xs)
        r = mean.abs() / var.sqrt()
        return torch.where(ratio0 > 0, (r / ratio0.clamp_min(1e-30) - 1).abs(), r), r

    gain = torch.ones(M, dtype=F64)
    best = store(gain)
    best_err, r = err_of(best)
    above, above_err = best.clone(), torch.where(r >= ratio0, best_err, torch.full_like(best_err, float("inf")))
    lo, hi = torch.full((M,), -4.0, dtype=F64), torch.full((M,), 4.0, dtype=F64)      # bisection on log2(gain): the ratio falls as it grows
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        xs = store(torch.where(ratio0 > 0, torch.exp2(mid), gain))
        e, r = err_of(xs)
        small = ~(r <= ratio0)                                       # sigma too small (or zero: r = inf / nan): raise the gain
        lo, hi = torch.where(small, mid, lo), torch.where(small, hi, mid)
        better = e < best_err
        best[better], best_err[better] = xs[better], e[better]
        better = (r >= ratio0) & (e < above_err)                     # the best candidate whose ratio is too large: the trim can lower it
        above[better], above_err[better] = xs[better], e[better]

    def trim(xs):
        """shift the row by j ulps of its largest element (j > 0: towards zero, always representable; j < 0 only where it round-trips)"""
        mean, var = _stats64(xs)
        q = _ulp_of_max(xs.double(), dtype)
        j = torch.where(ratio0 > 0, torch.round((mean.abs() - ratio0 * var.sqrt()) / q), torch.zeros_like(q))
        j = torch.nan_to_num(j, nan=0.0, posinf=0.0, neginf=0.0)
        cand64 = xs.double() - (torch.sign(mean) * j * q)[:, None]
        cand = cand64.to(dtype)
        exact = (cand.double() == cand64).all(-1)
        return cand, torch.where(exact, err_of(cand)[0], torch.full_like(q, float("inf")))

    for src in (best.clone(), above):
        cand, e = trim(src)
        take = e < best_err
        best[take], best_err[take] = cand[take], e[take]
    x = best.contiguous()
    mean, var = _stats64(x)
    desc = dict(ratio0=ratio0, scale=scale, sign=sign, outlier=out, mean=mean, var=var, sigma=var.sqrt(),
                ratio=mean.abs() / var.sqrt(), rstd=torch.rsqrt(var + EPS))
    return x, desc


def plain_rows(M, C, seed, dtype=F32):
    """What the whole-tensor tests of tests/test_gpu_ops.py draw: randn * 2 + 0.3 -- every row the same statistics."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, C, generator=g) * 2.0 + 0.3).to(dtype)


def describe(desc, i):
    return f"row {i} (ratio {float(desc['ratio0'][i]):g}, scale 2^{int(round(math.log2(float(desc['scale'][i]))))}" \
           f"{', outliers' if bool(desc['outlier'][i]) else ''})"


# ------------------------------------------------------------------------------------------------ fp64 references (of the stored operands)
def ln_ref64(x, gamma=None, beta=None, eps=EPS):
    """mean, rstd [M] and y [M, C] (None without gamma) of LayerNorm(eps, biased variance), all in fp64."""
    x = x.double()
    mean, var = _stats64(x)
    rstd = torch.rsqrt(var + eps)
    y = None if gamma is None else (x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return mean, rstd, y


def ln_bwd_ref64(dy, x, gamma, mean, rstd):
    """LayerNorm backward as the closed formula in fp64, from given (mean, rstd):  xh = (x - mean) rstd, gy = dy gamma,
    dx = rstd (gy - <gy> - xh <gy xh>); dgamma = sum_rows dy xh, dbeta = sum_rows dy.  Also returns sum_rows |dy xh| and sum_rows |dy|
    (the scales of the per-column bounds)."""
    x, dy, gamma, mean, rstd = x.double(), dy.double(), gamma.double(), mean.double(), rstd.double()
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = dy * gamma
    dx = rstd[:, None] * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0), (dy * xh).abs().sum(0), dy.abs().sum(0)


def slice_partials64(x, npp, P=None):
    """[P, M, 3] fp64: (sum, sum of squares, sum of |x|) of slice p = columns [p * npp, min((p + 1) * npp, C)); slices past C are NaN."""
    x = x.double()
    M, C = x.shape
    P = P if P is not None else (C + npp - 1) // npp
    part = torch.full((P, M, 3), float("nan"), dtype=F64)
    for p in range(P):
        blk = x[:, p * npp:(p + 1) * npp]
        if blk.shape[1] > 0:
            part[p, :, 0], part[p, :, 1], part[p, :, 2] = blk.sum(-1), (blk * blk).sum(-1), blk.abs().sum(-1)
    return part


def exact_partials(x, npp, P=None):
    """[P, M, 2] fp32: the fp64 slice sums rounded once to fp32 (what an ideal producer would write); slices past C are NaN."""
    return slice_partials64(x, npp, P)[:, :, :2].float().contiguous()


def folded_gemm_ref64(A, W, mean, rstd, colsum, bias, extra=None):
    """out64 = rstd (A.W^T - mean colsum) + bias (+ extra) in fp64 from the operands the kernel got (mean / rstd / colsum as given), and
    its per-element bound folded_gemm_bound (without the output-format term)."""
    A, W, mean, rstd, colsum = A.double(), W.double(), mean.double(), rstd.double(), colsum.double()
    K = A.shape[1]
    acc = A @ W.T
    absacc = A.abs() @ W.abs().T
    mc = mean[:, None] * colsum[None, :]
    out = rstd[:, None] * (acc - mc) + (bias.double() if bias is not None else 0.0)
    if extra is not None:
        out = out + extra.double()
    return out, folded_gemm_bound(K, rstd, absacc, mc, out)


# ------------------------------------------------------------------------------------------------ bounds
def bf16_half_ulp(y64):
    """Half an ulp of bf16 at y64: 2^(floor(log2 |y64|) - 8), between 2^-9 |y64| (upper end of a binade) and 2^-8 |y64| (lower end).
    "2^-9 |y64|" for every value would be violated by the correctly rounded exact result wherever the significand of y64 is below
    1.5 (tests/test_ln_cond_cpu.py shows it on the reference ops), so the bf16 term of every bound here is the exact half ulp: the
    smallest term any correct bf16 output satisfies."""
    a = y64.double().abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 8), torch.zeros_like(a))


def ln_mean_bound(desc):
    """Two-pass row kernels (ln_fwd_kernel): |mean - mean64| <= 64 u (1 + r) sigma.
    A lane adds at most 48 values (12 vector groups of 4, as (a + b) + (c + d) per group), six xor-shuffle steps follow, then one
    division: every partial sum is bounded by sum |x| <= C (|mean| + sigma) (Cauchy-Schwarz), so the absolute error of the row sum is at
    most (48 + 6) u C (1 + r) sigma, of the mean (54 + 1) u (1 + r) sigma; 64 leaves room for the second-order terms."""
    return 64 * U * (1 + desc["ratio"]) * desc["sigma"]


def ln_rstd_bound(desc=None):
    """Two-pass row kernels: |rstd / rstd64 - 1| <= 64 u + 4 u, whatever the ratio (up to 1000).
    The second pass sums d^2 with d = x - mean_f32: non-negative terms, depth <= 48 + 6 (+ 2 per term for the subtraction and the square),
    so the relative error of the sum is <= 64 u; half of it reaches rstd, the other half covers the mean's own error delta, which enters
    as delta^2 / var <= (64 u (1 + r))^2 = 1.5e-5 worst case at r = 1000 but ~ (a few u (1 + r))^2 for rounding errors that do not all
    align.  4 u: the division by C, + eps and the hardware rsqrt.  A one-pass E[x^2] - mean^2 errs by ~ u r^2 and breaks this at r >= 20."""
    return 68 * U


def ln_y_bound(x, gamma, beta, desc, y64, out_dtype):
    """Per element: fp32 term = |gamma| rstd64 mean_bound  +  |gamma xh64| rstd_bound  +  4 u (|gamma xh64| + |y64|)
    (the four roundings of (x - mean) * rstd * gamma + beta, each relative to a quantity <= |gamma xh| + |y|); bf16 outputs add the
    half ulp of y64 (bf16_half_ulp)."""
    gxh = ((x.double() - desc["mean"][:, None]) * desc["rstd"][:, None] * gamma.double()).abs()
    t = gamma.double().abs()[None, :] * (desc["rstd"] * ln_mean_bound(desc))[:, None] + gxh * ln_rstd_bound() + 4 * U * (gxh + y64.abs())
    return t + (bf16_half_ulp(y64) if out_dtype == BF else 0.0)


def finalize_rstd_bound(P, desc):
    """cs_ln_stats_finalize on exact partials: |rstd / rstd64 - 1| <= 0.5 (P + 16) u (1 + r^2) + 4 u.
    m2 = q + (b - s mean) with q = sum_p (Q_p - S_p^2 / n), b = sum_p S_p^2 / n: every term is bounded by sum x^2 = C var (1 + r^2), each
    input carries one rounding (u), each slice adds 3 operations on its t and 1 per running sum, and P sequential additions follow;
    P + 16 covers the depth for every P >= 1.  rstd takes half the relative error of the variance; 4 u as for the row kernels.  BOTH the
    within-slice term Q_p - S_p^2 / n and the between-slice term b - s mean cancel like 1 + r^2."""
    return 0.5 * (P + 16) * U * (1 + desc["ratio"] ** 2) + 4 * U


def finalize_mean_bound(P, desc, eps=EPS):
    """|mean - mean64| <= (P + 4) u sqrt(1 + r^2) sqrt(var + eps): P sequential additions of slice sums bounded by sum |x| <=
    C sqrt(var + mean^2), one input rounding each, one division."""
    return (P + 4) * U * torch.sqrt(1 + desc["ratio"] ** 2) * torch.sqrt(desc["var"] + eps)


def partial_bounds(part64, n):
    """Producers' partials against the fp64 sums (S, Q, sum |x|) of the kernel's own output slice of n columns:
    |s - S| <= n u sum |x|, |q - Q| <= n u Q (n - 1 additions in any order, one rounding per square)."""
    return n * U * part64[..., 2], n * U * part64[..., 1]


def folded_gemm_bound(K, rstd, absacc, mean_colsum, out64, out_dtype=F32):
    """Per element: |out - out64| <= rstd (K u sum_k |a_k w_nk| + 2 u |mean colsum_n|) + u |out64|  (+ bf16_half_ulp(out64) for bf16 outputs).
    The MFMA accumulates K exact bf16 products in fp32 in some order (K u sum |a w|); -rstd * mean and its product with the column sum
    round once each (2 u); the last operation rounds the result (u |out64|)."""
    b = rstd.double()[:, None] * (K * U * absacc + 2 * U * mean_colsum.abs()) + U * out64.abs()
    return b + (bf16_half_ulp(out64) if out_dtype == BF else 0.0)


def through_activation(bound_pre, x64, act64, name):
    """Bound of a bf16 activation output f(x) from the bound of its fp32 argument x: Lipschitz constant times the argument's bound;
    the activation's own fp32 evaluation: 4 u |x| absolute (0.5 x (1 + erf) and x / (1 + exp) lose the relative accuracy of the
    bracket where it cancels, at 1 .. 2 ulp of erf / exp / rcp) + 64 u |f| (the exponent's argument is rounded before exp2:
    relative error <= |arg| u ln 2 with |arg| <= 88 before exp2 saturates); and the bf16 rounding of the result."""
    return LIP[name] * bound_pre + 4 * U * x64.abs() + 64 * U * act64.abs() + bf16_half_ulp(act64)


def check_rows(err, bound, desc, what):
    """(worst error / bound, message or None).  err, bound: [M] or [M, N] with the rows of desc; desc = None: a vector over columns.
    A NaN or inf anywhere in err counts as a violation."""
    err, bound = err.double(), bound.double()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    per_row = ratio if ratio.dim() == 1 else ratio.amax(-1)
    worst = int(per_row.argmax())
    bad = int((per_row > 1).sum())
    msg = None
    if bad and desc is None:
        msg = f"{what}: {bad} columns outside the bound; worst column {worst}: error / bound = {float(per_row[worst]):.3g}"
    elif bad:
        msg = f"{what}: {bad} rows outside the bound; worst {describe(desc, worst)}: error / bound = {float(per_row[worst]):.3g}"
    return float(per_row[worst]), msg


# ------------------------------------------------------------------------------------------------ fp32 emulations of the kernels' formulas
def _wave_sum(s):
    """[M, 64] fp32 -> [M]: the xor-shuffle butterfly of wave_sum (offsets 32 .. 1), every lane ends with the same sum."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def emul_ln_two_pass(x, eps=EPS, one_pass=False):
    """ln_fwd_kernel in fp32: lane l of the row's wave holds vector group g = columns (g * 64 + l) * 4 .. + 3; first pass
    s += (v0 + v1) + (v2 + v3) per group, butterfly, / C; second pass q += d * d element by element, butterfly, rsqrt(q / C + eps).
    one_pass (the planted defect): sum and sum of squares in one sweep, var = E[x^2] - mean^2."""
    M, C = x.shape
    ng = (C + 255) // 256
    v = torch.zeros(M, ng * 256, dtype=F32)
    v[:, :C] = x.float()
    live = (torch.arange(ng * 256) < C).view(ng, 64, 4)
    v = v.view(M, ng, 64, 4)
    s = torch.zeros(M, 64, dtype=F32)
    for g in range(ng):
        s = s + ((v[:, g, :, 0] + v[:, g, :, 1]) + (v[:, g, :, 2] + v[:, g, :, 3]))
    Cf = torch.tensor(float(C), dtype=F32)
    mean = _wave_sum(s) / Cf
    q = torch.zeros(M, 64, dtype=F32)
    for g in range(ng):
        for i in range(4):
            d = v[:, g, :, i] if one_pass else v[:, g, :, i] - mean[:, None]
            q = q + torch.where(live[g, :, i], d * d, torch.zeros((), dtype=F32))
    var = _wave_sum(q) / Cf
    if one_pass:
        var = (var - mean * mean).clamp_min(0)
    return mean, torch.rsqrt(var + torch.tensor(eps, dtype=F32))


def emul_finalize(part, npp, C, eps=EPS, shape="8+tail", defect=None):
    """ln_stats_finalize_kernel ("8+tail": batches of 8 slices, then a scalar tail that stops at the first slice past C) and
    ln_stats_finalize2_kernel ("16clamped": batches of 16, slices past P re-read slice P - 1 and are not added) in fp32, one row per
    vector element.  Per slice: t = s_p * s_p / n; s += s_p; q += max(Q_p - t, 0); b += t.  Then mean = s / C,
    m2 = q + max(b - s * mean, 0), rstd = rsqrt(m2 / C + eps).
    Planted defects: "no_between" (m2 = q), "past_C" (a slice past C is added, with n = npp), "skip_ragged" (the last slice is dropped
    when it is narrower than npp), "mean_P_npp" (mean = s / (P * npp))."""
    part = part.float()
    P, M = part.shape[0], part.shape[1]
    s, q, b = (torch.zeros(M, dtype=F32) for _ in range(3))

    def add(v, n):
        nonlocal s, q, b
        t = v[:, 0] * v[:, 0] / torch.tensor(float(n), dtype=F32)
        s = s + v[:, 0]
        q = q + (v[:, 1] - t).clamp_min(0)
        b = b + t

    def width(p):
        n = min(npp, C - p * npp)
        if defect == "past_C" and n <= 0:
            return npp
        if defect == "skip_ragged" and 0 < n < npp:
            return 0
        return n

    if shape == "8+tail":
        p = 0
        while p + 8 <= P:
            v = [part[p + j] for j in range(8)]
            for j in range(8):
                if width(p + j) > 0:
                    add(v[j], width(p + j))
            p += 8
        while p < P:
            if width(p) <= 0:
                break
            add(part[p], width(p))
            p += 1
    else:
        assert shape == "16clamped"
        for p in range(0, P, 16):
            v = [part[min(p + j, P - 1)] for j in range(16)]
            for j in range(16):
                if p + j < P and width(p + j) > 0:
                    add(v[j], width(p + j))
    mean = s / torch.tensor(float(P * npp if defect == "mean_P_npp" else C), dtype=F32)
    m2 = q if defect == "no_between" else q + (b - s * mean).clamp_min(0)
    return mean, torch.rsqrt(m2 / torch.tensor(float(C), dtype=F32) + torch.tensor(eps, dtype=F32))


def standin_folded_gemm(A, W, mean, rstd, colsum, bias, defect=None, tile=256):
    """Python stand-in of a folded-LayerNorm GEMM epilogue, fp32: rstd * acc + ((-rstd * mean) * colsum + bias), as the kernels form it.
    Planted defects: "xor1" (the two rows of the last row pair of the first `tile`-row tile take each other's statistics -- a staging slip),
    "clamp_m2" (the rows of the ragged last tile are clamped to M - 2 instead of M - 1), "no_colsum" (mean * colsum dropped)."""
    M = A.shape[0]
    rows = torch.arange(M)
    if defect == "xor1":
        rows = torch.where((rows >= tile - 2) & (rows < tile), (rows ^ 1).clamp_max(M - 1), rows)
    elif defect == "clamp_m2":
        rows = torch.where(rows >= (M - 1) // tile * tile, rows.clamp_max(M - 2), rows)
    acc = A.float() @ W.float().T
    rs, mu = rstd.float()[rows], mean.float()[rows]
    st = -rs * mu
    inner = bias.float()[None, :] if defect == "no_colsum" else st[:, None] * colsum.float()[None, :] + bias.float()[None, :]
    return rs[:, None] * acc + inner


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ the documented claims
CLAIM_GROUPS = (0.0, 1.0, 2.0, 3.0, 5.0)
# Spread of RefOps' own folded / plain ratio over 8 seeds (CPU, 40 rows per group, K = 768, N = 192; tests/test_ln_cond_cpu.py re-measures
# it and profiles/ln_conditioning.md lists the figures): the largest |ratio / mean ratio - 1| of any group.
#   fp32 rows (norm1 / norm2):         0.038  (folded / plain, mean over the seeds: 0.99, 1.13, 1.46, 1.89, 2.85 for the five groups)
#   stored bf16 rows (sub-LayerNorms): 0.023  (0.84, 0.84, 0.85, 0.85, 0.85)
REFOPS_RATIO_SPREAD = {F32: 0.038, BF: 0.023}
CLAIM_MARGIN = {k: 3 * v for k, v in REFOPS_RATIO_SPREAD.items()}


def claim_problem(seed, dtype=F32, rows_per_group=40, K=768, N=192):
    """Rows in groups of |mean| / sigma = 0, 1, 2, 3, 5 (scale 1, no outliers), fp32 W / gamma / beta / bias, and the true fp64
    LayerNorm -> Linear of them.  dtype fp32: the residual stream in front of norm1 / norm2 (the folded chain contracts its bf16 copy);
    bf16: a stored bf16 tensor in front of a sub-LayerNorm (inner_attn_ln, ffn_ln), which both chains read as it is."""
    M = rows_per_group * len(CLAIM_GROUPS)
    x, desc = skewed_rows(M, K, seed, dtype, ratios=CLAIM_GROUPS, scales=(1.0,), outliers=False)
    g = torch.Generator().manual_seed(seed + 1000)
    W = torch.randn(N, K, generator=g) * 0.05
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    b = torch.randn(N, generator=g)
    _, _, y64 = ln_ref64(x, gamma, beta)
    true = y64 @ W.double().T + b.double()
    group = torch.arange(M) % len(CLAIM_GROUPS)
    return dict(x=x, W=W, gamma=gamma, beta=beta, b=b, true=true, group=group, desc=desc)


def claim_chains(ops, pr, device="cpu", flags=0):
    """(plain, folded) bf16 outputs [M, N] of `ops` (RefOps or HipOps): plain = layernorm_fwd -> gemm_nt; folded = the statistics of the
    fp32 rows (layernorm_fwd, y = None), their bf16 copy, gemm_nt_ln with W (.) gamma, its column sums and beta . W + b."""
    x, W, gamma, beta, b = (pr[k].to(device) for k in ("x", "W", "gamma", "beta", "b"))
    M, K = x.shape
    N = W.shape[0]
    kw = dict(flags=flags) if device != "cpu" else {}
    ln = torch.empty(M, K, dtype=BF, device=device)
    mean, rstd = torch.empty(M, device=device), torch.empty(M, device=device)
    ops.layernorm_fwd(x, gamma, beta, ln, mean, rstd, EPS)
    plain = torch.empty(M, N, dtype=BF, device=device)
    ops.gemm_nt(ln, W.to(BF), plain, b, epi=0, **kw)
    Wf = (W * gamma).to(BF)
    colsum, d = Wf.float().sum(1).contiguous(), (W @ beta + b).contiguous()
    folded = torch.empty(M, N, dtype=BF, device=device)
    ops.gemm_nt_ln(x.to(BF), Wf, folded, bias=d, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, epi=0, **kw)
    return plain.cpu(), folded.cpu()


def claim_rms(out, pr):
    """RMS distance to the true fp64 LayerNorm -> Linear per ratio group."""
    e = (out.double() - pr["true"]) ** 2
    return [float(e[pr["group"] == k].mean().sqrt()) for k in range(len(CLAIM_GROUPS))]
