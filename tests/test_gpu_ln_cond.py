"""`-m gpu`: the LayerNorm / row-statistics family on rows whose statistics differ row by row (tests/_ln_cond.py): |mean| / sigma from
0 to 1000, scales 2^-10 .. 2^10, alternating sign of the mean, outlier channels.  Every check is per row or per element against fp64 of
the operands the kernel got, with bounds derived from the number formats and the kernels' summation depths -- a row statistic that reaches
the wrong row, or a cancelling term that is dropped, misses them by orders of magnitude (tests/test_ln_cond_cpu.py plants such defects).
The worst error / bound of every case is appended to ln_cond_metrics.txt next to the metrics file of tests/test_gpu_ops.py; figures in
profiles/ln_conditioning.md."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _ln_cond as L  # noqa: E402
from _ln_cond import BF, EPS, F32, F64, U  # noqa: E402
from oracle.ops_ref import RefOps  # noqa: E402
from test_gpu_ops import _LOG as _OPS_LOG  # noqa: E402       (the metrics file that check() of the per-kernel tests appends to)

TOL_BF = 4e-3                                  # the project's own limits for dx (tests/test_gpu_ops.py)
_LOG = _OPS_LOG.with_name("ln_cond_metrics.txt")
FLAGS = [0, 0x30, 0x70, 0xB0, 0x10B0]
ROW_C = [192, 768, 1024, 1028, 2048, 2052, 2730, 3072]
FINALIZE_SETS = [(768, 64, 12), (1024, 64, 16), (2730, 32, 88), (341, 32, 12), (100, 64, 2), (64, 64, 1), (1090, 64, 18)] + \
                [(p * 32 - 5, 32, p) for p in (7, 8, 9, 15, 16, 17, 33)]                # C, npp, P


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@functools.lru_cache(maxsize=None)
def rows(M, C, seed, dtype, outliers=True):
    return L.skewed_rows(M, C, seed, dtype, outliers=outliers)


def _log(line):
    _LOG.parent.mkdir(exist_ok=True)
    with open(_LOG, "a") as f:
        f.write(line + "\n")


def within(name, got, want64, bound, desc):
    """per row / per element: |got - want64| <= bound; logs the worst error / bound, reports the worst row and the number of offenders"""
    worst, msg = L.check_rows((got.detach().double().cpu() - want64).abs(), bound, desc, name)
    _log(f"{name}: worst error/bound = {worst:.3e}")
    assert msg is None, msg


def rnd(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _padded(x, ld, pad_value=float("nan")):
    """[M, C] -> the [:, :C] view of an [M, ld] buffer: columns C .. roundup4(C) - 1 hold pad_value (the kernels fetch them), the rest 0."""
    M, C = x.shape
    buf = torch.zeros(M, ld, dtype=x.dtype)
    buf[:, :C] = x
    buf[:, C:(C + 3) // 4 * 4] = pad_value
    return buf.cuda()[:, :C]


def _vec(v, pad_value=float("nan")):
    C = v.shape[0]
    buf = torch.full(((C + 3) // 4 * 4,), pad_value)
    buf[:C] = v
    return buf.cuda()[:C]


def _ld(C):
    return C if C % 4 == 0 else (C + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ a. row kernels
@pytest.mark.parametrize("xdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", ROW_C)
def test_layernorm_forward_per_row(hip, C, xdt):
    M = 37                                                         # nine full workgroups of four rows + one row
    x, d = rows(M, C, 11, xdt)
    gamma, beta = 1 + rnd((C,), 12, 0.2), rnd((C,), 13, 0.2)
    _, _, y64 = L.ln_ref64(x, gamma, beta)
    ld = _ld(C)
    xd, gd, bd = _padded(x, ld), _vec(gamma), _vec(beta)           # C % 4 == 2: NaN in the pad columns of x / gamma / beta
    tag = f"ln_fwd[{C},{'f32' if xdt == F32 else 'bf16'}]"
    ybuf = torch.full((M, ld), 7.0, dtype=BF, device="cuda")
    md, rd = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
    hip.layernorm_fwd(xd, gd, bd, ybuf[:, :C], md, rd, EPS)
    within(tag + ".mean", md, d["mean"], L.ln_mean_bound(d), d)
    within(tag + ".rstd", rd.double().cpu() / d["rstd"], torch.ones(M, dtype=F64), L.ln_rstd_bound(d) * torch.ones(M, dtype=F64), d)
    within(tag + ".y", ybuf[:, :C], y64, L.ln_y_bound(x, gamma, beta, d, y64, BF), d)
    if C % 4:
        assert int((ybuf[:, C:(C + 3) // 4 * 4] != 0).sum()) == 0, "pad columns of y leave as exact zeros"
    # statistics only (y = NULL): the same bits
    m2, r2 = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    hip.layernorm_fwd(xd, None, None, None, m2, r2, EPS)
    assert torch.equal(m2, md) and torch.equal(r2, rd), f"{tag}: the statistics-only launch differs from the full launch"
    if C % 4 == 0 and xdt == F32:                                   # fp32 rows -> fp32 rows
        yf, m3, r3 = torch.full((M, C), float("nan"), device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
        hip.layernorm_fwd_f32(xd, gd, bd, yf, m3, r3, EPS)
        within(tag + ".f32.mean", m3, d["mean"], L.ln_mean_bound(d), d)
        within(tag + ".f32.rstd", r3.double().cpu() / d["rstd"], torch.ones(M, dtype=F64), L.ln_rstd_bound(d) * torch.ones(M, dtype=F64), d)
        within(tag + ".f32.y", yf, y64, L.ln_y_bound(x, gamma, beta, d, y64, F32), d)
    if C in (768, 2730):                                            # + the e4m3 copy: the row quantiser applied to what y holds, bit for bit
        Kp = (ld + 127) // 128 * 128
        y1 = torch.zeros(M, ld, dtype=BF, device="cuda")
        q1, s1 = torch.full((M, Kp), 0x55, dtype=torch.uint8, device="cuda"), torch.zeros(M, device="cuda")
        m4, r4 = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
        hip.layernorm_fwd(xd, gd, bd, y1[:, :C], m4, r4, EPS, q8=q1, q_scale=s1)
        assert torch.equal(y1[:, :C], ybuf[:, :C]) and torch.equal(m4, md) and torch.equal(r4, rd)
        q0, s0 = torch.full((M, Kp), 0xAA, dtype=torch.uint8, device="cuda"), torch.zeros(M, device="cuda")
        hip.quant_rows_fp8(y1, q0, s0)
        bad = (q0 != q1).any(-1) | (s0 != s1)
        assert not bool(bad.any()), f"{tag}.q8: {int(bad.sum())} rows differ from cs_quant_rows_fp8(y); first {L.describe(d, int(bad.nonzero()[0]))}"


# ------------------------------------------------------------------------------------------------ b. backward
def _row_rel(got, want64):
    got = got.detach().double().cpu()
    return (got - want64).norm(dim=-1) / want64.norm(dim=-1).clamp_min(1e-300)


@pytest.mark.parametrize("xdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", ROW_C)
def test_layernorm_backward_per_row_and_per_column(hip, C, xdt):
    M = 37
    x, d = rows(M, C, 11, xdt)
    gamma = 1 + rnd((C,), 12, 0.2)
    dy = rnd((M, C), 14, dtype=BF)
    mean, rstd = d["mean"].float(), d["rstd"].float()              # the fp64 statistics rounded to fp32: what the kernel is given
    dx64, dg64, db64, dg_abs, db_abs = L.ln_bwd_ref64(dy, x, gamma, mean, rstd)
    ld = _ld(C)
    xd, gd, dyd, md, rd = _padded(x, ld), _vec(gamma), _padded(dy, ld), mean.cuda(), rstd.cuda()
    ws = torch.empty(hip.layernorm_bwd_workspace(M, C), dtype=torch.uint8, device="cuda")
    tag = f"ln_bwd[{C},{'f32' if xdt == F32 else 'bf16'}]"
    ones = torch.ones(M, dtype=F64)
    for mode, odt, tol in ((0, BF, TOL_BF), (1, F32, 1e-4), (2, F32, 1e-4)):
        base = rnd((M, C), 15).to(odt)
        want = dx64 + (base.double() if mode == 2 else 0.0)
        for params in (True, False):
            dxd = _padded(base, ld, pad_value=3.0)
            dg, db = (torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")) if params else (None, None)
            hip.layernorm_bwd(dyd, xd, gd, md, rd, dxd, mode, dg, db, False, ws)
            within(f"{tag}.dx{mode}{'p' if params else ''}", _row_rel(dxd, want), torch.zeros(M, dtype=F64), tol * ones, d)
            if params:                                              # per column: depth <= M rows, three roundings per term
                within(f"{tag}.dgamma{mode}", dg, dg64, M * U * dg_abs, None)
                within(f"{tag}.dbeta{mode}", db, db64, M * U * db_abs, None)
            if mode == 0:
                continue
            dx2 = _padded(base, ld, pad_value=3.0)                  # + the bf16 copy of the updated rows and its column sums
            cpy = torch.full((M, ld), float("nan"), dtype=BF, device="cuda")[:, :C]
            cs = torch.full((C,), float("nan"), device="cuda")
            hip.layernorm_bwd(dyd, xd, gd, md, rd, dx2, mode, dg, db, False, ws, dx_copy=cpy, copy_colsum=cs)
            within(f"{tag}.copy.dx{mode}{'p' if params else ''}", _row_rel(dx2, want), torch.zeros(M, dtype=F64), tol * ones, d)
            assert torch.equal(cpy, dx2.to(BF)), f"{tag}: the copy is the rounded stream"
            c64 = cpy.double().cpu()
            within(f"{tag}.colsum{mode}{'p' if params else ''}", cs, c64.sum(0), M * U * c64.abs().sum(0), None)


# ------------------------------------------------------------------------------------------------ c. cs_ln_stats_finalize on exact partials
@pytest.mark.parametrize("M", [37, 38, 513, 514])
@pytest.mark.parametrize("C,npp,P", FINALIZE_SETS)
def test_stats_finalize_on_exact_partials(hip, C, npp, P, M):
    x, d = rows(M, C, 5, F32)
    part = L.exact_partials(x, npp, P)                              # slices past C are NaN: they must be ignored
    Pv = (C + npp - 1) // npp
    pd = part.cuda()
    mean, rstd = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
    hip.ln_stats_finalize(pd, npp, C, mean, rstd, EPS)              # odd M: one row per thread; even M: two rows per thread
    tag = f"finalize[C={C},npp={npp},P={P},M={M}]"
    within(tag + ".mean", mean, d["mean"], L.finalize_mean_bound(Pv, d), d)
    within(tag + ".rstd", rstd.double().cpu() / d["rstd"], torch.ones(M, dtype=F64), L.finalize_rstd_bound(Pv, d), d)
    if M % 2 == 0:
        # the two kernels are documented as bit-identical: the same partials 8 bytes into a larger buffer select the one-row kernel
        big = torch.zeros(P * M * 2 + 4, device="cuda")
        view = big[2:2 + P * M * 2].view(P, M, 2)
        view.copy_(pd)
        assert pd.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
        m1, r1 = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
        hip.ln_stats_finalize(view, npp, C, m1, r1, EPS)
        assert torch.equal(m1, mean) and torch.equal(r1, rstd), f"{tag}: the paired kernel differs from the one-row kernel"


# ------------------------------------------------------------------------------------------------ d. producers of the partials
def _check_partials(tag, part_d, out, n, desc):
    """part_d [P, M, 2] against the fp64 sums of the kernel's OWN output `out` [M, C], slices of n columns, per row and slice"""
    p64 = L.slice_partials64(out.detach().cpu(), n)
    Pv = p64.shape[0]
    bs, bq = L.partial_bounds(p64, n)
    got = part_d.detach().double().cpu()[:Pv]
    within(tag + ".sum", got[:, :, 0].T, p64[:, :, 0].T, bs.T, desc)
    within(tag + ".sumsq", got[:, :, 1].T, p64[:, :, 1].T, bq.T, desc)


def _out_desc(out):
    """descriptors of a kernel's output rows (for failure messages and the ratio-span assertions)"""
    o = out.detach().double().cpu()
    mean, var = o.mean(-1), o.var(-1, unbiased=False)
    ratio = mean.abs() / var.sqrt()
    sc = torch.exp2(torch.round(torch.log2(var.sqrt().clamp_min(1e-30))))
    return dict(ratio0=ratio.round(), ratio=ratio, scale=sc, outlier=torch.zeros(len(o), dtype=torch.bool), mean=mean, var=var)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("C", [192, 768])
def test_residual_gemm_partials_per_row_and_slice(hip, C, flags):
    M, K = 261, 128
    extra, d = rows(M, C, 31, F32)
    A, W, bias = rnd((M, K), 32, dtype=BF), rnd((C, K), 33, 2.0 ** -20, BF), rnd((C,), 34, 2.0 ** -17)      # A.W^T is small against every row
    S = (C + 63) // 64
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    x = extra.cuda().clone()
    xb = torch.zeros(M, C, dtype=BF, device="cuda")
    part = torch.full((S, M, 2), float("nan"), device="cuda")
    hip.gemm_nt_ln(Ad, Wd, x, bias=bd, extra=x, stats_part=part, xb_out=xb, epi=2, flags=flags)
    od = _out_desc(x)
    assert float(od["ratio"].min()) < 0.05 and float(od["ratio"].max()) >= 100, "the output rows keep ratios from 0 to >= 100"
    tag = f"resid_partials[{C}] flags={flags:#x}"
    _check_partials(tag, part, x, 64, d)
    assert torch.equal(xb, x.to(BF)), f"{tag}: the bf16 copy is the rounded stream"
    if flags in (0, 0x10B0):                                        # the split stream: fp32 in -> planes out (its flags carry no schedule)
        hi, lo = torch.zeros(M, C, dtype=BF, device="cuda"), torch.zeros(M, C, dtype=torch.int16, device="cuda")
        p2 = torch.full((S, M, 2), float("nan"), device="cuda")
        zero, one = torch.zeros(M, device="cuda"), torch.ones(M, device="cuda")
        hip.gemm_nt_ln_split(Ad, Wd, hi, lo, bd, zero, one, torch.zeros(C, device="cuda"), x_in=extra.cuda(), stats_part=p2, flags=flags & 0x1000)
        xs = RefOps.join_planes(hi, lo)
        _check_partials(tag + ".split", p2, xs, 64, d)
        want = extra.double() + A.double() @ W.double().T + bias.double()
        within(tag + ".split.x", xs, want, K * U * (A.double().abs() @ W.double().abs().T) + 3 * U * (want.abs() + extra.double().abs()), d)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("Hd,Hl", [(384, 341), (2752, 2730)])
def test_swiglu_gemm_partials_per_row_and_slice(hip, Hd, Hl, flags):
    M, K = 261, 128
    A = rnd((M, K), 40)
    A = (A * torch.tensor([0.02, 0.3, 1.0, 4.0, 16.0])[torch.arange(M) % 5][:, None]).to(BF)        # per-row scale: small rows are bias-driven
    W, bias = rnd((2 * Hd, K), 41, 0.05, BF), rnd((2 * Hd,), 42, 0.05)
    bias[:Hd] += 3.0                                                 # gate bias: silu(x1) ~ x1 > 0, so rows with small A have |mean| >> sigma
    bias[Hd:] += 2.0
    W[Hl:Hd] = 0; W[Hd + Hl:] = 0; bias[Hl:Hd] = 0; bias[Hd + Hl:] = 0          # padded hidden units are exact zeros
    P = 4 * ((Hd + 127) // 128)
    h = torch.full((M, Hd), float("nan"), dtype=BF, device="cuda")
    part = torch.full((P, M, 2), float("nan"), device="cuda")
    hip.gemm_nt_ln(A.cuda(), W.cuda(), h, bias=bias.cuda(), stats_part=part, epi=3, group=Hd, flags=flags)
    od = _out_desc(h[:, :Hl])
    assert float(od["ratio"].min()) < 0.5 and float(od["ratio"].max()) >= 5, (float(od["ratio"].min()), float(od["ratio"].max()))
    assert int((h[:, Hl:] != 0).sum()) == 0
    tag = f"swiglu_partials[{Hd},{Hl}] flags={flags:#x}"
    _check_partials(tag, part, h[:, :Hl], 32, od)
    mean, rstd = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    # the device's partials carry n roundings each instead of one (partial_bounds): the depth of the exact-partial bounds grows by n for
    # the mean and by 2 n for the variance (the sum enters it squared)
    hip.ln_stats_finalize(part, 32, Hl, mean, rstd, EPS)
    m64, r64, _ = L.ln_ref64(h[:, :Hl].cpu())
    Pv = (Hl + 31) // 32
    within(tag + ".mean", mean, m64, L.finalize_mean_bound(Pv + 32, od), od)
    within(tag + ".rstd", rstd.double().cpu() / r64, torch.ones(M, dtype=F64), L.finalize_rstd_bound(Pv + 64, od), od)


@pytest.mark.parametrize("B,Ntok,H", [(2, 17, 2), (1, 197, 3), (1, 226, 2)])
def test_attention_partials_per_row_and_head(hip, B, Ntok, H):
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), 50)
    for hh in range(H):
        qkv[:, 2 * C + hh * 64:2 * C + hh * 64 + 64] += 8.0 + 0.5 * hh            # v: a constant per head -> output rows with |mean| >> sigma
    qkv[:Ntok // 2, 2 * C:] -= 8.0                                   # ... and rows near ratio 0 where the first keys dominate
    qkv = qkv.to(BF).cuda()
    o = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
    part = torch.full((H, B * Ntok, 2), float("nan"), device="cuda")
    hip.attn_fwd_stats(qkv, None, None, o, None, part, B, Ntok, H, 0.125)
    od = _out_desc(o)
    assert float(od["ratio"].max()) >= 5, float(od["ratio"].max())
    tag = f"attn_partials[{B},{Ntok},{H}]"
    _check_partials(tag, part, o, 64, od)
    mean, rstd = torch.zeros(B * Ntok, device="cuda"), torch.zeros(B * Ntok, device="cuda")
    hip.ln_stats_finalize(part, 64, C, mean, rstd, EPS)
    m64, r64, _ = L.ln_ref64(o.cpu())
    within(tag + ".mean", mean, m64, L.finalize_mean_bound(H + 64, od), od)
    within(tag + ".rstd", rstd.double().cpu() / r64, torch.ones(B * Ntok, dtype=F64), L.finalize_rstd_bound(H + 128, od), od)


# ------------------------------------------------------------------------------------------------ e. folded GEMM epilogues
def _folded_operands(hip, K, N, seed):
    """skewed bf16 rows, their statistics from cs_ln_stats_finalize on exact partials (as in c.), W (.) gamma, its column sums, beta.W + b"""
    M = 261                                                          # one full 256-row tile + 5 rows
    xb, d = rows(M, K, 21, BF)
    mean, rstd = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    hip.ln_stats_finalize(L.exact_partials(xb, 64).cuda(), 64, K, mean, rstd, EPS)
    W, gamma, beta, b = rnd((N, K), seed, 0.05), 1 + rnd((K,), seed + 1, 0.2), rnd((K,), seed + 2, 0.1), rnd((N,), seed + 3)
    Wf = (W * gamma).to(BF)
    return xb, d, mean, rstd, Wf, Wf.float().sum(1).contiguous(), (W @ beta + b).contiguous()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("K", [192, 768])
def test_folded_layernorm_gemm_epilogues_per_element(hip, K, flags):
    M, N = 261, 192
    xb, d, mean, rstd, Wf, colsum, bias = _folded_operands(hip, K, N, 60)
    Ad, Wd, cd, bd = xb.cuda(), Wf.cuda(), colsum.cuda(), bias.cuda()
    m_c, r_c = mean.cpu(), rstd.cpu()                                # the reference takes the device's own mean / rstd
    pre64, bpre = L.folded_gemm_ref64(xb, Wf, m_c, r_c, colsum, bias)
    tag = f"fold[K={K}] flags={flags:#x}"
    kw = dict(bias=bd, ln_mean=mean, ln_rstd=rstd, ln_colsum=cd, flags=flags)
    out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt_ln(Ad, Wd, out, epi=0, **kw)
    within(tag + ".epi0", out, pre64, bpre + L.bf16_half_ulp(pre64), d)
    for epi, name, f in ((7, "gelu", lambda t: F.gelu(t)), (8, "qgelu", lambda t: t * torch.sigmoid(1.702 * t))):
        out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
        hip.gemm_nt_ln(Ad, Wd, out, epi=epi, **kw)
        within(f"{tag}.epi{epi}", out, f(pre64), L.through_activation(bpre, pre64, f(pre64), name), d)
    # SwiGLU: columns [0, 96) gate, [96, 192) value
    G = N // 2
    out = torch.full((M, G), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt_ln(Ad, Wd, out, epi=3, group=G, **kw)
    u64, v64, bu, bv = pre64[:, :G], pre64[:, G:], bpre[:, :G], bpre[:, G:]
    s64 = F.silu(u64)
    h64 = s64 * v64
    bs = L.through_activation(bu, u64, s64, "silu") - L.bf16_half_ulp(s64)          # silu(u) stays in fp32
    within(tag + ".epi3", out, h64, v64.abs() * bs + s64.abs() * bv + bs * bv + 2 * U * h64.abs() + L.bf16_half_ulp(h64), d)
    # residual stream (epilogue 6; epilogue 2 takes no folded LayerNorm) and the same on the split stream
    extra = rnd((M, N), 64)
    o64, bo = L.folded_gemm_ref64(xb, Wf, m_c, r_c, colsum, bias, extra=extra)
    x = extra.cuda().clone()
    hip.gemm_nt_ln(Ad, Wd, x, extra=x, epi=6, **kw)
    within(tag + ".epi6", x, o64, bo, d)
    with pytest.raises(RuntimeError):
        hip.gemm_nt_ln(Ad, Wd, x.clone(), extra=x, epi=2, **kw)
    if flags in (0, 0x10B0):
        hi, lo = torch.zeros(M, N, dtype=BF, device="cuda"), torch.zeros(M, N, dtype=torch.int16, device="cuda")
        part = torch.full(((N + 63) // 64, M, 2), float("nan"), device="cuda")
        hip.gemm_nt_ln_split(Ad, Wd, hi, lo, bd, mean, rstd, cd, x_in=extra.cuda(), stats_part=part, flags=flags & 0x1000)
        xs = RefOps.join_planes(hi, lo)
        within(tag + ".split", xs, o64, bo, d)
        if flags == 0x10B0:                                          # same kernel family: the same bits
            assert torch.equal(xs.view(torch.int32), x.view(torch.int32)), f"{tag}: the split stream is the fp32 stream bit for bit"
        _check_partials(tag + ".split", part, xs, 64, d)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32_rows", "bf16_rows"])
def test_documented_conditioning_of_the_folded_chain(hip, dtype):
    """engine_base.py: the folded norm1 / norm2 contract the bf16 copy of the fp32 stream, so their error grows like sqrt(1 + (mean / sigma)^2)
    against the plain LayerNorm -> GEMM chain, and the guard sits at 2 (fp32 rows).  engine.py: the sub-LayerNorm folds read a stored bf16
    tensor either way, are never worse than the plain chain and need no guard (bf16 rows).  Per ratio group 0 / 1 / 2 / 3 / 5: RMS
    distance of both chains to the true fp64 LayerNorm -> Linear, on the GPU and through RefOps (same roundings, another accumulation
    order).  The GPU's folded / plain ratio must lie within three times RefOps' own seed-to-seed spread of RefOps' ratio
    (tests/_ln_cond.py: CLAIM_MARGIN; neither side of that margin is the code under test)."""
    pr = L.claim_problem(0, dtype)
    ref_plain, ref_fold = L.claim_chains(RefOps(), pr)
    gpu_plain, gpu_fold = L.claim_chains(hip, pr, device="cuda")
    rows_ = zip(L.CLAIM_GROUPS, L.claim_rms(gpu_plain, pr), L.claim_rms(gpu_fold, pr), L.claim_rms(ref_plain, pr), L.claim_rms(ref_fold, pr))
    bad, name = [], "f32 rows" if dtype == F32 else "bf16 rows"
    for r, gp, gf, rp, rf in rows_:
        _log(f"claim {name} ratio={r:g}: GPU plain {gp:.4e} folded {gf:.4e} folded/plain {gf / gp:.3f} | RefOps plain {rp:.4e} folded {rf:.4e} "
             f"folded/plain {rf / rp:.3f} | sqrt(1+r^2) {(1 + r * r) ** 0.5:.3f}")
        if abs((gf / gp) / (rf / rp) - 1) > L.CLAIM_MARGIN[dtype] or (dtype == BF and gf > gp):
            bad.append((r, gf / gp, rf / rp))
    assert not bad, f"{name}: folded / plain (ratio group, GPU, RefOps) outside +-{L.CLAIM_MARGIN[dtype]:.3f} (or a sub-LN fold worse than plain): {bad}"
