"""`-m gpu`: the GEMM family on exactly representable operands -- every element, bit for bit (tests/_exact_gemm.py).

Small-integer / power-of-two operands whose partial sums stay below 2^24 steps make fp32 accumulation exact in any order, so every schedule,
tile shape, staging path, split count and raster must produce THE fp32 result known from float64 arithmetic; every linear epilogue is
compared in bits (bf16 outputs with their round-to-nearest-even image, ties included), every output is NaN-prefilled, operands sit in
rows wider than K whose padding holds NaN, and the padding of C must keep its prefill.  A mismatch names row, column, tile and schedule
(in the metrics file that test_gpu_ops.check() writes).  The non-linear epilogues (3, 7, 8) have an exact pre-activation: they are checked per element against the
float64 activation, bound derived from fp32 / bf16 precision.  Shapes: the edges of the row / column tiles and the K-tile counts against the
ring depths (_exact_gemm.TRIPLES).  What ran is summarised in gemm_exact_summary.txt beside that file (profiles/gemm_exact_tests.md)."""
import os
import time
from collections import Counter

import pytest
import torch

import _exact_gemm as X
from _exact_gemm import BF, F32
from oracle.ops_ref import RefOps

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-5                                  # tests/test_gpu_ops.py: the bound of cs_ln_stats_finalize (it divides and takes rsqrt)
NAN = float("nan")
LAUNCHES = Counter()                            # compared launches per family
ACT_SHARE = {}                                  # (family, epilogue) -> largest share of elements differing from bf16(float64 activation)
T0 = time.time()


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    ops = HipOps()
    yield ops
    X.LOG.parent.mkdir(exist_ok=True)
    with open(X.LOG.parent / "gemm_exact_summary.txt", "w") as f:
        f.write(f"module wall time {time.time() - T0:.1f} s, {sum(LAUNCHES.values())} compared launches\n")
        for k in sorted(LAUNCHES):
            f.write(f"launches {k}: {LAUNCHES[k]}\n")
        for k in sorted(ACT_SHARE):
            f.write(f"largest differing share {k}: {ACT_SHARE[k]:.4%}\n")


def tile_of(flags):
    return X.TILE_OF_FLAGS.get(flags & 0xF0, (256, 256))


def wide(t, pad):
    """t on the GPU as the left columns of rows `pad` elements wider; the padding holds NaN (0xFF bytes for integers): an operand read
    past K, or an output written past N, shows."""
    if not pad:
        return t.cuda().contiguous()
    if t.is_floating_point():
        buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype, device="cuda")
    else:
        buf = torch.full((t.shape[0], t.shape[1] + pad), 255 if t.dtype == torch.uint8 else -1, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def blank(rows, cols, dtype, pad):
    """NaN-prefilled output [rows, cols] inside rows `pad` wider: (whole buffer, view)."""
    buf = torch.full((rows, cols + pad), NAN, dtype=dtype, device="cuda")
    return buf, buf[:, :cols]


def same(fails, name, got, want_dev, tile=(256, 256), buf=None):
    """Bit comparison on the GPU; the localising comparator runs only on a mismatch.  buf: the padded buffer whose padding must be NaN."""
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[got.element_size()]
    if not torch.equal(got.view(iv), want_dev.view(iv)):
        fails.bits(name, got.cpu(), want_dev.cpu(), tile)
    if buf is not None and buf.shape[1] > got.shape[1] and not torch.isnan(buf[:, got.shape[1]:]).all():
        fails.add(f"{name}: the padding of the output rows (ldc > N) lost its prefill")


def act_check(fails, family, name, got, pre, epi, group=0):
    msg, share = X.activation_mismatch(name, got, pre, epi, group)
    fails.add(msg)
    ACT_SHARE[(family, epi)] = max(ACT_SHARE.get((family, epi), 0.0), share if got.numel() >= X.CENSUS_MIN_ELEMENTS else 0.0)


PADS = [0, 1]


# ------------------------------------------------------------------------------------------------ cs_gemm_nt, linear epilogues
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_linear_epilogues_on_every_schedule(hip, M, N, K, pad):
    """Epilogues 0, 1, 2 (in place), 4 (splits 1, 2, 3, 7 and the library's choice; 7 exceeds the K tiles of K <= 256) and 5 (a group
    that divides no row tile) on all twelve schedule flags.  Where launch<> falls back to another kernel the result is the same bits."""
    o = X.operands(M, N, K, seed=100)
    v = X.exact_gemm(o["A"], o["B"], o["bias"])
    X.assert_rounding_is_tested(f"wide[{M},{N},{K}]", v)
    w0, w1 = X.want_bf16(v).cuda(), X.want_f32(v).cuda()
    w2 = X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], o["res"])).cuda()
    w4 = X.want_f32(X.exact_gemm(o["A"], o["B"], None, o["res"])).cuda()
    G = X.patch_group(M)
    rows = M + (M + G - 1) // G
    pos = X.int_f32((G + 1, N), 1000, 107)
    orow, prow = X.patch_rows(M, G)
    w5 = torch.full((rows, N), NAN)
    w5[orow] = X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], pos[prow]))
    w5 = w5.cuda()
    A, B, bias, res = wide(o["A"], 8 * pad), wide(o["B"], 16 * pad), o["bias"].cuda(), o["res"].cuda()
    posd = wide(pos, 12 * pad)
    fails = X.Failures()
    for fl in X.FLAGS:
        tag, t = f"[{M},{N},{K}] pad={pad} flags={fl:#x}", tile_of(fl)
        buf, C = blank(M, N, BF, 12 * pad)
        hip.gemm_nt(A, B, C, bias, epi=0, flags=fl)
        same(fails, "epi0 " + tag, C, w0, t, buf)
        buf, C = blank(M, N, F32, 12 * pad)
        hip.gemm_nt(A, B, C, bias, epi=1, flags=fl)
        same(fails, "epi1 " + tag, C, w1, t, buf)
        buf, C = blank(M, N, F32, 12 * pad)
        C.copy_(res)
        hip.gemm_nt(A, B, C, bias, C, epi=2, flags=fl)
        same(fails, "epi2 in place " + tag, C, w2, t, buf)
        for splits in (1, 2, 3, 7, 0):
            buf, C = blank(M, N, F32, 12 * pad)
            C.copy_(res)
            hip.gemm_nt(A, B, C, epi=4, splits=splits, flags=fl)
            same(fails, f"epi4 splits={splits} " + tag, C, w4, t, buf)
        buf, C = blank(rows, N, F32, 12 * pad)
        hip.gemm_nt(A, B, C, bias, posd, epi=5, group=G, flags=fl)
        same(fails, f"epi5 group={G} " + tag, C, w5, t, buf)
        LAUNCHES["cs_gemm_nt linear"] += 9
    fails.done()


@pytest.mark.parametrize("pad", [1])
@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_nonlinear_epilogues_on_every_schedule(hip, M, N, K, pad):
    """Epilogues 3 (SwiGLU), 7 (GELU) and 8 (QuickGELU): exact pre-activation, float64 activation, per-element bound of one bf16 spacing
    + 8 * 2^-23 * max |pre|, and at most 1 % of the elements differing from bf16(float64) at all (the rest equal in bits)."""
    fails = X.Failures()
    for epi in (3, 7, 8):
        a = X.act_case(M, N, K, 300 + epi, epi)
        pre = a["pre"]
        A, B, bias = wide(a["A"], 8 * pad), wide(a["B"], 16 * pad), a["bias"].cuda()
        for fl in X.FLAGS:
            buf, C = blank(M, N, BF, 12 * pad)
            hip.gemm_nt(A, B, C, bias, epi=epi, group=N if epi == 3 else 0, flags=fl)
            name = f"epi{epi} [{M},{N},{K}] pad={pad} flags={fl:#x}"
            act_check(fails, "cs_gemm_nt", name, C, pre, epi, N)
            if pad and not torch.isnan(buf[:, N:]).all():
                fails.add(f"{name}: the padding of the output rows lost its prefill")
            LAUNCHES["cs_gemm_nt non-linear"] += 1
    fails.done()


# ------------------------------------------------------------------------------------------------ cs_gemm_nt_ln
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_folded_layernorm_linear_epilogues(hip, M, N, K, pad):
    """cs_gemm_nt_ln: epilogue 6; epilogue 0 with the fold; epilogues 2 and 6 with the bf16 copy and the statistics partials; then
    cs_ln_stats_finalize on the exact partials (it divides and takes rsqrt: RefOps.ln_stats_finalize under TOL_F32, not bits).  Epilogue 2
    takes no fold (include/clipself_hip.h: "epi 0 / 3 with ln_mean != NULL", epilogue 6 is its residual form): asking is an error."""
    o = X.operands(M, N, K, seed=200)
    ln = (o["mean"], o["rstd"], o["colsum"])
    w6 = X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], o["res"], ln=ln)).cuda()
    v0 = X.exact_gemm(o["A"], o["B"], o["bias"], ln=ln)
    X.assert_rounding_is_tested(f"ln wide[{M},{N},{K}]", v0)
    w0 = X.want_bf16(v0).cuda()
    A, B, bias, res = wide(o["A"], 8 * pad), wide(o["B"], 16 * pad), o["bias"].cuda(), o["res"].cuda()
    lnd = dict(ln_mean=ln[0].cuda(), ln_rstd=ln[1].cuda(), ln_colsum=ln[2].cuda())
    s = X.operands(M, N, K, seed=210, profile="stats")
    sln = (s["mean"], s["rstd"], s["colsum"])
    sA, sB, sbias, sres = wide(s["A"], 8 * pad), wide(s["B"], 16 * pad), s["bias"].cuda(), s["res"].cuda()
    slnd = dict(ln_mean=sln[0].cuda(), ln_rstd=sln[1].cuda(), ln_colsum=sln[2].cuda())
    S = (N + 63) // 64
    wants = {}
    for epi, fold in ((2, None), (6, sln)):
        v = X.exact_gemm(s["A"], s["B"], s["bias"], s["res"], ln=fold)
        X.assert_rounding_is_tested(f"stats[{M},{N},{K}] epi {epi}", v)
        part = X.exact_stats(v, 64)
        mr, rr = torch.empty(M), torch.empty(M)
        RefOps().ln_stats_finalize(part, 64, N, mr, rr, 1e-6)
        wants[epi] = (X.want_f32(v).cuda(), X.want_bf16(v).cuda(), part.cuda(), mr, rr)
    with pytest.raises(RuntimeError, match="folded LayerNorm exists for epilogues 0, 3, 6, 7 and 8"):
        hip.gemm_nt_ln(A, B, res.clone(), bias=bias, extra=res, epi=2, **lnd)
    fails = X.Failures()
    for fl in X.FLAGS:
        tag, t = f"[{M},{N},{K}] pad={pad} flags={fl:#x}", tile_of(fl)
        buf, C = blank(M, N, F32, 12 * pad)
        C.copy_(res)
        hip.gemm_nt_ln(A, B, C, bias=bias, extra=C, epi=6, flags=fl, **lnd)
        same(fails, "ln epi6 in place " + tag, C, w6, t, buf)
        buf, C = blank(M, N, BF, 12 * pad)
        hip.gemm_nt_ln(A, B, C, bias=bias, epi=0, flags=fl, **lnd)
        same(fails, "ln epi0 folded " + tag, C, w0, t, buf)
        for epi in (2, 6):
            wx, wxb, wpart, mr, rr = wants[epi]
            buf, C = blank(M, N, F32, 12 * pad)
            C.copy_(sres)
            xbuf, xb = blank(M, N, BF, 8 * pad)
            part = torch.full((S, M, 2), NAN, device="cuda")
            hip.gemm_nt_ln(sA, sB, C, bias=sbias, extra=C, stats_part=part, xb_out=xb, epi=epi, flags=fl, **(slnd if epi == 6 else {}))
            same(fails, f"ln epi{epi}+xb+stats x " + tag, C, wx, t, buf)
            same(fails, f"ln epi{epi}+xb+stats xb_out " + tag, xb, wxb, t, xbuf)
            same(fails, f"ln epi{epi}+xb+stats stats_part[slice*M + row] " + tag, part.reshape(S * M, 2), wpart.reshape(S * M, 2), (M, 2))
            md, rd = torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
            hip.ln_stats_finalize(part, 64, N, md, rd, 1e-6)
            for nm, g, w in (("mean", md, mr), ("rstd", rd, rr)):
                r = float((g.cpu().double() - w.double()).norm() / (w.double().norm() + 1e-30))
                if not (r <= TOL_F32):
                    fails.add(f"ln_stats_finalize {nm} after epi{epi} {tag}: rel {r:.3e} > {TOL_F32:.1e}")
        LAUNCHES["cs_gemm_nt_ln linear"] += 4
        LAUNCHES["cs_ln_stats_finalize"] += 2
    fails.done()


@pytest.mark.parametrize("pad", [1])
@pytest.mark.parametrize("M,N,K", X.TRIPLES)
def test_folded_layernorm_nonlinear_epilogues(hip, M, N, K, pad):
    """cs_gemm_nt_ln: epilogues 3, 7, 8 behind the fold, and epilogue 3 with stats_part (with and without the fold).  The partials are sums
    of the kernel's own rounded outputs: against their float64 sums, |error| <= 32 * 2^-24 * sum |h| (32 fp32 additions) and
    33 * 2^-24 * sum h^2 (one more rounding for the square) per 32-unit slice.  Of the 4 * ceil(group / 128) slices only those that begin
    below the hidden width are defined: a kernel writes the slices of the column tiles it runs, and cs_ln_stats_finalize ignores the others
    (include/clipself_hip.h: "slices past C ignored"), so they may keep their prefill."""
    fails = X.Failures()
    for epi in (3, 7, 8):
        a = X.act_case(M, N, K, 320 + epi, epi, fold=True)
        ln = (a["mean"], a["rstd"], a["colsum"])
        pre_ln, pre = a["pre_ln"], a["pre"]
        A, B, bias = wide(a["A"], 8 * pad), wide(a["B"], 16 * pad), a["bias"].cuda()
        lnd = dict(ln_mean=ln[0].cuda(), ln_rstd=ln[1].cuda(), ln_colsum=ln[2].cuda())
        P = 4 * ((N + 127) // 128)
        for fl in X.FLAGS:
            tag = f"[{M},{N},{K}] pad={pad} flags={fl:#x}"
            buf, C = blank(M, N, BF, 12 * pad)
            hip.gemm_nt_ln(A, B, C, bias=bias, epi=epi, group=N if epi == 3 else 0, flags=fl, **lnd)
            act_check(fails, "cs_gemm_nt_ln", f"ln epi{epi} folded " + tag, C, pre_ln, epi, N)
            LAUNCHES["cs_gemm_nt_ln non-linear"] += 1
            if epi != 3:
                continue
            for fold, kw, p in ((True, lnd, pre_ln), (False, {}, pre)):
                buf, C = blank(M, N, BF, 12 * pad)
                part = torch.full((P, M, 2), NAN, device="cuda")
                hip.gemm_nt_ln(A, B, C, bias=bias, stats_part=part, epi=3, group=N, flags=fl, **kw)
                name = f"ln epi3+stats fold={fold} " + tag
                act_check(fails, "cs_gemm_nt_ln", name, C, p, 3, N)
                h = torch.zeros(M, 32 * P, dtype=torch.float64)
                h[:, :N] = C.cpu().double()
                h = h.reshape(M, P, 32)
                live = (N + 31) // 32
                got, h = part.cpu().double()[:live], h[:, :live]
                for j, (w, scale) in enumerate(((h.sum(-1), 32), ((h * h).sum(-1), 33))):
                    bound = scale * 2.0 ** -24 * (h.abs() if j == 0 else h * h).sum(-1)
                    bad = ~((got[:, :, j].T - w).abs() <= bound)
                    if bad.any():
                        r, sl = (int(x) for x in bad.nonzero()[0])
                        fails.add(f"{name}: stats_part {'sum' if j == 0 else 'sum of squares'} of {int(bad.sum())} (row, slice) pairs outside the "
                                  f"bound, first row {r} slice {sl}: got {float(got[sl, r, j])!r} want {float(w[r, sl])!r}")
                if pad and not torch.isnan(buf[:, N:]).all():
                    fails.add(f"{name}: the padding of the output rows lost its prefill")
                LAUNCHES["cs_gemm_nt_ln non-linear"] += 1
    fails.done()


# ------------------------------------------------------------------------------------------------ cs_gemm_nt_ln_split
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("M,N,K", X.TRIPLES_N32)
def test_split_stream_chain(hip, M, N, K, pad):
    """The residual stream through three folded GEMMs as the tower chains them: fp32 in -> planes, planes -> planes, planes -> fp32 out.
    The planes equal RefOps.split_planes of the exact stream in bits (the hi plane rounds halves away from zero by construction:
    include/clipself_hip.h, "hi[m, n] = y >> 16"), the statistics are the exact sums.  The fourth combination, fp32 in and fp32 out, is
    cs_gemm_nt_ln's (test_folded_layernorm_linear_epilogues) and an argument error here."""
    o = X.operands(M, N, K, seed=400, profile="stats")
    xs = X.split_chain(o, M, N)
    A, B, bias = wide(o["A"], 8 * pad), wide(o["B"], 16 * pad), o["bias"].cuda()
    ln = (o["mean"].cuda(), o["rstd"].cuda(), o["colsum"].cuda())
    S = (N + 63) // 64
    x0 = wide(o["res"], 4 * pad)
    hbuf, hi = blank(M, N, BF, 8 * pad)
    lbuf = torch.full((M, N + 8 * pad), -1, dtype=torch.int16, device="cuda")
    lo = lbuf[:, :N]
    fails = X.Failures()
    for step, x in enumerate(xs[:2]):
        part = torch.full((S, M, 2), NAN, device="cuda")
        hip.gemm_nt_ln_split(A, B, hi, lo, bias, *ln, x_in=x0 if step == 0 else None, stats_part=part)
        h, l = RefOps.split_planes(X.want_f32(x))
        tag = f"split stream [{M},{N},{K}] pad={pad} GEMM {step + 1} ({'fp32' if step == 0 else 'planes'} -> planes)"
        same(fails, tag + " hi", hi, h.cuda(), buf=hbuf)
        same(fails, tag + " lo", lo, l.cuda())
        same(fails, tag + " stats_part[slice*M + row]", part.reshape(S * M, 2), X.exact_stats(x, 64).cuda().reshape(S * M, 2), (M, 2))
        if pad and not bool((lbuf[:, N:] == -1).all()):
            fails.add(tag + ": the padding of the lo plane lost its prefill")
    obuf, out = blank(M, N, F32, 4 * pad)
    hi_before, lo_before = hi.clone(), lo.clone()
    hip.gemm_nt_ln_split(A, B, hi, lo, bias, *ln, x_out=out)
    same(fails, f"split stream [{M},{N},{K}] pad={pad} GEMM 3 (planes -> fp32)", out, X.want_f32(xs[2]).cuda(), buf=obuf)
    if not (torch.equal(hi, hi_before) and torch.equal(lo, lo_before)):
        fails.add(f"split stream [{M},{N},{K}]: fp32 out must only read the planes")
    with pytest.raises(RuntimeError, match="fp32 in and fp32 out is cs_gemm_nt_ln"):
        hip.gemm_nt_ln_split(A, B, hi, lo, bias, *ln, x_in=x0, x_out=out)
    LAUNCHES["cs_gemm_nt_ln_split"] += 3
    fails.done()


# ------------------------------------------------------------------------------------------------ 192-row tiles of the streaming kernel
@pytest.mark.parametrize("M,N,K", X.BM192_SHAPES)
def test_stream_kernel_192_and_256_row_tiles_against_the_exact_reference(hip, M, N, K):
    """The streaming kernel's M >= 192 branch (192-row tiles when they fill the chip better: always at these sizes) and its 256-row form
    (CS_NO_BM192=1, read per launch), each against the exact reference: bf16, fp32 residual and SwiGLU outputs."""
    o = X.operands(M, N, K, seed=800)
    w0 = X.want_bf16(X.exact_gemm(o["A"], o["B"], o["bias"])).cuda()
    w2 = X.want_f32(X.exact_gemm(o["A"], o["B"], o["bias"], o["res"])).cuda()
    a = X.operands(M, N, K, seed=810, profile="act", rows_b=2 * N)
    pre = X.exact_gemm(a["A"], a["B"], a["bias"])
    A, B, bias, res = wide(o["A"], 8), wide(o["B"], 16), o["bias"].cuda(), o["res"].cuda()
    aA, aB, abias = wide(a["A"], 8), wide(a["B"], 16), a["bias"].cuda()
    fails = X.Failures()
    swiglu = {}
    for form in ("192-row", "256-row"):
        if form == "256-row":
            os.environ["CS_NO_BM192"] = "1"
        try:
            for fl in (0xB0,):                                   # bit 12 (slab epilogues) keeps the 256-row form
                tag = f"[{M},{N},{K}] {form} tiles flags={fl:#x}"
                buf, C = blank(M, N, BF, 12)
                hip.gemm_nt(A, B, C, bias, epi=0, flags=fl)
                same(fails, "epi0 " + tag, C, w0, (192 if form == "192-row" else 256, 256), buf)
                buf, C = blank(M, N, F32, 12)
                C.copy_(res)
                hip.gemm_nt(A, B, C, bias, C, epi=2, flags=fl)
                same(fails, "epi2 " + tag, C, w2, (192 if form == "192-row" else 256, 256), buf)
                buf, C = blank(M, N, BF, 12)
                hip.gemm_nt(aA, aB, C, abias, epi=3, group=N, flags=fl)
                act_check(fails, "bm192", "epi3 " + tag, C, pre, 3, N)
                swiglu[(form, fl)] = C
                LAUNCHES["192 / 256-row forms"] += 3
            torch.cuda.synchronize()
        finally:
            os.environ.pop("CS_NO_BM192", None)
    same(fails, f"epi3 [{M},{N},{K}]: 192-row form against the 256-row form", swiglu[("192-row", 0xB0)], swiglu[("256-row", 0xB0)])
    fails.done()


# ------------------------------------------------------------------------------------------------ persistent kernels, more tiles than workgroups
@pytest.mark.parametrize("grid", [16, 24])
@pytest.mark.parametrize("epi", [0, 3])
def test_persistent_tile_loop_with_more_tiles_than_workgroups(hip, epi, grid):
    """30 tiles of 256x256 (M = 1300) on a persistent grid of 16 / 24 workgroups (flags bits 20-27 leave the other compute units free):
    schedule 9 on the grouped raster and raster modes 1, 2 (B-stationary, two N parts), 3; schedule 11 (the streaming kernel, N % 32 == 0)
    with both epilogue forms -- every workgroup walks two tiles, the ragged last row / column tiles among them."""
    reserve = hip.num_compute_units() - grid
    assert 0 < reserve < 256
    M, K = 1300, 128
    fails = X.Failures()
    for sched, (n0, n3) in (((0x90, 0x10290, 0x20290, 0x30090), (1100, 548)), ((0xB0, 0x10B0), (1120, 576))):
        N = n0 if epi == 0 else n3
        if epi == 0:
            o = X.operands(M, N, K, seed=900)
            v = X.exact_gemm(o["A"], o["B"], o["bias"])
            X.assert_rounding_is_tested("persistent", v)
            want = X.want_bf16(v).cuda()
        else:
            o = X.operands(M, N, K, seed=910, profile="act", rows_b=2 * N)
            pre = X.exact_gemm(o["A"], o["B"], o["bias"])
        A, B, bias = wide(o["A"], 8), wide(o["B"], 16), o["bias"].cuda()
        for fl in sched:
            buf, C = blank(M, N, BF, 12)
            hip.gemm_nt(A, B, C, bias, epi=epi, group=N if epi == 3 else 0, flags=fl | (reserve << 20))
            name = f"persistent loop epi{epi} [{M},{N},{K}] grid={grid} flags={fl:#x}"
            if epi == 0:
                same(fails, name, C, want, (256, 256), buf)
            else:
                act_check(fails, "persistent loop", name, C, pre, 3, N)
                if not torch.isnan(buf[:, N:]).all():
                    fails.add(name + ": the padding of the output rows lost its prefill")
            LAUNCHES["persistent tile loop"] += 1
    fails.done()


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("M,N,K", X.WGRAD_SHAPES)
def test_wgrad_split_through_partials(hip, M, N, K):
    """cs_gemm_wgrad: dW (pre-filled with integers: the call accumulates) += A.B^T over 1, 2, 3 and 13 K tiles, into a strided destination
    whose padding keeps its prefill; twice, for bit-reproducibility."""
    A, B, base = X.int_bf16((M, K), 3, 500), X.int_bf16((N, K), 2, 501), X.int_f32((M, N), 1000, 502)
    want = X.want_f32(X.exact_gemm(A, B, None, base)).cuda()
    ws = torch.empty(hip.gemm_wgrad_workspace(M, N, K), dtype=torch.uint8, device="cuda")
    Ad, Bd = wide(A, 8), wide(B, 16)
    fails = X.Failures()
    outs = []
    for rep in range(2):
        for pad in (0, 12):
            buf, dW = blank(M, N, F32, pad)
            dW.copy_(base)
            hip.gemm_wgrad(Ad, Bd, dW, ws)
            same(fails, f"wgrad [{M},{N},{K}] ldc=N+{pad} run {rep}", dW, want, (128, 128), buf)
            outs.append(dW)
            LAUNCHES["cs_gemm_wgrad"] += 1
    if not all(torch.equal(outs[0], t) for t in outs[1:]):
        fails.add(f"wgrad [{M},{N},{K}]: not bit-reproducible")
    fails.done()


@pytest.mark.parametrize("T,N,K", X.WGRAD_TN_SHAPES)
def test_wgrad_token_major(hip, T, N, K):
    """cs_gemm_wgrad_tn: dW[N, K] += dY^T X from token-major operands: token counts below / at / past the 64-token tile (the zeroed last token
    tile), widths below / at / past 256 (the ragged re-read), strided operands and destination, twice."""
    dY, Xt, base = X.int_bf16((T, N), 3, 510), X.int_bf16((T, K), 2, 511), X.int_f32((N, K), 1000, 512)
    want = X.want_f32(X.exact_gemm(dY.T, Xt.T, None, base)).cuda()
    need = hip.gemm_wgrad_tn_workspace(N, K, T)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    fails = X.Failures()
    outs = []
    for rep in range(2):
        for pad in (0, 1):
            dYd, Xd = wide(dY, 8 * pad), wide(Xt, 16 * pad)
            buf, dW = blank(N, K, F32, 12 * pad)
            dW.copy_(base)
            hip.gemm_wgrad_tn(dYd, Xd, dW, ws)
            same(fails, f"wgrad_tn tokens={T} [{N},{K}] pad={pad} run {rep}", dW, want, (256, 256), buf)
            outs.append(dW)
            LAUNCHES["cs_gemm_wgrad_tn"] += 1
    if not all(torch.equal(outs[0], t) for t in outs[1:]):
        fails.add(f"wgrad_tn tokens={T} [{N},{K}]: not bit-reproducible")
    fails.done()


# ------------------------------------------------------------------------------------------------ fp8
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("M,N,K8", X.F8_SHAPES)
def test_fp8_gemm(hip, M, N, K8, pad):
    """cs_gemm_nt_f8 on e4m3 codes of small integers with power-of-two row / column scales: epilogues 0 and 2 (in place), bit for bit."""
    A8, B8 = X.e4m3_codes((M, K8), 3, 600), X.e4m3_codes((N, K8), 2, 601)
    rs, cs, bias, res = X.pow2_f32(M, 602), X.pow2_f32(N, 603), X.int_f32((N,), 1000, 604), X.int_f32((M, N), 1000, 605)
    v = X.exact_gemm(A8, B8, bias, scales=(rs, cs))
    X.assert_rounding_is_tested(f"f8[{M},{N},{K8}]", v)
    w0 = X.want_bf16(v).cuda()
    w2 = X.want_f32(X.exact_gemm(A8, B8, bias, res, scales=(rs, cs))).cuda()
    Ad, Bd = wide(A8, 16 * pad), wide(B8, 32 * pad)                    # padding bytes 0xFF: the e4m3 NaN
    fails = X.Failures()
    buf, C = blank(M, N, BF, 12 * pad)
    hip.gemm_nt_f8(Ad, Bd, C, rs.cuda(), cs.cuda(), bias=bias.cuda(), epi=0)
    same(fails, f"f8 epi0 [{M},{N},{K8}] pad={pad}", C, w0, (256, 256), buf)
    buf, C = blank(M, N, F32, 12 * pad)
    C.copy_(res.cuda())
    hip.gemm_nt_f8(Ad, Bd, C, rs.cuda(), cs.cuda(), bias=bias.cuda(), extra=C, epi=2)
    same(fails, f"f8 epi2 in place [{M},{N},{K8}] pad={pad}", C, w2, (256, 256), buf)
    LAUNCHES["cs_gemm_nt_f8"] += 2
    fails.done()


def test_fp8_quantiser_on_rows_whose_amax_is_a_power_of_two_times_448(hip):
    """cs_quant_rows_fp8 spot check: there the scale 2^k is exact and the codes are the integers themselves; the K padding is zero."""
    x, codes, scale = X.fp8_quant_case(37, 200, 610)
    q, s = torch.full((37, 256), 0x55, dtype=torch.uint8, device="cuda"), torch.full((37,), NAN, device="cuda")
    hip.quant_rows_fp8(x.cuda(), q, s)
    X.assert_bits_equal("quant_rows_fp8 codes", q, codes, (37, 128))
    X.assert_bits_equal("quant_rows_fp8 scales", s, scale)
    LAUNCHES["cs_quant_rows_fp8"] += 1
