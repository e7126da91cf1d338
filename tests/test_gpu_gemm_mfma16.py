"""`-m gpu`: the frozen tower's folded-LayerNorm GEMMs on the streaming kernel's two K-loop forms -- v_mfma_f32_16x16x32_bf16 (the default)
and v_mfma_f32_32x32x16_bf16 (CS_GEMM_MFMA32=1) -- held to the same checks:

  * exactly representable operands (tests/_exact_gemm.py): every element bit for bit against the float64 value, NaN-prefilled outputs
    inside wider rows whose padding and tail must keep their prefill;
  * the SwiGLU epilogue on an exact pre-activation: per element against the float64 activation (the bound of tests/test_gpu_gemm_exact.py),
    its statistics partials per (32-unit slice, row) against the float64 moments of the kernel's own rounded outputs;
  * random operands against the float64 reference under TOL_BF of tests/test_gpu_ops.py, the partials under the per-row bound of
    tests/test_gpu_ln_cond.py (_ln_cond.partial_bounds).

Shapes: K = 64 (only the first, zero-accumulating K tile), 128 and 192 (an odd number of K tiles walks the 3-slot / 2-slot rings out of
phase); M = 1, 17, 255, 257 (ragged row tiles, the 16-row block boundary); N = 96, 288 (ragged column tiles); and M = 7500, N = 2304: 270
tiles, more than the persistent grid, so a workgroup carries the operand ring across an epilogue.  SwiGLU: hidden widths 96 and 160 (ragged
column tiles, waves whose 32 units lie past the width) and M = 4353 with 2048 hidden units (18 x 16 tiles)."""
import os

import pytest
import torch

import _exact_gemm as X
import _ln_cond as L
from _exact_gemm import BF
from test_gpu_ops import TOL_BF, rel

pytestmark = pytest.mark.gpu

NAN = float("nan")
STREAM = 0xB0                                   # flags: the streaming kernel, whatever the shape
SMALL = [(1, 96, 64), (17, 288, 128), (255, 96, 192), (257, 288, 192), (257, 96, 64), (17, 96, 192), (255, 288, 128), (1, 288, 192)]
BIG = (7500, 2304, 192)
FORMS = ["mfma16", "mfma32"]


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def in_form(form, fn):
    """fn() with the K loop of `form`: the switch is read at every launch."""
    try:
        if form == "mfma32":
            os.environ["CS_GEMM_MFMA32"] = "1"
        return fn()
    finally:
        os.environ.pop("CS_GEMM_MFMA32", None)


def poisoned(rows, cols, pad, tail=3):
    """NaN-filled [rows + tail, cols + pad]; the kernel is given the [rows, cols] corner."""
    buf = torch.full((rows + tail, cols + pad), NAN, dtype=BF, device="cuda")
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols):
    return bool(torch.isnan(buf[:rows, cols:]).all()) and bool(torch.isnan(buf[rows:]).all())


_exact_cache = {}


def exact_case(M, N, K, fold):
    """Operands and the bf16 image of the exact value, computed once per case and shared by the two forms."""
    key = (M, N, K, fold)
    if key not in _exact_cache:
        o = X.operands(M, N, K, seed=700 + (1 if fold else 0))
        if fold:
            ln = (o["mean"], o["rstd"], o["colsum"])
        else:
            ln = (torch.zeros(M), torch.ones(M), torch.zeros(N))
        v = X.exact_gemm(o["A"], o["B"], o["bias"], ln=ln)
        _exact_cache[key] = (o, ln, X.want_bf16(v))
    return _exact_cache[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fold", [False, True], ids=["identity", "folded"])
@pytest.mark.parametrize("M,N,K", SMALL + [BIG])
def test_exact_operands_bf16_bit_for_bit(hip, M, N, K, fold, form):
    o, ln, want = exact_case(M, N, K, fold)
    Abuf = torch.full((M, K + 8), NAN, dtype=BF, device="cuda")
    Bbuf = torch.full((N, K + 16), NAN, dtype=BF, device="cuda")
    Abuf[:, :K], Bbuf[:, :K] = o["A"].cuda(), o["B"].cuda()
    lnd = dict(ln_mean=ln[0].cuda(), ln_rstd=ln[1].cuda(), ln_colsum=ln[2].cuda())
    buf, C = poisoned(M, N, 24)
    in_form(form, lambda: hip.gemm_nt_ln(Abuf[:, :K], Bbuf[:, :K], C, bias=o["bias"].cuda(), epi=0, flags=STREAM, **lnd))
    X.assert_bits_equal(f"{form} ln epi0 [{M},{N},{K}] fold={fold}", C.cpu(), want)
    assert untouched(buf, M, N), "the padding (ldc > N) or the tail rows of the output lost their prefill"


_random_cache = {}


def random_case(M, N, K):
    if (M, N, K) not in _random_cache:
        g = torch.Generator().manual_seed(41)
        A = (torch.randn(M, K, generator=g) * 1.5 + 0.25).to(BF)
        B = (torch.randn(N, K, generator=g) * 0.05).to(BF)
        bias = torch.randn(N, generator=g)
        a64 = A.double()
        mean, rstd = a64.mean(-1), 1.0 / (a64.var(-1, unbiased=False) + 1e-6).sqrt()
        colsum = B.double().sum(-1)
        mean, rstd, colsum = mean.float(), rstd.float(), colsum.float()
        want = rstd.double()[:, None] * (a64 @ B.double().T - mean.double()[:, None] * colsum.double()[None, :]) + bias.double()
        _random_cache[(M, N, K)] = (A, B, bias, mean, rstd, colsum, want)
    return _random_cache[(M, N, K)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("epi", [0, 8])
@pytest.mark.parametrize("M,N,K", [(257, 288, 192), (3000, 768, 768)])
def test_random_operands_bf16_against_float64(hip, M, N, K, epi, form):
    A, B, bias, mean, rstd, colsum, want = random_case(M, N, K)
    if epi == 8:
        want = want * torch.sigmoid(1.702 * want)
    buf, C = poisoned(M, N, 8)
    in_form(form, lambda: hip.gemm_nt_ln(A.cuda(), B.cuda(), C, bias=bias.cuda(), ln_mean=mean.cuda(), ln_rstd=rstd.cuda(), ln_colsum=colsum.cuda(),
                                         epi=epi, flags=STREAM))
    assert torch.isfinite(C.float()).all()
    r = rel(C, want)
    print(f"{form} epi{epi} [{M},{N},{K}]: rel {r:.3e} (bound {TOL_BF:.1e})")
    assert r <= TOL_BF
    assert untouched(buf, M, N)


# ------------------------------------------------------------------------------------------------ SwiGLU (+ statistics partials)
SWI_SMALL = [(1, 96, 64), (17, 160, 128), (255, 96, 192), (257, 160, 192), (257, 96, 64), (17, 96, 192), (255, 160, 128), (1, 160, 192)]
SWI_BIG = (4353, 2048, 192)
_swi_cache = {}


def swi_case(M, G, K):
    if (M, G, K) not in _swi_cache:
        _swi_cache[(M, G, K)] = X.act_case(M, G, K, 900, 3, fold=True)
    return _swi_cache[(M, G, K)]


def partials_of(h):
    """float64 (sum, sum of squares, sum of magnitudes) of the 32-unit slices of the kernel's own output h [M, G]: [G / 32, M, 3]"""
    return L.slice_partials64(h.detach().cpu(), 32)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("M,G,K", SWI_SMALL + [SWI_BIG])
def test_exact_preactivation_swiglu_and_partials(hip, M, G, K, stats, form):
    a = swi_case(M, G, K)
    Abuf = torch.full((M, K + 8), NAN, dtype=BF, device="cuda")
    Bbuf = torch.full((2 * G, K + 16), NAN, dtype=BF, device="cuda")
    Abuf[:, :K], Bbuf[:, :K] = a["A"].cuda(), a["B"].cuda()
    lnd = dict(ln_mean=a["mean"].cuda(), ln_rstd=a["rstd"].cuda(), ln_colsum=a["colsum"].cuda())
    P = 4 * ((G + 127) // 128)
    live = G // 32
    buf, C = poisoned(M, G, 24)
    pbuf = torch.full((P * M + 5, 2), NAN, device="cuda")
    part = pbuf[:P * M].view(P, M, 2) if stats else None
    in_form(form, lambda: hip.gemm_nt_ln(Abuf[:, :K], Bbuf[:, :K], C, bias=a["bias"].cuda(), stats_part=part, epi=3, group=G, flags=STREAM, **lnd))
    name = f"{form} ln epi3 [{M},{G},{K}] stats={stats}"
    msg, _ = X.activation_mismatch(name, C, a["pre_ln"], 3, G)
    assert msg is None, msg
    assert untouched(buf, M, G), "the padding (ldc > group) or the tail rows of the output lost their prefill"
    if not stats:
        assert torch.isnan(pbuf).all()
        return
    # sums of the kernel's own rounded outputs: 32 fp32 additions, one more rounding for the square (tests/test_gpu_gemm_exact.py)
    p64 = partials_of(C)
    got = part.cpu().double()[:live]
    assert ((got[:, :, 0] - p64[:, :, 0]).abs() <= 32 * 2.0 ** -24 * p64[:, :, 2]).all(), name + ": sums"
    assert ((got[:, :, 1] - p64[:, :, 1]).abs() <= 33 * 2.0 ** -24 * p64[:, :, 1]).all(), name + ": sums of squares"
    assert torch.isnan(pbuf[P * M:]).all(), "the tail of stats_part lost its prefill"
    assert torch.isfinite(part[:live]).all()                # every slice of the problem is written (those past the hidden width are ignored)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,G,K", [(257, 160, 192), (3000, 384, 768)])
def test_random_operands_swiglu_against_float64(hip, M, G, K, form):
    g = torch.Generator().manual_seed(43)
    A = (torch.randn(M, K, generator=g) * 1.5 + 0.25).to(BF)
    B = (torch.randn(2 * G, K, generator=g) * 0.05).to(BF)
    bias = torch.randn(2 * G, generator=g) * 0.5
    a64 = A.double()
    mean, rstd = a64.mean(-1).float(), (1.0 / (a64.var(-1, unbiased=False) + 1e-6).sqrt()).float()
    colsum = B.double().sum(-1).float()
    pre = rstd.double()[:, None] * (a64 @ B.double().T - mean.double()[:, None] * colsum.double()[None, :]) + bias.double()
    want = X.act64(pre, 3, G)
    P = 4 * ((G + 127) // 128)
    buf, C = poisoned(M, G, 8)
    part = torch.full((P, M, 2), NAN, device="cuda")
    in_form(form, lambda: hip.gemm_nt_ln(A.cuda(), B.cuda(), C, bias=bias.cuda(), ln_mean=mean.cuda(), ln_rstd=rstd.cuda(), ln_colsum=colsum.cuda(),
                                         stats_part=part, epi=3, group=G, flags=STREAM))
    assert torch.isfinite(C.float()).all()
    r = rel(C, want)
    print(f"{form} epi3 [{M},{G},{K}]: rel {r:.3e} (bound {TOL_BF:.1e})")
    assert r <= TOL_BF
    assert untouched(buf, M, G)
    p64 = partials_of(C)
    bs, bq = L.partial_bounds(p64, 32)
    got = part.cpu().double()[:G // 32]
    es, eq = (got[:, :, 0] - p64[:, :, 0]).abs(), (got[:, :, 1] - p64[:, :, 1]).abs()
    print(f"{form} partials: worst error/bound sum {float((es / bs.clamp_min(1e-300)).max()):.3e} sumsq {float((eq / bq.clamp_min(1e-300)).max()):.3e}")
    assert (es <= bs).all() and (eq <= bq).all()
