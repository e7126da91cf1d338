"""`-m gpu`: every HIP kernel behind the C ABI, in isolation, against its CPU reference (oracle/ops_ref.py) on
identical seeded inputs.  Tolerances: bf16 outputs <= 4e-3 relative L2 (1 bf16 ulp = 3.9e-3 element-wise; only
rounding flips differ), fp32 outputs <= 2e-5.  Metrics are appended to gpurun_out/ops_metrics.txt."""
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.ops_ref import RefOps  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
TOL_BF, TOL_F32 = 4e-3, 2e-5
_LOG = Path(__file__).resolve().parent.parent / "gpurun_out" / "ops_metrics.txt"


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOps()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _metric(line):
    _LOG.parent.mkdir(exist_ok=True)
    with open(_LOG, "a") as f:
        f.write(line + "\n")


def check(name, got, want, tol):
    r = rel(got, want)
    bad = not torch.isfinite(got.float()).all().item()
    _LOG.parent.mkdir(exist_ok=True)
    with open(_LOG, "a") as f:
        f.write(f"{name}: rel={r:.3e} tol={tol:.1e} {'NONFINITE' if bad else ''}\n")
    assert not bad, f"{name}: non-finite output"
    assert r <= tol, f"{name}: rel {r:.3e} > {tol:.1e}"


def rnd(shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def both(cpu_tensors):
    return [t.cuda() if t is not None else None for t in cpu_tensors]


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("flags", [0, 1, 0x10, 0x20, 0x30, 0x31, 0x70, 0x71, 0x8070, 0x90, 0xB0, 0x10B0])      # heuristic, register staging, forced 128x128 / 256x128 / 256x256 / split rings (+ burst DMA) / persistent / streaming (+ slab epilogue)
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (3152, 768, 768), (300, 192, 64), (128, 64, 256), (1000, 2304, 768)])
def test_gemm_bf16_bias(hip, ref, M, N, K, flags):
    A, B, bias = rnd((M, K), BF, seed=1), rnd((N, K), BF, 0.05, seed=2), rnd((N,), F32, seed=3)
    Cr = torch.empty(M, N, dtype=BF)
    ref.gemm_nt(A, B, Cr, bias, epi=0)
    Ad, Bd, bd = both([A, B, bias])
    Cd = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt(Ad, Bd, Cd, bd, epi=0, flags=flags)
    check(f"gemm_bf16[{M},{N},{K}] flags={flags}", Cd, Cr, TOL_BF)


@pytest.mark.parametrize("flags", [0, 1, 0x10, 0x20, 0x30, 0x70, 0x71, 0x90, 0xB0, 0x10B0])
def test_gemm_f32_resid_strided(hip, ref, flags):
    M, N, K = 788, 768, 2048
    Abig = rnd((M, K + 64), BF, seed=4)
    A = Abig[:, :K]                                    # lda != K
    B, bias, res = rnd((N, K), BF, 0.03, seed=5), rnd((N,), F32, seed=6), rnd((M, N), F32, seed=7)
    Cr = torch.empty(M, N)
    ref.gemm_nt(A, B, Cr, bias, res, epi=2)
    Abd = Abig.cuda()
    Cd = res.cuda().clone()
    hip.gemm_nt(Abd[:, :K], B.cuda(), Cd, bias.cuda(), Cd, epi=2, flags=flags)   # in-place residual
    check(f"gemm_resid_inplace flags={flags}", Cd, Cr, TOL_F32)
    Cr2 = torch.empty(M, N)
    ref.gemm_nt(A, B, Cr2, None, epi=1)
    Cd2 = torch.empty(M, N, device="cuda")
    hip.gemm_nt(Abd[:, :K], B.cuda(), Cd2, None, epi=1, flags=flags)
    check(f"gemm_f32_nobias flags={flags}", Cd2, Cr2, TOL_F32)


@pytest.mark.parametrize("M,N,K", [(12608, 768, 768), (12608, 768, 2048), (12608, 768, 4096), (1000, 768, 256), (200, 256, 64), (12608, 4096, 768)])
def test_gemm_192_row_tiles_equal_256_row_tiles_bit_for_bit(hip, M, N, K):
    """Round 4: the streaming kernel's 192-row tile form (taken when the 256-row tiling fills the chip badly: the student's N = 768 GEMMs at
    12 608 rows run 198 tiles instead of 150) accumulates every element in the same order: bf16, fp32-residual and
    SwiGLU outputs equal the 256-row form (CS_NO_BM192=1) bit for bit."""
    import os
    A = rnd((M, K), BF, seed=60).cuda()
    W = rnd((N, K), BF, 0.1, seed=61).cuda()
    bias = rnd((N,), F32, 0.5, seed=62).cuda()
    x0 = rnd((M, N), F32, seed=63).cuda()

    def run():
        out = {}
        c = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
        hip.gemm_nt(A, W, c, bias, epi=0)
        out["bf16"] = c
        r = x0.clone()
        hip.gemm_nt(A, W, r, bias, extra=r, epi=2)
        out["resid"] = r
        h = torch.full((M, N // 2), float("nan"), dtype=BF, device="cuda")
        hip.gemm_nt(A, W, h, bias, epi=3, group=N // 2)
        out["swiglu"] = h
        torch.cuda.synchronize()
        return out

    try:
        os.environ["CS_NO_BM192"] = "1"
        want = run()
    finally:
        os.environ.pop("CS_NO_BM192", None)
    got = run()
    assert set(got) == set(want)
    for k in want:
        a, b = got[k], want[k]
        v = torch.int16 if a.element_size() == 2 else torch.int32
        assert torch.equal(a.view(v), b.view(v)), f"{k} [{M},{N},{K}]"
    check(f"gemm192.bf16[{M},{N},{K}]", got["bf16"], (A.float() @ W.float().T + bias).cpu(), TOL_BF)


@pytest.mark.parametrize("flags", [0, 0x10, 0x20, 0x30, 0x70, 0x71, 0x8070, 0x90, 0xB0, 0x10B0])
@pytest.mark.parametrize("Hd,M", [(2048, 394), (256, 34), (96, 130)])
def test_gemm_swiglu(hip, ref, Hd, M, flags):
    K = 128
    A, W, bias = rnd((M, K), BF, seed=8), rnd((2 * Hd, K), BF, 0.1, seed=9), rnd((2 * Hd,), F32, 0.5, seed=10)
    Cr = torch.empty(M, Hd, dtype=BF)
    ref.gemm_nt(A, W, Cr, bias, epi=3, group=Hd)
    Cd = torch.full((M, Hd), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt(A.cuda(), W.cuda(), Cd, bias.cuda(), epi=3, group=Hd, flags=flags)
    check(f"gemm_swiglu[{M},{Hd}] flags={flags}", Cd, Cr, TOL_BF)


def test_gemm_splitk_atomic_wgrad_shape(hip, ref):
    # wgrad form: dW[N,K] += dY^T[N,Mp] . X^T[K,Mp]^T with a long contraction split 7 ways
    N, Kd, Mp = 768, 256, 3200
    A, B = rnd((N, Mp), BF, seed=11), rnd((Kd, Mp), BF, seed=12)
    base = rnd((N, Kd), F32, seed=13)
    Cr = base.clone()
    ref.gemm_nt(A, B, Cr, epi=4)
    for flags in (0, 0x10, 0x20, 0x30, 0x70):
        Cd = base.cuda()
        hip.gemm_nt(A.cuda(), B.cuda(), Cd, epi=4, splits=7, flags=flags)
        check(f"gemm_splitk_atomic flags={flags}", Cd, Cr, TOL_F32)


def test_removed_schedules_and_ablation_bits_are_not_reachable(hip, ref):
    """Round 3 removed the schedules that lost every measurement (3-stage ring 4, ping-pong 5 / 10, L2 warm-up 6, two workgroups per CU 8):
    asking for one is an argument error, not a silent fallback.  The timing-ablation bits (flags bits 13-14: skip the MFMA loop / the
    epilogue, mask the stores -- wrong results by construction) are compiled out of the shipped library: setting them changes nothing."""
    M, N, K = 300, 192, 128
    A, B, bias = rnd((M, K), BF, seed=1), rnd((N, K), BF, seed=2), rnd((N,), F32, seed=3)
    Cr = torch.empty(M, N, dtype=BF)
    ref.gemm_nt(A, B, Cr, bias, epi=0)
    for cfg in (4, 5, 6, 8, 10, 12):
        with pytest.raises(RuntimeError, match="does not exist"):
            hip.gemm_nt(A.cuda(), B.cuda(), torch.empty(M, N, dtype=BF, device="cuda"), bias.cuda(), epi=0, flags=cfg << 4)
    for cfg in (0x30, 0x70, 0x90, 0xB0):
        for abl in (0x2000, 0x4000, 0x6000, 0x8000 if cfg == 0xB0 else 0):
            Cd = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
            hip.gemm_nt(A.cuda(), B.cuda(), Cd, bias.cuda(), epi=0, flags=cfg | abl)
            check(f"ablation bits ignored cfg={cfg:#x} abl={abl:#x}", Cd, Cr, TOL_BF)


@pytest.mark.parametrize("N,Kd,Mp", [(768, 256, 3200), (2304, 768, 12672), (128, 64, 64), (4096, 768, 1280), (300, 192, 640)])
def test_gemm_wgrad_split_through_partials(hip, ref, N, Kd, Mp):
    """cs_gemm_wgrad: dW += dY^T . X through split-K partial buffers + one reduction pass (no atomics: bit-reproducible)."""
    A, B = rnd((N, Mp), BF, seed=60), rnd((Kd, Mp), BF, seed=61)
    base = rnd((N, Kd), F32, seed=62)
    Cr = base.clone()
    ref.gemm_wgrad(A, B, Cr, None)
    ws = torch.empty(hip.gemm_wgrad_workspace(N, Kd, Mp), dtype=torch.uint8, device="cuda")
    Cd = base.cuda()
    hip.gemm_wgrad(A.cuda(), B.cuda(), Cd, ws)
    check(f"gemm_wgrad[{N},{Kd},{Mp}]", Cd, Cr, TOL_F32)
    Cd2 = base.cuda()
    hip.gemm_wgrad(A.cuda(), B.cuda(), Cd2, ws)
    assert torch.equal(Cd, Cd2)
    # strided destination (a slice of the flat grad buffer viewed with a wider row)
    wide = torch.zeros(N, Kd + 64, device="cuda")
    hip.gemm_wgrad(A.cuda(), B.cuda(), wide[:, :Kd], ws)
    check(f"gemm_wgrad_strided[{N},{Kd},{Mp}]", wide[:, :Kd] + base.cuda(), Cr, TOL_F32)
    assert float(wide[:, Kd:].abs().sum()) == 0.0


def test_gemm_patch_epilogue(hip, ref):
    nimg, G, N, K = 5, 16, 128, 192
    A, W, bias = rnd((nimg * G, K), BF, seed=14), rnd((N, K), BF, 0.1, seed=15), rnd((N,), F32, seed=16)
    pos = rnd((G + 1, N), F32, seed=17)
    Cr = torch.zeros(nimg * (G + 1), N)
    ref.gemm_nt(A, W, Cr, bias, pos, epi=5, group=G)
    for flags in (0x10, 0x20, 0x30, 0):
        Cd = torch.zeros(nimg * (G + 1), N, device="cuda")
        hip.gemm_nt(A.cuda(), W.cuda(), Cd, bias.cuda(), pos.cuda(), epi=5, group=G, flags=flags)
        check(f"gemm_patch flags={flags}", Cd, Cr, TOL_F32)
    cls = rnd((N,), F32, seed=18)
    xr, xd = Cr.reshape(nimg, G + 1, N), Cd.reshape(nimg, G + 1, N)
    ref.cls_row(xr, cls, pos)
    hip.cls_row(xd, cls.cuda(), pos.cuda())
    check("cls_row", xd, xr, TOL_F32)


# ------------------------------------------------------------------------------------------------ LayerNorm / L2
@pytest.mark.parametrize("C", [128, 768, 2048, 2732])
@pytest.mark.parametrize("xdt", [F32, BF])
def test_layernorm_fwd_bwd(hip, ref, C, xdt):
    M = 523
    x = (rnd((M, C), F32, 2.0, seed=20) + 0.5).to(xdt)
    gamma, beta = 1 + rnd((C,), F32, 0.2, seed=21), rnd((C,), F32, 0.2, seed=22)
    dy = rnd((M, C), BF, seed=23)
    yr, mr, rr = torch.empty(M, C, dtype=BF), torch.empty(M), torch.empty(M)
    ref.layernorm_fwd(x, gamma, beta, yr, mr, rr)
    xd, gd, bd, dyd = both([x, gamma, beta, dy])
    yd, md, rd = torch.empty(M, C, dtype=BF, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    hip.layernorm_fwd(xd, gd, bd, yd, md, rd)
    tag = f"ln[{C},{'f32' if xdt == F32 else 'bf16'}]"
    check(tag + ".y", yd, yr, TOL_BF)
    check(tag + ".mean", md, mr, TOL_F32)
    check(tag + ".rstd", rd, rr, TOL_F32)
    ws = torch.empty(hip.layernorm_bwd_workspace(M, C), dtype=torch.uint8, device="cuda")
    for mode, odt in ((0, BF), (1, F32), (2, F32)):
        base = rnd((M, C), F32, seed=24).to(odt)
        dxr, dgr, dbr = base.clone(), torch.zeros(C), torch.zeros(C)
        ref.layernorm_bwd(dy, x, gamma, mr, rr, dxr, mode, dgr, dbr)
        dxd, dgd, dbd = base.cuda(), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        hip.layernorm_bwd(dyd, xd, gd, md, rd, dxd, mode, dgd, dbd, False, ws)
        check(f"{tag}.dx{mode}", dxd, dxr, TOL_BF if odt == BF else 1e-4)
        check(f"{tag}.dgamma{mode}", dgd, dgr, 1e-4)
        check(f"{tag}.dbeta{mode}", dbd, dbr, 1e-4)
    # frozen LN: no param grads requested
    dxd = torch.empty(M, C, device="cuda")
    hip.layernorm_bwd(dyd, xd, gd, md, rd, dxd, 1)
    dxr = torch.empty(M, C)
    ref.layernorm_bwd(dy, x, gamma, mr, rr, dxr, 1)
    check(tag + ".dx_frozen", dxd, dxr, 1e-4)
    # fp32 stream modes with the bf16 copy of the updated rows and its column sums (the bias gradient that used to need a cast + a
    # column-sum pass): copy == bf16(dx) exactly, sums == fp32 column sums of the copy, accumulated onto what was there; with and
    # without parameter gradients; bit-reproducible
    for mode in (1, 2):
        for with_params in (True, False):
            base, cs0 = rnd((M, C), F32, seed=25), rnd((C,), F32, seed=26)
            dxd, cpy, csd = base.cuda(), torch.full((M, C), float("nan"), dtype=BF, device="cuda"), cs0.cuda()
            dgd, dbd = (torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")) if with_params else (None, None)
            hip.layernorm_bwd(dyd, xd, gd, md, rd, dxd, mode, dgd, dbd, True, ws, dx_copy=cpy, copy_colsum=csd)
            dxr, dgr, dbr, cpr, csr = base.clone(), torch.zeros(C), torch.zeros(C), torch.empty(M, C, dtype=BF), cs0.clone()
            ref.layernorm_bwd(dy, x, gamma, mr, rr, dxr, mode, dgr, dbr, True, None, dx_copy=cpr, copy_colsum=csr)
            check(f"{tag}.copy.dx{mode}", dxd, dxr, 1e-4)
            assert torch.equal(cpy, dxd.to(BF)), f"{tag}: the copy is the rounded stream"
            check(f"{tag}.copy.colsum{mode}", csd - cs0.cuda(), cpy.float().sum(0), 1e-4)
            if with_params:
                check(f"{tag}.copy.dgamma{mode}", dgd, dgr, 1e-4)
            dx2, cp2, cs2 = base.cuda(), torch.empty_like(cpy), cs0.cuda()
            hip.layernorm_bwd(dyd, xd, gd, md, rd, dx2, mode, None, None, True, ws, dx_copy=cp2, copy_colsum=cs2)
            assert torch.equal(cs2, csd) and torch.equal(cp2, cpy)


def test_layernorm_strided_rows(hip, ref):
    # CLS rows of a [B, N, C] stream (teacher: final norm on token 0 only), ldx = N*C
    B, N, C = 9, 17, 128
    x = rnd((B, N, C), F32, seed=25)
    gamma, beta = 1 + rnd((C,), F32, 0.2, seed=26), rnd((C,), F32, 0.2, seed=27)
    yr = torch.empty(B, C, dtype=BF)
    ref.layernorm_fwd(x[:, 0, :], gamma, beta, yr)
    xd = x.cuda()
    yd = torch.empty(B, C, dtype=BF, device="cuda")
    hip.layernorm_fwd(xd[:, 0, :], gamma.cuda(), beta.cuda(), yd)
    check("ln_strided_cls", yd, yr, TOL_BF)


def test_l2norm(hip, ref):
    M, C = 777, 512
    x, dy = rnd((M, C), F32, seed=28), rnd((M, C), F32, seed=29)
    x[5] = 0.0                                        # zero row -> eps clamp
    yr, ir, dxr = torch.empty(M, C), torch.empty(M), torch.empty(M, C, dtype=BF)
    ref.l2norm_fwd(x, yr, ir)
    ref.l2norm_bwd(dy, yr, ir, dxr)
    yd, idv, dxd = torch.empty(M, C, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, C, dtype=BF, device="cuda")
    hip.l2norm_fwd(x.cuda(), yd, idv)
    hip.l2norm_bwd(dy.cuda(), yd, idv, dxd)
    check("l2norm.y", yd, yr, TOL_F32)
    mask = torch.ones(M, dtype=torch.bool); mask[5] = False
    check("l2norm.inv", idv.cpu()[mask], ir[mask], TOL_F32)
    check("l2norm.dx", dxd.cpu()[mask], dxr[mask], TOL_BF)


# ------------------------------------------------------------------------------------------------ attention
def _rope(Ntok, seed):
    from oracle.eva_ref import rope_tables
    g = int(round((Ntok - 1) ** 0.5))
    assert g * g == Ntok - 1
    return rope_tables(g, 64)


@pytest.mark.parametrize("B,Ntok,H,qscale", [(2, 197, 12, 1.0), (3, 17, 2, 3.0), (2, 65, 2, 2.0), (1, 577, 3, 1.5), (2, 197, 2, 6.0), (2, 226, 2, 1.0), (1, 257, 3, 2.0),
                                              (1, 401, 2, 1.0),       # 226 / 257 / 401: one key / 33 keys / a ragged chunk past the first 224-key image (multiscale grids)
                                              (1, 785, 2, 1.0), (1, 785, 2, 4.0), (1, 4097, 2, 1.0), (1, 4097, 2, 3.0), (2, 1025, 3, 1.0)])
                                              # round 6: the 224-key-chunk kernels at 4 / 5 / 19 chunks (448^2, 512^2 and the recipe's 1024^2 student), flat and peaky
                                              # softmax, dQ / dK / dV against RefOps.attn_bwd -- until round 5 these lengths were only compared with the round-1 kernels
def test_attention_fwd_bwd(hip, ref, B, Ntok, H, qscale):
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=30)
    qkv[:, :2 * C] *= qscale                           # peaky softmax for the larger scales
    qkv = qkv.to(BF)
    cos, sin = _rope(Ntok, 0)
    scale = 64 ** -0.5
    dout = rnd((B * Ntok, C), BF, seed=31)
    o_r, lse_r = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
    ref.attn_fwd(qkv, cos, sin, o_r, lse_r, B, Ntok, H, scale)
    qd, cd, sd, dd = both([qkv, cos, sin, dout])
    o_d = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
    lse_d = torch.empty(B * H, Ntok, device="cuda")
    hip.attn_fwd(qd, cd, sd, o_d, lse_d, B, Ntok, H, scale)
    tag = f"attn[{B},{Ntok},{H},x{qscale}]"
    check(tag + ".o", o_d, o_r, 4e-3)                  # measured <= 2.4e-3 (4097 tokens), round 6: profiles/r06_parity.md
    check(tag + ".lse", lse_d, lse_r, 1e-4)            # measured <= 2.8e-6
    # inference variant (no lse)
    o_d2 = torch.empty_like(o_d)
    hip.attn_fwd(qd, cd, sd, o_d2, None, B, Ntok, H, scale)
    assert torch.equal(o_d2, o_d)
    # backward: both sides start from the reference forward's o / lse so only the bwd kernels are compared
    dq_r = torch.zeros(B * Ntok, 3 * C, dtype=BF)
    ref.attn_bwd(qkv, o_r, dout, lse_r, cos, sin, dq_r, None, B, Ntok, H, scale)
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
    dq_d = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF, device="cuda")
    hip.attn_bwd(qd, o_r.cuda(), dd, lse_r.cuda(), cd, sd, dq_d, ws, B, Ntok, H, scale)
    check(tag + ".dq", dq_d[:, :C], dq_r[:, :C], 1e-3)              # measured <= 2.4e-4 on all 13 shapes (bf16 outputs of fp32 accumulators)
    check(tag + ".dk", dq_d[:, C:2 * C], dq_r[:, C:2 * C], 1e-3)
    check(tag + ".dv", dq_d[:, 2 * C:], dq_r[:, 2 * C:], 1e-3)


@pytest.mark.parametrize("Ntok", [197, 401])
def test_attention_bwd_padding_keys_cannot_poison_a_row_with_a_very_negative_lse(hip, ref, Ntok):
    """the dQ kernel keeps no per-element key mask -- a padding key's K row is zero in the LDS image, its score 0 and its
    "probability" exp2(-lse2).  For a query whose scaled scores are ALL below ~ -88 that overflows to +inf, and inf x 0 (the zero K^T
    column) would be NaN for the whole dQ row.  Here every score is ~ -128 (q = +16, k = -16 on the two lowest-frequency rotary pairs of
    each half, where the rotation is ~ identity): lse ~ -123.  The ragged last tile zeroes the padding keys' dS (wave-uniform branch)."""
    B, H = 1, 2
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), F32, 0.02, seed=41)
    for h in range(H):
        for d in (30, 31, 62, 63):
            qkv[:, h * 64 + d] += 16.0
            qkv[:, C + h * 64 + d] -= 16.0
    qkv = qkv.to(BF)
    cos, sin = _rope(Ntok, 0)
    scale = 64 ** -0.5
    dout = rnd((B * Ntok, C), BF, seed=42)
    o_r, lse_r = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
    ref.attn_fwd(qkv, cos, sin, o_r, lse_r, B, Ntok, H, scale)
    assert float(lse_r.max()) < -100, float(lse_r.max())
    dq_r = torch.zeros(B * Ntok, 3 * C, dtype=BF)
    ref.attn_bwd(qkv, o_r, dout, lse_r, cos, sin, dq_r, None, B, Ntok, H, scale)
    qd, cd, sd, dd = both([qkv, cos, sin, dout])
    o_d = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
    lse_d = torch.empty(B * H, Ntok, device="cuda")
    hip.attn_fwd(qd, cd, sd, o_d, lse_d, B, Ntok, H, scale)
    check(f"attn_neg_lse[{Ntok}].o", o_d, o_r, 6e-3)
    check(f"attn_neg_lse[{Ntok}].lse", lse_d, lse_r, 1e-3)
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
    dq_d = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF, device="cuda")
    hip.attn_bwd(qd, o_r.cuda(), dd, lse_r.cuda(), cd, sd, dq_d, ws, B, Ntok, H, scale)
    assert torch.isfinite(dq_d.float()).all(), "NaN / inf in the attention backward at lse << -88"
    check(f"attn_neg_lse[{Ntok}].dv", dq_d[:, 2 * C:], dq_r[:, 2 * C:], 1.5e-2)
    # dq / dk are differences of nearly equal probabilities here (all scores equal): compare on the scale of dv's magnitude
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C))):
        err = float((dq_d[:, sl].float().cpu() - dq_r[:, sl].float()).norm() / (dq_r[:, 2 * C:].float().norm() + 1e-30))
        _metric(f"attn_neg_lse[{Ntok}].{name}: |diff| / |dv| = {err:.3e}")
        assert err < 1.5e-2, (name, err)


@pytest.mark.parametrize("B,Ntok,H,qscale", [(9, 197, 12, 1.0), (3, 17, 2, 3.0), (2, 65, 2, 2.0), (2, 577, 3, 1.5), (1, 785, 2, 4.0), (2, 4097, 3, 1.0),
                                              (2, 226, 2, 1.0), (1, 257, 3, 2.0), (1, 401, 2, 1.0)])
def test_attention_bwd_restaged_kernels_against_the_round1_kernels(hip, B, Ntok, H, qscale):
    """Round 5 re-staged the attention backward (all rows of a chunk requested up front, next chunk prefetched into registers, RoPE from the
    LDS tables, K^T / Q^T / dO^T read from the row-major images with ds_read_b64_tr_b16) and trimmed its hot loop (no masks: zero K rows /
    +inf lse for the padding; raw v_exp_f32; the softmax scale folded into one FMA: dS = P (dP * scale - D * scale)).  Same products in the
    same order; the folded scale changes fp32 roundings in general, but NOT under this test's precondition: head width 64 makes the scale
    2^-3, a multiplication by a power of two commutes with every rounding, and no probability here is denormal -- so the new kernels must
    still produce the round-1 kernels' bits (CS_ATTN_BWD_V1, read per launch), and two launches must agree in every bit.  The distances are
    logged as well.  (The comparison with the ORACLE at these lengths is test_attention_fwd_bwd, round 6.)  A scale that is not a power of
    two would only satisfy the distance bound, not the bit equality."""
    import os
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=36)
    qkv[:, :2 * C] *= qscale
    qkv = qkv.to(BF).cuda()
    cos, sin = (t.cuda() for t in _rope(Ntok, 0))
    scale = 64 ** -0.5
    dout = rnd((B * Ntok, C), BF, seed=37).cuda()
    o = torch.empty(B * Ntok, C, dtype=BF, device="cuda")
    lse = torch.empty(B * H, Ntok, device="cuda")
    hip.attn_fwd(qkv, cos, sin, o, lse, B, Ntok, H, scale)
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
    got = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF, device="cuda")
    hip.attn_bwd(qkv, o, dout, lse, cos, sin, got, ws, B, Ntok, H, scale)
    assert torch.isfinite(got.float()).all()
    again = torch.full_like(got, float("nan"))
    hip.attn_bwd(qkv, o, dout, lse, cos, sin, again, ws, B, Ntok, H, scale)
    assert torch.equal(got, again), "the backward is not reproducible from launch to launch"
    old = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF, device="cuda")
    os.environ["CS_ATTN_BWD_V1"] = "1"
    try:
        hip.attn_bwd(qkv, o, dout, lse, cos, sin, old, ws, B, Ntok, H, scale)
        torch.cuda.synchronize()
    finally:
        del os.environ["CS_ATTN_BWD_V1"]
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        a, b = got[:, sl].float(), old[:, sl].float()
        r = float((a - b).norm() / b.norm())
        worst = float((a - b).abs().max() / b.pow(2).mean().sqrt())
        _metric(f"attn_bwd v2 vs v1 [{B},{Ntok},{H},x{qscale}] {name}: rel-L2 {r:.2e}, worst |diff| / rms {worst:.2e}, differing {float((a != b).float().mean()):.2%}")
        assert r <= 2e-3 and worst <= 0.1, (name, r, worst)
        assert scale == 2.0 ** -3                        # the precondition of the bit equality (docstring)
        assert torch.equal(got[:, sl], old[:, sl]), f"{name}: {int((a != b).sum())} elements differ from the round-1 kernel"


@pytest.mark.parametrize("B,Ntok,H", [(40, 197, 12), (9, 17, 2), (5, 65, 12), (3, 145, 4), (2, 197, 2), (7, 101, 3)])
def test_attention_forward_short_sequences_against_the_oracle(hip, ref, B, Ntok, H):
    """The short-sequence forward (attn_fwd8_kernel, Ntok <= 224) on grids of 4 ... 14 tokens per side, with and without the ragged-tail
    variant: cs_attn_fwd_stats against RefOps.attn_fwd (o, lse); cs_attn_fwd and cs_attn_fwd_stats agree in every bit; the statistics
    partials are the per-head (sum, sum of squares) of the bf16 output rows."""
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), BF, 1.0, seed=38)
    cos, sin = _rope(Ntok, 0)
    scale = 64 ** -0.5
    o_r, lse_r = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
    ref.attn_fwd(qkv, cos, sin, o_r, lse_r, B, Ntok, H, scale)
    qd, cd, sd = both([qkv, cos, sin])
    o = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
    lse = torch.full((B * H, Ntok), float("nan"), device="cuda")
    part = torch.full((H, B * Ntok, 2), float("nan"), device="cuda")
    hip.attn_fwd_stats(qd, cd, sd, o, lse, part, B, Ntok, H, scale)
    tag = f"attn_fwd8[{B},{Ntok},{H}]"
    check(tag + ".o", o, o_r, 4e-3)                    # the bounds of test_attention_fwd_bwd
    check(tag + ".lse", lse, lse_r, 1e-4)
    o2 = torch.full_like(o, float("nan"))
    lse2 = torch.full_like(lse, float("nan"))
    hip.attn_fwd(qd, cd, sd, o2, lse2, B, Ntok, H, scale)
    assert torch.equal(o2, o) and torch.equal(lse2, lse), "cs_attn_fwd and cs_attn_fwd_stats differ"
    assert torch.isfinite(part).all()
    of = o.float().cpu().view(B * Ntok, H, 64)
    check(tag + ".stats.sum", part[..., 0], of.sum(-1).t(), TOL_F32)
    check(tag + ".stats.sumsq", part[..., 1], of.pow(2).sum(-1).t(), TOL_F32)


@pytest.mark.parametrize("B,Ntok,H", [(2, 4097, 12), (1, 4097, 3), (2, 577, 3), (1, 785, 2), (3, 1025, 2), (1, 401, 2), (5, 2305, 4)])
def test_long_sequence_tail_split_schedule_is_bit_identical_to_the_rectangular_grid(hip, B, Ntok, H):
    """Round 6: the 8-wave long-sequence kernels (forward, dQ, dK/dV) issue the blocks of a launch's last, partly filled round as half blocks
    of four row tiles, and a sequence's last tiles ride on the upper half of its last full block (map_block / set_schedule in attention.hip;
    the recipe's 2 x 12 x 4097: 384 + 24 workgroups -> 256 full + 256 half blocks).  Which workgroup computes a row does not enter its
    arithmetic: outputs, lse and all three gradients equal the rectangular grid's (CS_ATTN_NOSPLIT=1, read per launch) in every bit."""
    import os
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), BF, 1.0, seed=39).cuda()
    cos, sin = (t.cuda() for t in _rope(Ntok, 0))
    dout = rnd((B * Ntok, C), BF, seed=40).cuda()
    scale = 64 ** -0.5
    outs = []
    for nosplit in (False, True):
        o = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
        lse = torch.full((B * H, Ntok), float("nan"), device="cuda")
        part = torch.full((H, B * Ntok, 2), float("nan"), device="cuda")
        dq = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF, device="cuda")
        ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
        if nosplit:
            os.environ["CS_ATTN_NOSPLIT"] = "1"
        try:
            hip.attn_fwd_stats(qkv, cos, sin, o, lse, part, B, Ntok, H, scale)
            hip.attn_bwd(qkv, o, dout, lse, cos, sin, dq, ws, B, Ntok, H, scale)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("CS_ATTN_NOSPLIT", None)
        for t in (o, lse, part, dq):
            assert torch.isfinite(t.float()).all()
        outs.append((o, lse, part, dq))
    for a, b, name in zip(outs[0], outs[1], ("o", "lse", "statistics", "dqkv")):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ between the split and the rectangular schedule"


@pytest.mark.parametrize("B,Ntok,H", [(120, 197, 12), (700, 17, 2), (90, 65, 12)])
def test_attention_units_are_launch_size_invariant(hip, B, Ntok, H):
    """A (crop, head) unit's result must not depend on the size of the launch it is part of (more units than resident workgroups: 12
    rounds of 512): every sampled crop of a large launch equals, bit for bit, the same crop attended in a launch of its own; the statistics
    partials and the lse too.  (Round 4 built a unit-loop form of attn_fwd8_kernel -- two workgroups per CU walking the units, the next
    unit's rows requested behind the last P.V -- that this test pinned; measured a tie, not kept: profiles/r04_t_attention_timeline.md.)"""
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), BF, 1.0, seed=33).cuda()
    cos, sin = (t.cuda() for t in _rope(Ntok, 0))
    scale = 64 ** -0.5
    o = torch.full((B * Ntok, C), float("nan"), dtype=BF, device="cuda")
    lse = torch.full((B * H, Ntok), float("nan"), device="cuda")
    part = torch.full((H, B * Ntok, 2), float("nan"), device="cuda")
    hip.attn_fwd_stats(qkv, cos, sin, o, lse, part, B, Ntok, H, scale)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all() and torch.isfinite(part).all()
    for b in (0, 1, B // 2, B - 2, B - 1):
        rows = slice(b * Ntok, (b + 1) * Ntok)
        o1 = torch.empty(Ntok, C, dtype=BF, device="cuda")
        lse1 = torch.empty(H, Ntok, device="cuda")
        part1 = torch.empty(H, Ntok, 2, device="cuda")
        hip.attn_fwd_stats(qkv[rows].contiguous(), cos, sin, o1, lse1, part1, 1, Ntok, H, scale)
        assert torch.equal(o1, o[rows]), f"crop {b}: output differs from the single-crop launch"
        assert torch.equal(lse1, lse[b * H:(b + 1) * H])
        assert torch.equal(part1, part[:, rows])
    o2 = torch.empty_like(o)                            # repeated launch: same bits
    hip.attn_fwd(qkv, cos, sin, o2, None, B, Ntok, H, scale)
    assert torch.equal(o2, o)


@pytest.mark.parametrize("B,Ntok,H,qscale", [(5, 197, 12, 1.0), (3, 17, 2, 3.0), (2, 577, 16, 2.0), (2, 785, 3, 4.0)])
def test_attention_cls_query(hip, ref, B, Ntok, H, qscale):
    """cs_attn_cls_fwd (teacher's last block: CLS query only) against the reference op and against the CLS rows of the
    full attention kernel on the same q|k|v."""
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C + 8), F32, 1.0, seed=33)       # padded row stride
    qkv[:, :2 * C] *= qscale
    qkv = qkv.to(BF)
    cos, sin = _rope(Ntok, 0)
    scale = 64 ** -0.5
    q = qkv.view(B, Ntok, -1)[:, 0, :C].contiguous()
    kv = qkv[:, C:3 * C]
    tag = f"attn_cls[{B},{Ntok},{H},x{qscale}]"
    o_r = torch.empty(B, C, dtype=BF)
    ref.attn_cls_fwd(q, kv, cos, sin, o_r, B, Ntok, H, scale)
    full_r = torch.empty(B * Ntok, C, dtype=BF)
    ref.attn_fwd(qkv[:, :3 * C], cos, sin, full_r, None, B, Ntok, H, scale)
    check(tag + ".ref_vs_ref_full", o_r, full_r.view(B, Ntok, C)[:, 0], 4e-3)   # the two reference ops agree (bf16 ulps)
    qkv_d, cd, sd = both([qkv, cos, sin])
    o_d = torch.full((B, C), float("nan"), dtype=BF, device="cuda")
    hip.attn_cls_fwd(qkv_d.view(B, Ntok, -1)[:, 0, :C], qkv_d[:, C:3 * C], cd, sd, o_d, B, Ntok, H, scale)
    check(tag + ".o", o_d, o_r, 6e-3)
    full_d = torch.empty(B * Ntok, C, dtype=BF, device="cuda")
    hip.attn_fwd(qkv_d[:, :3 * C], cd, sd, full_d, None, B, Ntok, H, scale)
    check(tag + ".vs_full_kernel", o_d, full_d.view(B, Ntok, C)[:, 0], 4e-3)


# ------------------------------------------------------------------------------------------------ folded sub-LayerNorm pieces
@pytest.mark.parametrize("flags", [0, 0x10, 0x20, 0x30, 0x70, 0x90, 0xB0, 0x10B0])
@pytest.mark.parametrize("Hd,Hl,M", [(2048, 2048, 394), (384, 341, 130), (2752, 2730, 300)])
def test_gemm_swiglu_stats_finalize_and_folded_w3(hip, ref, Hd, Hl, M, flags):
    """SwiGLU GEMM that also emits per-slice LayerNorm partials -> cs_ln_stats_finalize -> w3 GEMM with the LayerNorm folded in,
    against (a) the reference ops of the same three calls and (b) the unfolded chain LN(h) . W3^T on the same inputs."""
    K, C = 128, 192
    A, W, bias = rnd((M, K), BF, seed=40), rnd((2 * Hd, K), BF, 0.1, seed=41), rnd((2 * Hd,), F32, 0.5, seed=42)
    W[Hl:Hd] = 0; W[Hd + Hl:] = 0; bias[Hl:Hd] = 0; bias[Hd + Hl:] = 0           # padded hidden units are exact zeros
    P = 4 * ((Hd + 127) // 128)
    h_r, part_r = torch.empty(M, Hd, dtype=BF), torch.zeros(P, M, 2)
    ref.gemm_nt_ln(A, W, h_r, bias=bias, stats_part=part_r, epi=3, group=Hd)
    h_d = torch.full((M, Hd), float("nan"), dtype=BF, device="cuda")
    part_d = torch.full((P, M, 2), float("nan"), device="cuda")
    hip.gemm_nt_ln(A.cuda(), W.cuda(), h_d, bias=bias.cuda(), stats_part=part_d, epi=3, group=Hd, flags=flags)
    tag = f"lnfold[{Hd},{Hl},{M}] flags={flags}"
    check(tag + ".h", h_d, h_r, TOL_BF)
    mean_r, rstd_r, mean_d, rstd_d = torch.empty(M), torch.empty(M), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ref.ln_stats_finalize(part_r, 32, Hl, mean_r, rstd_r, 1e-6)
    hip.ln_stats_finalize(part_d, 32, Hl, mean_d, rstd_d, 1e-6)
    check(tag + ".mean", mean_d, mean_r, 2e-3)
    check(tag + ".rstd", rstd_d, rstd_r, 2e-3)
    # statistics really are those of the rows of h
    hf = h_d.float().cpu()[:, :Hl]
    check(tag + ".mean_vs_rows", mean_d, hf.mean(-1), 1e-4)
    check(tag + ".rstd_vs_rows", rstd_d, torch.rsqrt(hf.var(-1, unbiased=False) + 1e-6), 1e-4)
    # folded w3
    g, beta = rnd((Hl,), F32, 0.2, seed=43) + 1.0, rnd((Hl,), F32, 0.1, seed=44)
    W3, b3, res = rnd((C, Hd), F32, 0.05, seed=45), rnd((C,), F32, seed=46), rnd((M, C), F32, seed=47)
    W3[:, Hl:] = 0
    Wf = torch.zeros(C, Hd, dtype=BF)
    Wf[:, :Hl] = (W3[:, :Hl] * g).to(BF)
    cs, d = Wf.float().sum(1), W3[:, :Hl] @ beta + b3
    out_r = torch.empty(M, C)
    ref.gemm_nt_ln(h_d.cpu(), Wf, out_r, bias=d, extra=res, ln_mean=mean_d.cpu(), ln_rstd=rstd_d.cpu(), ln_colsum=cs)   # same operands as the kernel
    out_d = res.cuda().clone()
    hip.gemm_nt_ln(h_d, Wf.cuda(), out_d, bias=d.cuda(), extra=out_d, ln_mean=mean_d, ln_rstd=rstd_d, ln_colsum=cs.cuda(), flags=flags)
    check(tag + ".out", out_d, out_r, 2e-4)
    # unfolded chain on the same h: LayerNorm -> bf16 -> GEMM
    fln = torch.zeros(M, Hd, dtype=BF)
    gp, bp = torch.zeros(Hd), torch.zeros(Hd)
    gp[:Hl], bp[:Hl] = g, beta
    ref.layernorm_fwd(h_r[:, :Hl], gp[:Hl], bp[:Hl], fln[:, :Hl], None, None, 1e-6)
    plain = torch.empty(M, C)
    ref.gemm_nt(fln, W3.to(BF), plain, b3, res, epi=2)
    check(tag + ".vs_unfolded", out_d - res.cuda(), plain - res, 1e-2)


@pytest.mark.parametrize("flags", [0, 0x10, 0x20, 0x30, 0x70, 0x90, 0xB0, 0x10B0])
@pytest.mark.parametrize("M,C,Hd", [(394, 768, 2048), (130, 192, 384), (1000, 1024, 2752)])
def test_block_layernorms_folded_into_gemms(hip, ref, M, C, Hd, flags):
    """norm1 -> q|k|v and norm2 -> W1|W2 folded into the GEMM epilogues, fed by the residual GEMM's bf16 copy + row statistics:
    each call against its reference op, and the chain against plain LayerNorm -> GEMM on the same residual stream."""
    K0 = 128
    A0, Wp, res = rnd((M, K0), BF, seed=70), rnd((C, K0), BF, 0.1, seed=71), rnd((M, C), F32, 2.0, seed=72) + 0.3
    bp = rnd((C,), F32, seed=73)
    P = (C + 63) // 64
    # residual GEMM emitting the bf16 copy and the per-slice statistics
    x_r, xb_r, part_r = torch.empty(M, C), torch.zeros(M, C, dtype=BF), torch.zeros(P, M, 2)
    ref.gemm_nt_ln(A0, Wp, x_r, bias=bp, extra=res, stats_part=part_r, xb_out=xb_r, epi=2)
    x_d = res.cuda().clone()
    xb_d = torch.zeros(M, C, dtype=BF, device="cuda")
    part_d = torch.full((P, M, 2), float("nan"), device="cuda")
    hip.gemm_nt_ln(A0.cuda(), Wp.cuda(), x_d, bias=bp.cuda(), extra=x_d, stats_part=part_d, xb_out=xb_d, epi=2, flags=flags)
    tag = f"blockfold[{M},{C},{Hd}] flags={flags}"
    check(tag + ".x", x_d, x_r, TOL_F32)
    check(tag + ".xb", xb_d, xb_r, TOL_BF)
    mean_d, rstd_d = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    hip.ln_stats_finalize(part_d, 64, C, mean_d, rstd_d, 1e-6)
    xf = x_d.cpu()
    check(tag + ".mean", mean_d, xf.mean(-1), 1e-5)
    check(tag + ".rstd", rstd_d, torch.rsqrt(xf.var(-1, unbiased=False) + 1e-6), 1e-5)
    # q|k|v-style GEMM with norm folded in
    g, beta = rnd((C,), F32, 0.2, seed=74) + 1.0, rnd((C,), F32, 0.1, seed=75)
    N = 3 * 64
    W, bq = rnd((N, C), F32, 0.05, seed=76), rnd((N,), F32, seed=77)
    Wf = (W * g).to(BF)
    cs, d = Wf.float().sum(1), W @ beta + bq
    q_r = torch.empty(M, N, dtype=BF)
    ref.gemm_nt_ln(xb_d.cpu(), Wf, q_r, bias=d, ln_mean=mean_d.cpu(), ln_rstd=rstd_d.cpu(), ln_colsum=cs, epi=0)
    q_d = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt_ln(xb_d, Wf.cuda(), q_d, bias=d.cuda(), ln_mean=mean_d, ln_rstd=rstd_d, ln_colsum=cs.cuda(), epi=0, flags=flags)
    check(tag + ".qkv", q_d, q_r, TOL_BF)
    ln = torch.empty(M, C, dtype=BF)
    ref.layernorm_fwd(xf, g, beta, ln, None, None, 1e-6)
    plain = torch.empty(M, N, dtype=BF)
    ref.gemm_nt(ln, W.to(BF), plain, bq, epi=0)
    check(tag + ".qkv_vs_unfolded", q_d, plain, 1.2e-2)
    # W1|W2-style GEMM with norm folded in, SiLU*mul + statistics of the result
    W12, b12 = rnd((2 * Hd, C), F32, 0.05, seed=78), rnd((2 * Hd,), F32, 0.3, seed=79)
    W12f = (W12 * g).to(BF)
    c12, d12 = W12f.float().sum(1), W12 @ beta + b12
    Ph = 4 * ((Hd + 127) // 128)
    h_r, ph_r = torch.empty(M, Hd, dtype=BF), torch.zeros(Ph, M, 2)
    ref.gemm_nt_ln(xb_d.cpu(), W12f, h_r, bias=d12, ln_mean=mean_d.cpu(), ln_rstd=rstd_d.cpu(), ln_colsum=c12, stats_part=ph_r, epi=3, group=Hd)
    h_d = torch.full((M, Hd), float("nan"), dtype=BF, device="cuda")
    ph_d = torch.full((Ph, M, 2), float("nan"), device="cuda")
    hip.gemm_nt_ln(xb_d, W12f.cuda(), h_d, bias=d12.cuda(), ln_mean=mean_d, ln_rstd=rstd_d, ln_colsum=c12.cuda(), stats_part=ph_d, epi=3,
                   group=Hd, flags=flags)
    check(tag + ".hid", h_d, h_r, 6e-3)
    mh, rh = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    hip.ln_stats_finalize(ph_d, 32, Hd, mh, rh, 1e-6)
    hf = h_d.float().cpu()
    check(tag + ".hid_mean", mh, hf.mean(-1), 1e-4)
    check(tag + ".hid_rstd", rh, torch.rsqrt(hf.var(-1, unbiased=False) + 1e-6), 1e-4)


@pytest.mark.parametrize("B,Q,Ntok,H", [(3, 5, 197, 12), (2, 1, 17, 2), (2, 9, 577, 16), (4, 3, 65, 4)])
def test_attention_extra_query_tokens_with_key_masks(hip, ref, B, Q, Ntok, H):
    """cs_attn_query_fwd (mask-attention pooling of the OpenAI-CLIP family, open_clip/transformer.py:736-834): Q query rows per image against
    the image's k|v columns of a q|k|v tensor (strided view), per-query key masks incl. a CLS-only row; against the reference op, against
    the CLS-query kernel (all keys allowed, identity rotary tables) and bit-reproducible."""
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=70)
    qkv[:, C:2 * C] *= 2.0
    qkv = qkv.to(BF)
    q = (rnd((B * Q, C), F32, 1.0, seed=71) * 2.0).to(BF)
    gen = torch.Generator().manual_seed(72)
    allow = (torch.rand(B * Q, Ntok, generator=gen) > 0.5).to(torch.uint8)
    allow[:, 0] = 1                                          # the CLS key is always visible in the reference's mask
    allow[0, 1:] = 0                                         # an empty mask
    allow[-1] = 1                                            # a see-everything (padding) token
    o_r = torch.empty(B * Q, C, dtype=BF)
    ref.attn_query_fwd(q, qkv[:, C:], allow, o_r, B, Q, Ntok, H, 0.125)
    qd, kvd, ad = q.cuda(), qkv.cuda()[:, C:], allow.cuda()
    o_d = torch.full((B * Q, C), float("nan"), dtype=BF, device="cuda")
    hip.attn_query_fwd(qd, kvd, ad, o_d, B, Q, Ntok, H, 0.125)
    tag = f"attn_query[{B},{Q},{Ntok},{H}]"
    check(tag + ".o", o_d, o_r, 6e-3)
    o_d2 = torch.empty_like(o_d)
    hip.attn_query_fwd(qd, kvd, ad, o_d2, B, Q, Ntok, H, 0.125)
    assert torch.equal(o_d2, o_d)
    # CLS-only row: softmax over one key = that key's value row, exactly (bf16 of a bf16)
    v0 = qkv[:Ntok][0, 2 * C:].cuda()
    assert torch.equal(o_d[0], v0)
    # everything allowed == the CLS-query kernel with identity rotary tables (same arithmetic, one query per image)
    ones = torch.ones(B, Ntok, dtype=torch.uint8, device="cuda")
    g = int(round((Ntok - 1) ** 0.5))
    cos, sin = torch.ones(g * g, 64, device="cuda"), torch.zeros(g * g, 64, device="cuda")
    q1 = q[::Q].contiguous().cuda()
    a, b = torch.empty(B, C, dtype=BF, device="cuda"), torch.empty(B, C, dtype=BF, device="cuda")
    hip.attn_query_fwd(q1, kvd, ones, a, B, 1, Ntok, H, 0.125)
    hip.attn_cls_fwd(q1, kvd, cos, sin, b, B, Ntok, H, 0.125)
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,Ntok,H", [(3, 197, 12), (2, 577, 16), (4, 17, 2)])
def test_attention_fwd_stats_and_layernorm_stats_only(hip, ref, B, Ntok, H):
    C = H * 64
    qkv = rnd((B * Ntok, 3 * C), BF, 1.0, seed=50)
    cos, sin = _rope(Ntok, 0)
    scale = 64 ** -0.5
    qd, cd, sd = both([qkv, cos, sin])
    o_plain = torch.empty(B * Ntok, C, dtype=BF, device="cuda")
    hip.attn_fwd(qd, cd, sd, o_plain, None, B, Ntok, H, scale)
    o_d = torch.empty_like(o_plain)
    part = torch.full((H, B * Ntok, 2), float("nan"), device="cuda")
    hip.attn_fwd_stats(qd, cd, sd, o_d, None, part, B, Ntok, H, scale)
    assert torch.equal(o_d, o_plain)
    mean_d, rstd_d = torch.empty(B * Ntok, device="cuda"), torch.empty(B * Ntok, device="cuda")
    hip.ln_stats_finalize(part, 64, C, mean_d, rstd_d, 1e-6)
    of = o_d.float().cpu()
    tag = f"attn_stats[{B},{Ntok},{H}]"
    check(tag + ".mean", mean_d, of.mean(-1), 2e-4)
    check(tag + ".rstd", rstd_d, torch.rsqrt(of.var(-1, unbiased=False) + 1e-6), 2e-4)
    # statistics-only LayerNorm launch (y = NULL) gives the same numbers
    m2, r2 = torch.empty_like(mean_d), torch.empty_like(rstd_d)
    hip.layernorm_fwd(o_d, None, None, None, m2, r2, 1e-6)
    check(tag + ".ln_stats_only.mean", m2, mean_d, 2e-4)
    check(tag + ".ln_stats_only.rstd", r2, rstd_d, 2e-4)


# ------------------------------------------------------------------------------------------------ GPU input pipeline
@pytest.mark.parametrize("H,W,size,pad_center", [(427, 640, 224, True), (500, 333, 224, True), (683, 1024, 336, True), (96, 130, 224, True),
                                                   (480, 640, 224, False)])
def test_crop_resize_is_pillow_exact(hip, H, W, size, pad_center):
    """cs_crop_resize_u8 (crop -> bicubic resize of the longest side -> zero pad -> /255 -> normalise) against Pillow itself:
    grid cells of the reference's (M, N) templates (data.py:200-224), free-form boxes, and the whole image (the det transform)."""
    import numpy as np
    from oracle.pil_crops_ref import pil_crops
    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[: H // 2, : W // 3] = (rng.integers(0, 256, (H // 2, W // 3, 1)) // 3 + 90).astype(np.uint8)      # some smooth structure too
    boxes = []
    for M, N in ((1, 1), (2, 3), (6, 6), (5, 3)):
        xs, ys = np.linspace(0, 1, N + 1) * W, np.linspace(0, 1, M + 1) * H
        boxes += [(xs[j], ys[i], xs[j + 1], ys[i + 1]) for i in range(M) for j in range(N)]
    for _ in range(12):
        x0, y0 = rng.uniform(0, W * 0.6), rng.uniform(0, H * 0.6)
        boxes.append((x0, y0, min(x0 + rng.uniform(8, W * 0.4), W), min(y0 + rng.uniform(8, H * 0.4), H)))
    boxes.append((10.5, 20.5, 41.5, 37.5))                                                                 # .5 edges: round-half-even
    if not pad_center:
        boxes = [(0.0, 0.0, float(W), float(H))]                                                            # det image transform
    boxes = np.asarray(boxes, np.float32)
    want = torch.from_numpy(pil_crops(img, boxes, size, pad_center))
    got = hip.crop_resize(torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda(), size, pad_center)
    bad = int((got.cpu() != want).sum())
    with open(_LOG, "a") as f:
        f.write(f"crop_resize[{H}x{W}->{size}, {len(boxes)} boxes, centre={pad_center}]: {bad} of {want.numel()} values differ from Pillow\n")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ elementwise
def test_swiglu_cast_transpose_colsum_im2row(hip, ref):
    M, Hd = 333, 2048
    x12, dh = rnd((M, 2 * Hd), BF, 2.0, seed=40), rnd((M, Hd), BF, seed=41)
    hr, dxr = torch.empty(M, Hd, dtype=BF), torch.empty(M, 2 * Hd, dtype=BF)
    ref.swiglu_fwd(x12, hr)
    ref.swiglu_bwd(dh, x12, dxr)
    hd, dxd = torch.empty(M, Hd, dtype=BF, device="cuda"), torch.empty(M, 2 * Hd, dtype=BF, device="cuda")
    hip.swiglu_fwd(x12.cuda(), hd)
    hip.swiglu_bwd(dh.cuda(), x12.cuda(), dxd)
    check("swiglu.fwd", hd, hr, TOL_BF)
    check("swiglu.bwd", dxd, dxr, TOL_BF)

    x = rnd((4096 * 8,), F32, seed=42)
    yd = torch.empty(x.numel(), dtype=BF, device="cuda")
    hip.cast_f32_bf16(x.cuda(), yd)
    assert torch.equal(yd.cpu(), x.to(BF))

    for R, Cc in ((197, 768), (64, 64), (3152, 2304), (130, 70)):
        big = rnd((R, Cc + 8), BF, seed=43)
        inp = big[:, :Cc]
        ld = (R + 63) // 64 * 64
        outr = torch.empty(Cc, ld, dtype=BF)
        ref.transpose_bf16(inp, outr)
        outd = torch.full((Cc, ld), float("nan"), dtype=BF, device="cuda")
        hip.transpose_bf16(big.cuda()[:, :Cc], outd)
        assert torch.equal(outd.cpu(), outr), f"transpose[{R},{Cc}]"
    # the same shapes (strided input views, padded outputs) as ONE batched launch, twice (the second call reuses the cached descriptors)
    ins = [rnd((R, Cc + 8), BF, seed=50 + i).cuda()[:, :Cc] for i, (R, Cc) in enumerate(((197, 768), (64, 64), (3152, 2304), (130, 70), (2304, 768)))]
    outs = [torch.full((a.shape[1], (a.shape[0] + 63) // 64 * 64), float("nan"), dtype=BF, device="cuda") for a in ins]
    for rep in range(2):
        for o in outs:
            o.fill_(float("nan"))
        hip.transpose_bf16_batched(list(zip(ins, outs)))
        for a, o in zip(ins, outs):
            want = torch.empty(o.shape, dtype=BF)
            ref.transpose_bf16(a.cpu(), want)
            assert torch.equal(o.cpu(), want), f"batched transpose {tuple(a.shape)} rep {rep}"

    xs = rnd((1234, 770), BF, seed=44)
    base = rnd((770,), F32, seed=45)
    cr = base.clone()
    ref.colsum_bf16(xs, cr)
    cd = base.cuda()
    hip.colsum_bf16(xs.cuda(), cd)
    check("colsum", cd, cr, 1e-4)
    big = rnd((12608, 768), BF, seed=47).cuda()                       # the step's shape: row-block partials + a fixed-order combine, no atomics
    outs = []
    for _ in range(3):
        o = torch.zeros(768, device="cuda")
        hip.colsum_bf16(big, o, torch.empty(hip.colsum_workspace(12608, 768), dtype=torch.uint8, device="cuda"))
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    check("colsum.step_shape", outs[0], big.float().sum(0), 1e-4)

    for dt in (F32, BF):
        img = rnd((3, 3, 64, 64), F32, seed=46).to(dt)
        outr = torch.empty(3 * 16, 3 * 256, dtype=BF)
        ref.im2row(img, outr, 16)
        outd = torch.empty(3 * 16, 3 * 256, dtype=BF, device="cuda")
        hip.im2row(img.cuda(), outd, 16)
        assert torch.equal(outd.cpu(), outr), "im2row"


# ------------------------------------------------------------------------------------------------ RoIAlign / loss / AdamW
def _boxes(K, B, seed, wild=False):
    g = torch.Generator().manual_seed(seed)
    xy0 = torch.rand(K, 2, generator=g) * 0.6
    wh = torch.rand(K, 2, generator=g) * 0.3 + 0.1
    xy1 = (xy0 + wh).clamp(max=1.0)
    if wild:                                           # degenerate / border-crossing / tiny boxes
        xy0[0], xy1[0] = torch.tensor([0.3, 0.3]), torch.tensor([0.3, 0.3])
        xy0[1], xy1[1] = torch.tensor([-0.2, 0.1]), torch.tensor([0.2, 0.5])
        xy0[2], xy1[2] = torch.tensor([0.9, 0.9]), torch.tensor([1.2, 1.3])
        xy0[3], xy1[3] = torch.tensor([0.5, 0.5]), torch.tensor([0.51, 0.52])
        xy0[4], xy1[4] = torch.tensor([0.0, 0.0]), torch.tensor([1.0, 1.0])
        xy0[5], xy1[5] = torch.tensor([0.6, 0.2]), torch.tensor([0.4, 0.1])
    b = torch.randint(0, B, (K, 1), generator=g).float()
    return torch.cat([b, xy0, xy1], dim=1)


@pytest.mark.parametrize("grid,E", [(14, 512), (4, 64), (24, 768), (14, 1280)])      # 1280: wider than one workgroup's 1024 channels
def test_roialign_fwd_bwd(hip, ref, grid, E):
    B, K = 3, 40
    Ntok = grid * grid + 1
    feat = rnd((B, Ntok, E), F32, seed=50)
    rois = _boxes(K, B, 51, wild=True)
    dp = rnd((K, E), F32, seed=52)
    pr, dfr = torch.empty(K, E), torch.zeros(B, Ntok, E)
    ref.roialign_fwd(feat, rois, pr, grid, grid, 1)
    ref.roialign_bwd(dp, rois, dfr, grid, grid, 1)
    pd, dfd = torch.empty(K, E, device="cuda"), torch.zeros(B, Ntok, E, device="cuda")
    hip.roialign_fwd(feat.cuda(), rois.cuda(), pd, grid, grid, 1)
    hip.roialign_bwd(dp.cuda(), rois.cuda(), dfd, grid, grid, 1)
    check(f"roialign[{grid}].fwd", pd, pr, TOL_F32)
    check(f"roialign[{grid}].bwd", dfd, dfr, TOL_F32)
    assert float(dfd[:, 0].abs().max()) == 0.0          # CLS rows never receive gradient
    # the backward is a gather in a fixed order: bit-reproducible, and "+=" onto what the caller left in dfeat
    again = torch.zeros(B, Ntok, E, device="cuda")
    hip.roialign_bwd(dp.cuda(), rois.cuda(), again, grid, grid, 1)
    assert torch.equal(again, dfd)
    hip.roialign_bwd(dp.cuda(), rois.cuda(), again, grid, grid, 1)
    check(f"roialign[{grid}].bwd accumulates", again, 2 * dfr, TOL_F32)


def test_roialign_bwd_is_deterministic_at_step_size(hip):
    """BASELINE configs[1]'s pooling problem (64 images x 32 heavily overlapping boxes on the 14 x 14 map, E = 512): two backward passes
    give identical bits (torchvision's / round 2's atomic scatter differed run to run by ~3e-4 relative)."""
    B, per, grid, E = 64, 32, 14, 512
    g = torch.Generator().manual_seed(5)
    xy0 = torch.rand(B * per, 2, generator=g) * 0.6
    wh = torch.rand(B * per, 2, generator=g) * 0.3 + 0.1
    rois = torch.cat([torch.arange(B).repeat_interleave(per)[:, None].float(), xy0, (xy0 + wh).clamp(max=1.0)], dim=1).cuda()
    dp = torch.randn(B * per, E, generator=g).cuda()
    outs = []
    for _ in range(3):
        d = torch.zeros(B, grid * grid + 1, E, device="cuda")
        hip.roialign_bwd(dp, rois, d, grid, grid, 1)
        outs.append(d)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert float(outs[0].abs().sum()) > 0.0


def test_cosine_loss(hip, ref):
    K, E = 2048, 512
    s, t = rnd((K, E), F32, 0.3, seed=60), rnd((K, E), F32, 2.0, seed=61)
    sr, lr, dr = torch.empty(K, 3), torch.empty(1), torch.empty(K, E)
    ref.cosine_loss_fwd(s, t, sr, lr, 1.0)
    ref.cosine_loss_bwd(s, t, sr, dr, 1.0, 1.0)
    sd, ld, dd = torch.empty(K, 3, device="cuda"), torch.empty(1, device="cuda"), torch.empty(K, E, device="cuda")
    hip.cosine_loss_fwd(s.cuda(), t.cuda(), sd, ld, 1.0)
    hip.cosine_loss_bwd(s.cuda(), t.cuda(), sd, dd, 1.0, 1.0)
    check("cosine.loss", ld, lr, 1e-6)
    check("cosine.stats", sd, sr, TOL_F32)
    check("cosine.bwd", dd, dr, TOL_F32)
    # autograd cross-check of the reference formula itself
    s2 = s.clone().requires_grad_(True)
    loss = 1.0 - (torch.nn.functional.normalize(s2, dim=-1) * torch.nn.functional.normalize(t, dim=-1)).sum(-1).mean()
    loss.backward()
    assert rel(dr, s2.grad) < 1e-5 and abs(float(loss) - float(lr)) < 1e-6


def test_adamw_matches_torch(hip, ref):
    n = 256 * 40
    p0, g = rnd((n,), F32, 0.02, seed=70), rnd((n,), F32, 1e-3, seed=71)
    flags = torch.tensor([3, 1, 0, 2] * 10, dtype=torch.uint8).repeat_interleave(4)   # one byte per 64 elements
    flags[4:8] = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)     # mixed flags inside one 256-element wave chunk
    pd, md, vd = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    sh = torch.zeros(n, dtype=BF, device="cuda")
    tp = [p0[i * 64:(i + 1) * 64].clone().requires_grad_(True) for i in range(160)]
    dec = [t for i, t in enumerate(tp) if flags[i] == 3]
    nod = [t for i, t in enumerate(tp) if flags[i] == 1]
    opt = torch.optim.AdamW([{"params": nod, "weight_decay": 0.0}, {"params": dec, "weight_decay": 0.1}], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for step in range(1, 4):
        gs = g * step
        hip.adamw_step(pd, gs.cuda(), md, vd, sh, flags.cuda(), 1e-3, 0.9, 0.999, 1e-8, 0.1, step)
        for i, t in enumerate(tp):
            t.grad = gs[i * 64:(i + 1) * 64].clone() if flags[i] & 1 else None
        opt.step()
    want = torch.cat([t.detach() for t in tp])
    check("adamw.p", pd, want, 1e-6)
    act = (flags & 1).bool().repeat_interleave(64)
    assert torch.equal(sh.cpu()[act], pd.cpu().to(BF)[act]) and float(sh.cpu()[~act].abs().max()) == 0.0


def test_fed_bce(hip, ref):
    K, ns, ld = 77, 100, 128
    logits = rnd((K, ld), F32, 3.0, seed=80)
    tgt = torch.randint(-1, ns, (K,), generator=torch.Generator().manual_seed(81)).to(torch.int32)
    up = torch.tensor([0.7])
    rl_r, l_r, dz_r = torch.empty(K), torch.empty(1), torch.empty(K, ld, dtype=BF)
    ref.fed_bce_fwd(logits, tgt, rl_r, l_r, ns, 14.3, 1.0)
    ref.fed_bce_bwd(logits, tgt, dz_r, ns, 14.3, 1.0, up)
    rl_d, l_d = torch.empty(K, device="cuda"), torch.empty(1, device="cuda")
    dz_d = torch.full((K, ld), float("nan"), dtype=BF, device="cuda")
    hip.fed_bce_fwd(logits.cuda(), tgt.cuda(), rl_d, l_d, ns, 14.3, 1.0)
    hip.fed_bce_bwd(logits.cuda(), tgt.cuda(), dz_d, ns, 14.3, 1.0, up.cuda())
    check("fed_bce.rowloss", rl_d, rl_r, 1e-5)
    check("fed_bce.loss", l_d, l_r, 1e-5)
    check("fed_bce.dz", dz_d, dz_r, TOL_BF)
    assert float(dz_d[:, ns:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ OpenAI-CLIP ViT family (N4)
@pytest.mark.parametrize("flags", [0, 1, 0x10, 0x20, 0x30, 0x70, 0x90, 0xB0, 0x10B0])
@pytest.mark.parametrize("quick", [False, True])
@pytest.mark.parametrize("M,N,K", [(394, 3072, 768), (130, 512, 128), (1000, 4096, 1024)])
def test_gemm_gelu_epilogues(hip, ref, M, N, K, quick, flags):
    """c_fc + bias + GELU / QuickGELU fused into the GEMM epilogue (epi 7 / 8) on every schedule."""
    epi = 8 if quick else 7
    A, B, bias = rnd((M, K), BF, 1.5, seed=61), rnd((N, K), BF, 0.05, seed=62), rnd((N,), F32, seed=63)
    Cr = torch.empty(M, N, dtype=BF)
    ref.gemm_nt(A, B, Cr, bias, epi=epi)
    assert float((Cr.float() < 0).float().mean()) > 0.2          # both signs: the non-linear part of the activation is exercised
    Cd = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt(A.cuda(), B.cuda(), Cd, bias.cuda(), epi=epi, flags=flags)
    check(f"gemm_gelu[{M},{N},{K}] quick={quick} flags={flags}", Cd, Cr, TOL_BF)


@pytest.mark.parametrize("quick", [False, True])
def test_gemm_gelu_with_folded_layernorm(hip, ref, quick):
    """epi 7 / 8 through cs_gemm_nt_ln: the LayerNorm in front of c_fc applied in the epilogue, then the activation."""
    M, N, K, epi = 394, 3072, 768, 8 if quick else 7
    X = rnd((M, K), F32, 2.0, seed=64) + 0.5
    gamma, beta = 1 + 0.1 * rnd((K,), F32, seed=65), 0.1 * rnd((K,), F32, seed=66)
    W, b = rnd((N, K), F32, 0.05, seed=67), rnd((N,), F32, 0.1, seed=68)
    mean, var = X.mean(-1), X.var(-1, unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    Xb, Wf = X.to(BF), (W * gamma[None, :]).to(BF)
    colsum, bias = Wf.float().sum(1).contiguous(), (W @ beta + b).contiguous()
    Cr = torch.empty(M, N, dtype=BF)
    ref.gemm_nt_ln(Xb, Wf, Cr, bias=bias, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, epi=epi)
    plain = torch.empty(M, N, dtype=BF)                           # the unfolded computation it replaces
    ln = torch.nn.functional.layer_norm(X, (K,), gamma, beta, 1e-5).to(BF)
    ref.gemm_nt(ln, W.to(BF), plain, b, epi=epi)
    assert rel(Cr, plain) < 2e-2
    Cd = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt_ln(Xb.cuda(), Wf.cuda(), Cd, bias=bias.cuda(), ln_mean=mean.cuda(), ln_rstd=rstd.cuda(), ln_colsum=colsum.cuda(), epi=epi)
    check(f"gemm_gelu_lnfold quick={quick}", Cd, Cr, TOL_BF)


@pytest.mark.parametrize("quick", [False, True])
def test_gelu_fwd_bwd(hip, ref, quick):
    M, N = 394, 3072
    xbig = rnd((M, N + 64), BF, 2.0, seed=70)
    x, dy = xbig[:, :N], rnd((M, N), BF, seed=71)                  # strided input rows
    yr, dxr = torch.empty(M, N, dtype=BF), torch.empty(M, N, dtype=BF)
    ref.gelu_fwd(x, yr, quick)
    ref.gelu_bwd(dy, x, dxr, quick)
    xd = xbig.cuda()[:, :N]
    yd, dxd = torch.full((M, N), float("nan"), dtype=BF, device="cuda"), torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    hip.gelu_fwd(xd, yd, quick)
    hip.gelu_bwd(dy.cuda(), xd, dxd, quick)
    check(f"gelu_fwd quick={quick}", yd, yr, TOL_BF)
    check(f"gelu_bwd quick={quick}", dxd, dxr, TOL_BF)


@pytest.mark.parametrize("C", [128, 768, 1024, 1280])
def test_layernorm_fwd_f32_out(hip, ref, C):
    M = 395
    x = rnd((M, C), F32, 3.0, seed=72) + 1.0
    gamma, beta = 1 + 0.1 * rnd((C,), F32, seed=73), 0.1 * rnd((C,), F32, seed=74)
    yr, mr, rr = torch.empty(M, C), torch.empty(M), torch.empty(M)
    ref.layernorm_fwd_f32(x, gamma, beta, yr, mr, rr, 1e-5)
    yd, md, rd = torch.full((M, C), float("nan"), device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    hip.layernorm_fwd_f32(x.cuda(), gamma.cuda(), beta.cuda(), yd, md, rd, 1e-5)
    check(f"layernorm_f32[{C}] y", yd, yr, TOL_F32)
    check(f"layernorm_f32[{C}] mean", md, mr, TOL_F32)
    check(f"layernorm_f32[{C}] rstd", rd, rr, TOL_F32)
    y2 = torch.full((M, C), float("nan"), device="cuda")
    hip.layernorm_fwd_f32(x.cuda(), gamma.cuda(), beta.cuda(), y2, None, None, 1e-5)
    assert torch.equal(y2, yd)


# ------------------------------------------------------------------------------------------------ persistent-kernel raster / cache-policy modes
@pytest.mark.parametrize("mode", [0x10090, 0x10190, 0x10290, 0x10490, 0x10890, 0x20090, 0x20290, 0x30090, 0xB0, 0x10B0, 0xB0 | (24 << 20), 0x10090 | (16 << 20),
                                  0x10290 | (232 << 20), 0xB0 | (232 << 20)])      # bits 20-27: 24 / 16 / 232 CUs left free (streaming kernel, B-stationary raster)
@pytest.mark.parametrize("M,N,K,epi", [(65536 + 300, 2304, 128, 0), (70000, 4096, 64, 3), (66000, 768, 192, 0), (300, 512, 64, 0)])
def test_gemm_persistent_raster_modes_cover_every_tile(hip, ref, M, N, K, epi, mode):
    """flags bits 16-17: B-stationary raster (N parts in bits 8-11; 0 = automatic), with non-temporal A loads, and non-temporal B loads on the
    grouped raster -- every output tile written exactly as by the default raster (NaN-prefilled output, bitwise comparison)."""
    A, B, bias = rnd((M, K), BF, seed=81), rnd((N, K), BF, 0.05, seed=82), rnd((N,), F32, seed=83)
    Ad, Bd, bd = both([A, B, bias])
    cols, group = (N // 2, N // 2) if epi == 3 else (N, 0)
    base = torch.full((M, cols), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt(Ad, Bd, base, bd, epi=epi, group=group, flags=0x90)
    assert torch.isfinite(base.float()).all()
    got = torch.full((M, cols), float("nan"), dtype=BF, device="cuda")
    hip.gemm_nt(Ad, Bd, got, bd, epi=epi, group=group, flags=mode)
    assert torch.equal(got, base), f"mode {mode:#x}: {int((got != base).sum())} elements differ"
    if M < 1000:
        Cr = torch.empty(M, cols, dtype=BF)
        ref.gemm_nt(A, B, Cr, bias, epi=epi, group=group)
        check(f"gemm_raster_mode[{M},{N},{K}] epi={epi} mode={mode:#x}", got, Cr, TOL_BF)


def test_factory_transforms_run_the_crop_kernel_and_equal_pillow(hip):
    """The `[det transform, crop transform]` pair of create_model_and_transforms on the GPU (cs_crop_resize_u8 behind the reference's
    transform API): PIL image in, normalised tensor out, bit-identical to the Pillow statement of ResizeLongest / ResizeMaxSize."""
    import numpy as np
    from PIL import Image
    from clipself_amd.open_clip.transform import det_image_transform, image_transform
    from oracle.pil_crops_ref import pil_crops
    rng = np.random.default_rng(9)
    for (H, W), size in (((427, 640), 224), ((500, 333), 336), ((96, 130), 1024)):
        arr = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        img = Image.fromarray(arr, mode="RGB")
        whole = np.array([[0.0, 0.0, float(W), float(H)]], np.float32)
        det = det_image_transform(size, is_train=False, ops=hip)(img)
        crop = image_transform(size, is_train=False, resize_longest_max=True, ops=hip)(img)
        assert det.is_cuda and tuple(det.shape) == (3, size, size)
        assert np.array_equal(det.cpu().numpy(), pil_crops(arr, whole, size, pad_center=False)[0]), (H, W, size, "det")
        assert np.array_equal(crop.cpu().numpy(), pil_crops(arr, whole, size, pad_center=True)[0]), (H, W, size, "crop")


@pytest.mark.parametrize("M,N,K", [(394, 768, 768), (130, 3072, 1024), (1000, 1024, 2752), (70000, 2304, 768), (64, 512, 128)])
@pytest.mark.parametrize("epi", [0, 2])
def test_fp8_quantisation_and_gemm(hip, ref, M, N, K, epi):
    """BASELINE configs[4] "fp8 MFMA weights": cs_quant_rows_fp8 (row-wise e4m3, amax/448 scales, K padded to 128) is bit-identical to the
    torch.float8_e4m3fn statement, and cs_gemm_nt_f8 (block-scaled fp8 MFMA at unit block scales, fp32 accumulate, row x column scales +
    bias [+ residual] in the epilogue) equals the exact product of the quantised operands."""
    x, w = rnd((M, K), BF, seed=90), rnd((N, K), BF, 0.05, seed=91)
    bias, res = rnd((N,), F32, seed=92), rnd((M, N), F32, seed=93)
    Kp = (K + 127) // 128 * 128
    q = {}
    for tag, ops, dev in (("ref", ref, "cpu"), ("hip", hip, "cuda")):
        xq, wq = torch.full((M, Kp), 0x55, dtype=torch.uint8, device=dev), torch.full((N, Kp), 0x55, dtype=torch.uint8, device=dev)
        sx, sw = torch.empty(M, device=dev), torch.empty(N, device=dev)
        ops.quant_rows_fp8(x.to(dev), xq, sx)
        ops.quant_rows_fp8(w.to(dev), wq, sw)
        q[tag] = (xq, wq, sx, sw)
    # quantiser: same scales (1 ulp: the kernel multiplies by 448/amax) and the same e4m3 codes except for round-to-nearest ties that a
    # 1-ulp different scaled value flips -- at most one code step, on a vanishing fraction of the elements
    for tag, (a, b) in (("x", (q["ref"][0], q["hip"][0].cpu())), ("w", (q["ref"][1], q["hip"][1].cpu()))):
        da = a.view(torch.float8_e4m3fn).float()
        db = b.view(torch.float8_e4m3fn).float()
        diff = (a != b)
        frac = float(diff.float().mean())
        step = float(((da - db).abs() / da.abs().clamp_min(2.0 ** -6))[diff].max()) if diff.any() else 0.0
        with open(_LOG, "a") as f:
            f.write(f"quant_fp8[{M},{N},{K}].{tag}: {int(diff.sum())} of {a.numel()} codes differ ({frac:.2e}), worst relative step {step:.3f}\n")
        assert frac < 2e-3 and step <= 0.126, (tag, frac, step)
        assert torch.equal(a[:, K:], b[:, K:])
    assert torch.allclose(q["ref"][2], q["hip"][2].cpu(), rtol=2e-7, atol=0) and torch.allclose(q["ref"][3], q["hip"][3].cpu(), rtol=2e-7, atol=0)
    # GEMM: exact product of the kernel's own quantised operands
    xq, wq, sx, sw = q["hip"]
    cpu = [t.cpu() for t in q["hip"]]
    if epi == 0:
        Cd, Cr = torch.full((M, N), float("nan"), dtype=BF, device="cuda"), torch.empty(M, N, dtype=BF)
        hip.gemm_nt_f8(xq, wq, Cd, sx, sw, bias=bias.cuda(), epi=0)
        ref.gemm_nt_f8(cpu[0], cpu[1], Cr, cpu[2], cpu[3], bias=bias, epi=0)
        check(f"gemm_f8_bf16[{M},{N},{K}]", Cd, Cr, TOL_BF)
    else:
        Cd, Cr = res.cuda().clone(), torch.empty(M, N)
        hip.gemm_nt_f8(xq, wq, Cd, sx, sw, bias=bias.cuda(), extra=Cd, epi=2)
        ref.gemm_nt_f8(cpu[0], cpu[1], Cr, cpu[2], cpu[3], bias=bias, extra=res, epi=2)
        check(f"gemm_f8_resid[{M},{N},{K}]", Cd, Cr, 2e-5)
    # and the quantised product is a faithful GEMM: within fp8 rounding of the bf16 product
    exact = x.float() @ w.float().T + bias + (res if epi == 2 else 0)
    got = Cd.float().cpu()
    assert float((got - exact).norm() / exact.norm()) < 6e-2


@pytest.mark.parametrize("C,mode", [(768, 2), (1024, 1), (64, 2), (2048, 2)])
def test_layernorm_backward_with_fused_fp8_quantiser(hip, ref, C, mode):
    """cs_layernorm_bwd_q8: dx, the bf16 copy, its column sums and the parameter gradients unchanged; the copy's e4m3 codes + row scales are
    bit-identical to cs_quant_rows_fp8 applied to the copy afterwards."""
    M = 517
    x, dy = rnd((M, C), F32, 2.0, seed=80), rnd((M, C), BF, 0.3, seed=81)
    gamma = 1 + rnd((C,), F32, 0.2, seed=82)
    dy[11] = 0
    mean = x.mean(-1)
    rstd = torch.rsqrt(x.var(-1, unbiased=False) + 1e-6)
    xd, dyd, gd, md, rd = both([x, dy, gamma, mean, rstd])
    ws = torch.empty(hip.layernorm_bwd_workspace(M, C), dtype=torch.uint8, device="cuda")
    Kp = (C + 127) // 128 * 128
    outs = []
    for fused in (False, True):
        dx = torch.full((M, C), 0.25, device="cuda")
        dx[11] = 0
        cp, cs = torch.empty(M, C, dtype=BF, device="cuda"), torch.zeros(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        q, sc = torch.full((M, Kp), 0x55, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
        kw = dict(q8=q, q_scale=sc) if fused else {}
        hip.layernorm_bwd(dyd, xd, gd, md, rd, dx, mode, dg, db, True, ws, dx_copy=cp, copy_colsum=cs, **kw)
        if not fused:
            hip.quant_rows_fp8(cp, q, sc)
        outs.append((dx, cp, cs, dg, db, q, sc))
    for a, b, name in zip(outs[0], outs[1], ("dx", "copy", "colsum", "dgamma", "dbeta", "codes", "scales")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("Hd,M", [(2048, 333), (2752, 129), (64, 5), (4096, 17)])
def test_swiglu_backward_with_fused_fp8_quantiser(hip, ref, Hd, M):
    """cs_swiglu_bwd_q8: dx12 unchanged, and its e4m3 copy + row scales are bit-identical to cs_quant_rows_fp8 applied to dx12 afterwards."""
    dh = rnd((M, Hd), BF, 0.5, seed=70)
    x12 = rnd((M, 2 * Hd), BF, 1.5, seed=71)
    dh[3] = 0                                                       # an all-zero row: scale 1, codes 0
    dhd, xd = both([dh, x12])
    d0 = torch.empty(M, 2 * Hd, dtype=BF, device="cuda")
    hip.swiglu_bwd(dhd, xd, d0)
    Kp = (2 * Hd + 127) // 128 * 128
    d1 = torch.empty_like(d0)
    q1, s1 = torch.full((M, Kp), 0x55, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    hip.swiglu_bwd(dhd, xd, d1, q8=q1, q_scale=s1)
    assert torch.equal(d0, d1)
    q0, s0 = torch.full((M, Kp), 0xAA, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    hip.quant_rows_fp8(d0, q0, s0)
    assert torch.equal(s0, s1), "row scales"
    assert torch.equal(q0, q1), f"{int((q0 != q1).sum())} e4m3 codes differ"


@pytest.mark.parametrize("M,Hd", [(12608, 2048), (333, 2048), (577, 2752), (61, 64), (130, 1032)])
def test_swiglu_backward_with_fused_bias_gradients(hip, ref, M, Hd):
    """cs_swiglu_bwd_colsum (round 5): d x1|x2 unchanged and the accumulated column sums -- the w1 | w2 bias gradients -- bit-identical to
    cs_swiglu_bwd followed by cs_colsum_bf16 over the stored matrix (the 103 MB pass per block it removes); ragged row blocks, hidden widths that
    are not multiples of 512, and against the fp32 reference op."""
    dh = rnd((M, Hd), BF, 0.5, seed=72)
    x12 = rnd((M, 2 * Hd), BF, 1.5, seed=73)
    dhd, xd = both([dh, x12])
    ws = torch.empty(hip.colsum_workspace(M, 2 * Hd), dtype=torch.uint8, device="cuda")
    start = rnd((2 * Hd,), F32, seed=74).cuda()                     # the gradient slot is accumulated into, not assigned
    d0, c0 = torch.empty(M, 2 * Hd, dtype=BF, device="cuda"), start.clone()
    hip.swiglu_bwd(dhd, xd, d0)
    hip.colsum_bf16(d0, c0, ws)
    d1, c1 = torch.full((M, 2 * Hd), float("nan"), dtype=BF, device="cuda"), start.clone()
    hip.swiglu_bwd_colsum(dhd, xd, d1, c1, ws)
    assert torch.equal(d0, d1), f"{int((d0 != d1).sum())} elements of dx12 differ"
    assert torch.equal(c0, c1), f"{int((c0 != c1).sum())} of {2 * Hd} column sums differ"
    dr, cr = torch.empty(M, 2 * Hd, dtype=BF), start.cpu().clone()
    ref.swiglu_bwd_colsum(dh, x12, dr, cr)
    check(f"swiglu_bwd_colsum[{M},{Hd}].dx", d1, dr, TOL_BF)
    check(f"swiglu_bwd_colsum[{M},{Hd}].colsum", c1, cr, 2e-5 if M < 2000 else 2e-4)


@pytest.mark.parametrize("C,ld,xdt", [(768, 768, F32), (768, 768, BF), (2048, 2048, BF), (2730, 2752, BF), (64, 64, F32)])
def test_layernorm_forward_with_fused_fp8_quantiser(hip, ref, C, ld, xdt):
    """cs_layernorm_fwd_q8: y unchanged, and its e4m3 copy + row scales are bit-identical to cs_quant_rows_fp8 applied to y afterwards
    (the pass the fused form removes); padded storage (L/14: 2730 normalised columns in 2752-wide rows) quantises its padding to zero."""
    M = 300
    x = torch.zeros(M, ld, dtype=xdt)
    x[:, :C] = (rnd((M, C), F32, 2.0, seed=91) + 0.3).to(xdt)
    x[7] = 0                                                      # an all-zero row: scale 1, codes 0
    gamma, beta = torch.zeros(ld), torch.zeros(ld)
    gamma[:C], beta[:C] = 1 + rnd((C,), F32, 0.2, seed=92), rnd((C,), F32, 0.2, seed=93)
    beta[:C] *= 0 if C == 64 else 1
    Kp = (ld + 127) // 128 * 128
    xd, gd, bd = both([x, gamma, beta])
    y0 = torch.zeros(M, ld, dtype=BF, device="cuda")
    hip.layernorm_fwd(xd[:, :C], gd[:C], bd[:C], y0[:, :C])
    y1 = torch.zeros(M, ld, dtype=BF, device="cuda")
    q1, s1 = torch.full((M, Kp), 0x55, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    hip.layernorm_fwd(xd[:, :C], gd[:C], bd[:C], y1[:, :C], q8=q1, q_scale=s1)
    assert torch.equal(y0, y1)
    q0, s0 = torch.full((M, Kp), 0xAA, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    hip.quant_rows_fp8(y0, q0, s0)
    assert torch.equal(s0, s1), "row scales"
    assert torch.equal(q0, q1), f"{int((q0 != q1).sum())} e4m3 codes differ"
    assert int(q1[:, C:].abs().max() if C < Kp else 0) == 0


@pytest.mark.parametrize("shape,size", [((2, 3, 1024, 1024), 640), ((3, 3, 896, 896), 336), ((1, 3, 64, 64), 96), ((2, 3, 224, 224), 224)])
def test_multiscale_bilinear_resize_matches_torch(hip, ref, shape, size):
    """--multiscale (src/training/clipself.py:17-27): F.interpolate(images, size, mode='bilinear') as cs_resize_bilinear_f32."""
    x = rnd(shape, F32, seed=123)
    got = hip.resize_bilinear(x.cuda(), size)
    want = ref.resize_bilinear(x, size)
    check(f"resize_bilinear{list(shape)}->{size}", got, want, 1e-6)


@pytest.mark.parametrize("N,K,T", [(768, 768, 12608), (2304, 768, 12608), (4096, 768, 12608), (768, 2048, 12608), (256, 256, 64), (1024, 3072, 1152),
                                   (5504, 1024, 9232), (1024, 2752, 9232), (64, 64, 17), (344, 64, 51), (768, 768, 8194), (8, 264, 1)])
def test_gemm_wgrad_token_major_operands(hip, ref, N, K, T):
    """cs_gemm_wgrad_tn: dW += dY^T X straight from the token-major operands (transposing LDS reads, no transposed copies), against the
    fp32 product; accumulates into dW; ragged token counts and widths (L/14-336: 9232 tokens, hidden 2752; tiny towers: 17 tokens, width 64;
    the recipe's 8194 tokens); reports shapes it does not cover instead of computing them."""
    dY, X = rnd((T, N), BF, 0.5, seed=70), rnd((T, K), BF, 0.5, seed=71)
    base = rnd((N, K), F32, seed=72)
    need = hip.gemm_wgrad_tn_workspace(N, K, T)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    got = base.cuda().clone()
    hip.gemm_wgrad_tn(dY.cuda(), X.cuda(), got, ws)
    want = base + dY.float().T @ X.float()
    check(f"gemm_wgrad_tn[{N},{K},{T}]", got, want, 2e-5)
    again = base.cuda().clone()
    hip.gemm_wgrad_tn(dY.cuda(), X.cuda(), again, ws)
    assert torch.equal(again, got), "split-K through partials must be bit-reproducible"
    # strided operands (views into wider matrices), as the engine passes them
    wide = rnd((T, N + 256), BF, 0.5, seed=73)
    got2 = torch.zeros(N, K, device="cuda")
    hip.gemm_wgrad_tn(wide.cuda()[:, 256:], X.cuda(), got2, ws)
    check(f"gemm_wgrad_tn_strided[{N},{K},{T}]", got2, wide[:, 256:].float().T @ X.float(), 2e-5)
    assert hip.gemm_wgrad_tn_workspace(N + 4, K, T) == 0 and hip.gemm_wgrad_tn_workspace(N, K + 2, T) == 0      # widths must be multiples of 8


@pytest.mark.parametrize("M,N,K", [(1000, 768, 768), (2 * 197 * 7, 768, 2048), (300, 64, 64), (50432, 1024, 1024)])
def test_split_stream_residual_gemm_is_the_fp32_one_bit_for_bit(hip, ref, M, N, K):
    """cs_gemm_nt_ln_split: the residual stream as two 16-bit planes of bits(x) + 0x8000.  All three forms (fp32 in -> planes out, planes
    in -> planes out, planes in -> fp32 out) must reproduce the fp32 stream of cs_gemm_nt_ln (epilogue 6) bit for bit, statistics included;
    the hi plane is the bf16 operand of the next folded GEMM and equals the RNE copy except on exact ties; against the fp32 reference."""
    A = rnd((M, K), BF, seed=1).cuda()
    B = rnd((N, K), BF, 0.05, seed=2).cuda()
    bias, colsum = rnd((N,), seed=3).cuda(), rnd((N,), seed=4).cuda()
    mean, rstd = rnd((M,), seed=5, scale=0.1).cuda(), (rnd((M,), seed=6).abs() + 0.5).cuda()
    x0 = rnd((M, N), seed=7, scale=3.0).cuda()
    S = (N + 63) // 64

    def fp32_form(x_in, stats=True):
        x = x_in.clone()
        part = torch.zeros(S, M, 2, device="cuda") if stats else None
        xb = torch.zeros(M, N, dtype=BF, device="cuda") if stats else None
        hip.gemm_nt_ln(A, B, x, bias=bias, extra=x, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, stats_part=part, xb_out=xb, epi=6, flags=0xB0)
        return x, part, xb

    x1, part1, xb1 = fp32_form(x0)
    x2, part2, _ = fp32_form(x1)
    x3, _, _ = fp32_form(x2, stats=False)
    hi = torch.zeros(M, N, dtype=BF, device="cuda")
    lo = torch.zeros(M, N, dtype=torch.int16, device="cuda")
    p1, p2 = torch.zeros(S, M, 2, device="cuda"), torch.zeros(S, M, 2, device="cuda")
    hip.gemm_nt_ln_split(A, B, hi, lo, bias, mean, rstd, colsum, x_in=x0, stats_part=p1)
    assert torch.equal(RefOps.join_planes(hi, lo).view(torch.int32), x1.view(torch.int32)) and torch.equal(p1, part1)
    ties = int((hi != xb1).sum())
    assert ties <= max(4, M * N // 10000) and float((hi.float() - x1).abs().max()) <= float((xb1.float() - x1).abs().max()) * 1.0001
    hip.gemm_nt_ln_split(A, B, hi, lo, bias, mean, rstd, colsum, stats_part=p2)
    assert torch.equal(RefOps.join_planes(hi, lo).view(torch.int32), x2.view(torch.int32)) and torch.equal(p2, part2)
    out = torch.zeros(M, N, device="cuda")
    hip.gemm_nt_ln_split(A, B, hi, lo, bias, mean, rstd, colsum, x_out=out)
    assert torch.equal(out.view(torch.int32), x3.view(torch.int32))
    want = x0.cpu()
    acc = rstd.cpu()[:, None] * (A.cpu().float() @ B.cpu().float().T - mean.cpu()[:, None] * colsum.cpu()[None, :]) + bias.cpu()
    with open(_LOG, "a") as f:
        f.write(f"split stream M={M} N={N} K={K}: bit-equal to the fp32 stream in all three forms; hi plane differs from the RNE copy at {ties} ties\n")
    check("split stream vs reference", x1.cpu(), want + acc, 2e-3)
