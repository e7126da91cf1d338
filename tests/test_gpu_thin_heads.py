"""`-m gpu`: the thin 1 x 1 convolutions and the two heads built on them, on the MI355X.

Kernels alone (HipOps.thin_fwd / thin_dgrad, epilogues 10 / 11 of cs_gemm_nt): against the np.float32 restatement of the header's text
(tests/_thin_ref.RefOpsThin) -- bit for bit on exact operands, inside the derived bounds on random ones -- over every N, K and geometry
the layouts distinguish, rows and planes forms, both element types of the K-wide rows, padded row strides, with and without bias,
second block and gate; every call made twice for equal bits into NaN-filled outputs; the grid-stride wrap; the poisoned halos of
tests/_extents.py; the header's rejections.  Then the layers and the modules on HipOps: exact operands bit for bit against float64
autograd, the chain into det_losses.rpn_loss and det_proposals.rpn_proposals, and the modules with norm against the fp32 twin."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from _thin_ref import (BF, F32, LAYER_SHAPES, LAYOUTS, PARITY_REL_L2, RefOpsThin, check_dy_rounding, check_exact, check_thin, exact_case,  # noqa: E402
                       copy_state, make_module, parity, run_module, same_bits)

U = 2.0 ** -24
N_SET, K_SET = [1, 3, 4, 12, 15, 16], [64, 256, 320]
# (B, h, w): M = 105 is no multiple of 16 and R = 35 takes the one-element store path | R = 16 | one pixel | R = 128, several tiles per image
GEOMS = [(3, 5, 7), (2, 4, 4), (1, 1, 1), (2, 16, 8)]
_INT = {BF: torch.int16, F32: torch.int32}
NAN_BITS = {BF: 0x7FA5, F32: 0x7FA5A5A5}
BLOCKS_PER_CU, ROWS_PER_BLOCK = 8, 64                                    # the grid cap of include/clipself_hip.h: a wave owns 16 rows at a time


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOpsThin()


def _nan(shape, dtype):
    return torch.full(shape, NAN_BITS[dtype], dtype=_INT[dtype]).view(dtype)


def _place(data, ld, dtype):
    """[rows, C] view with row stride ld holding data as dtype; the padding columns hold NaN."""
    buf = _nan((data.shape[0], ld), dtype)
    buf[:, :data.shape[1]] = data.to(dtype)
    return buf


def _bits_equal(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.cpu().contiguous().view(_INT[got.dtype]), want.contiguous().view(_INT[want.dtype])
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, kind):
    """x fp32 [M, K] (exact: integers; random: fp32 values that bf16 does NOT hold, so the fp32 form rounds), W, bias, dy [M, N] and a gate
    with zeros, negatives and positives -- computed once, shared read-only."""
    g = torch.Generator().manual_seed(M * 7919 + N * 131 + K + (kind == "exact"))
    if kind == "exact":
        r = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)
        x, w, b, dy = r(M, K), r(N, K), r(N), r(M, N)
    else:
        r = lambda *s: torch.randn(*s, generator=g)
        x, w, b, dy = r(M, K), (r(N, K) * K ** -0.5).to(BF).to(F32), r(N), r(M, N)
    gate = torch.randint(-1, 3, (M, K), generator=g).to(F32) * 0.5
    return x, w, b, dy, gate


def _within(got, want64, bound, what):
    err = (got.cpu().double() - want64).abs()
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the bound, worst {float((err / bound.clamp_min(1e-300)).max()):.3f} x"


def _forward_forms(M, N, R):
    forms = [("rows", 0, None), ("planes", R, None)]
    if N == 15:
        forms.append(("planes", R, 3))
    return forms


def _check_fwd(hip, ref, geom, N, K, kind):
    B, h, w = geom
    M, R = B * h * w, h * w
    x, W, b, _, _ = _operands(M, N, K, kind)
    Wd = W.to(BF).cuda()
    for xdt in (BF, F32):
        xin = x.to(BF).to(F32) if xdt == BF else x
        y64 = xin.to(BF).double() @ W.double().T
        ay = xin.to(BF).double().abs() @ W.double().abs().T
        for ld, bias in ((K, b), (K + 8, None)):
            Xh = _place(xin, ld, xdt)
            want64 = y64 + (bias.double() if bias is not None else 0)
            bound = 2.0 * (K + 2) * U * (ay + (bias.double().abs() if bias is not None else 0))
            for form, Rf, split in _forward_forms(M, N, R):
                ldc = N + 3 if (form == "rows" and ld != K) else N
                want = _nan((M, ldc), F32) if form == "rows" else _nan((M * N,), F32)
                ref.thin_fwd(Xh[:, :K], W.to(BF), bias, want[:, :N] if form == "rows" else want, R=Rf, split=split)
                runs = []
                for _ in range(2):
                    out = want.clone().view(torch.int32).fill_(NAN_BITS[F32]).view(F32).cuda()
                    hip.thin_fwd(Xh.cuda()[:, :K], Wd, None if bias is None else bias.cuda(), out[:, :N] if form == "rows" else out, R=Rf, split=split)
                    runs.append(out)
                what = f"thin_fwd {kind} {geom} N={N} K={K} {xdt} lda={ld} {form} split={split} bias={bias is not None}"
                assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), what + ": two calls, different bits"
                if kind == "exact":
                    _bits_equal(runs[0], want, what)                             # the NaN padding columns included
                else:
                    got = runs[0][:, :N] if form == "rows" else _planes_to_rows(runs[0].cpu(), M, N, R, split)
                    _within(got, want64, bound, what)
                    if form == "rows" and ldc > N:
                        assert bool(torch.isnan(runs[0][:, N:]).all()), what + ": columns >= N were touched"


def _planes_to_rows(flat, M, N, R, split):
    s = N if split is None else split
    a = flat[:M * s].view(M // R, s, R).permute(0, 2, 1).reshape(M, s)
    if s == N:
        return a
    return torch.cat([a, flat[M * s:].view(M // R, N - s, R).permute(0, 2, 1).reshape(M, N - s)], 1)


def _rows_to_planes(rows, R, c0, c1):
    M = rows.shape[0]
    return rows[:, c0:c1].reshape(M // R, R, c1 - c0).permute(0, 2, 1).contiguous()


def _check_dgrad(hip, ref, geom, N, K, kind):
    B, h, w = geom
    M, R = B * h * w, h * w
    _, W, _, dy, gate = _operands(M, N, K, kind)
    Wd = W.to(BF).cuda()
    dyb = dy.to(BF).double()
    dx64, adx = dyb @ W.double(), dyb.abs() @ W.double().abs()
    forms = [("rows", 0, N), ("planes", R, N)] + ([("planes", R, 3)] if N == 15 else [])
    for ddt in (BF, F32):
        for ld, use_gate in ((K, False), (K + 8, True)):
            g = _place(gate, ld, BF) if use_gate else None
            want64 = torch.where(gate <= 0, torch.zeros((), dtype=torch.float64), dx64) if use_gate else dx64
            bound = 2.0 * (N + 2) * U * adx
            if ddt == BF:
                bound = bound + 2.0 ** -8 * (want64.abs() + bound)
            for form, Rf, s in forms:
                if form == "rows":
                    d1, d2 = dy.contiguous(), None
                else:
                    d1, d2 = _rows_to_planes(dy, R, 0, s), (_rows_to_planes(dy, R, s, N) if s < N else None)
                want = _nan((M, ld), ddt)
                ref.thin_dgrad(d1, W.to(BF), want[:, :K], R=Rf, dY2=d2, gate=None if g is None else g[:, :K])
                runs = []
                for _ in range(2):
                    out = _nan((M, ld), ddt).cuda()
                    hip.thin_dgrad(d1.cuda(), Wd, out[:, :K], R=Rf, dY2=None if d2 is None else d2.cuda(), gate=None if g is None else g.cuda()[:, :K])
                    runs.append(out)
                what = f"thin_dgrad {kind} {geom} N={N} K={K} {ddt} ld={ld} {form} s={s} gate={use_gate}"
                assert torch.equal(runs[0].view(_INT[ddt]), runs[1].view(_INT[ddt])), what + ": two calls, different bits"
                if kind == "exact":
                    _bits_equal(runs[0], want, what)
                else:
                    _within(runs[0][:, :K], want64, bound, what)
                    if ld > K:
                        assert bool(torch.isnan(runs[0][:, K:].float()).all()), what + ": columns >= K were touched"


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("K", K_SET)
@pytest.mark.parametrize("N", N_SET)
def test_thin_fwd_is_the_headers_text(hip, ref, N, K, kind):
    assert hip.THIN_HEADS
    for geom in GEOMS:
        _check_fwd(hip, ref, geom, N, K, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("K", K_SET)
@pytest.mark.parametrize("N", N_SET)
def test_thin_dgrad_is_the_headers_text(hip, ref, N, K, kind):
    for geom in GEOMS:
        _check_dgrad(hip, ref, geom, N, K, kind)


@pytest.mark.parametrize("K", K_SET)
def test_fp32_rows_give_the_bits_of_cast_then_bf16(hip, K):
    M, N, R = 105, 15, 35
    x, W, b, _, _ = _operands(M, N, K, "random")
    pad = torch.zeros(M * K % 8 and 8 - M * K % 8)
    xc = torch.cat([x.reshape(-1), pad]).cuda()                          # cs_cast_f32_bf16 takes multiples of 8
    xb = torch.empty_like(xc, dtype=BF)
    hip.cast_f32_bf16(xc, xb)
    Wd, bd = W.to(BF).cuda(), b.cuda()
    a, c = _nan((M * N,), F32).cuda(), _nan((M * N,), F32).cuda()
    hip.thin_fwd(x.cuda(), Wd, bd, a, R=R, split=3)
    hip.thin_fwd(xb[:M * K].view(M, K), Wd, bd, c, R=R, split=3)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and not bool(torch.isnan(a).any())


def test_the_grid_stride_loop_wraps_past_the_cap(hip, ref):
    cap_rows = BLOCKS_PER_CU * hip.num_cus * ROWS_PER_BLOCK
    B, R, N, K = 3, (cap_rows + 1024) // 3 // 4 * 4 + 4, 15, 64              # 3 * R rows > the cap: the loop goes round again; ~17 MB of X
    M = B * R
    assert M > cap_rows + 16 and R % 4 == 0
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(-8, 9, (M, K), generator=g, device="cuda").to(BF)
    W = torch.randint(-8, 9, (N, K), generator=g, device="cuda").to(BF)
    b = torch.randint(-8, 9, (N,), generator=g, device="cuda").to(F32)
    out = _nan((M * N,), F32).cuda()
    hip.thin_fwd(x, W, b, out, R=R, split=3)
    want = _nan((M * N,), F32)
    ref.thin_fwd(x.cpu(), W.cpu(), b.cpu(), want, R=R, split=3)
    _bits_equal(out, want, "thin_fwd past the grid cap")
    y = _planes_to_rows(out.cpu(), M, N, R, 3)
    gate = (torch.randint(-1, 2, (M, K), generator=g, device="cuda").to(BF))
    dx = _nan((M, K), BF).cuda()
    hip.thin_dgrad(out[:M * 3], W, dx, R=R, dY2=out[M * 3:], gate=gate)
    want_dx = _nan((M, K), BF)
    ref.thin_dgrad(want[:M * 3], W.cpu(), want_dx, R=R, dY2=want[M * 3:], gate=gate.cpu())
    _bits_equal(dx, want_dx, "thin_dgrad past the grid cap")
    assert float(y.abs().max()) > 0


def _halo_case(geom, N, K, kdt, form, split, fwd):
    B, h, w = geom
    M, R = B * h * w, h * w
    Rf = R if form == "planes" else 0
    s = N if split is None else split

    def fn(ops, a):
        x, W, b, dy, gate = _operands(M, N, K, "random")
        Wd = a.inp(W.to(BF), a.ld(K, 8))
        if fwd:
            X = a.inp(x.to(kdt), a.ld(K, 8))
            bias = a.inp(b)
            out = a.out((M, N), F32, ld=a.ld(N)) if form == "rows" else a.out((M * N,), F32)
            ops.thin_fwd(X, Wd, bias, out, R=Rf, split=split)
            return {"y": out}
        if form == "rows":
            d1, d2 = a.inp(dy.contiguous()), None
        else:
            d1, d2 = a.inp(_rows_to_planes(dy, R, 0, s)), (a.inp(_rows_to_planes(dy, R, s, N)) if s < N else None)
        g = a.inp(gate.to(BF), a.ld(K, 8))
        dX = a.out((M, K), kdt, ld=a.ld(K, 8))
        ops.thin_dgrad(d1, Wd, dX, R=Rf, dY2=d2, gate=g)
        return {"dx": dX}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("geom,N,K", [((3, 5, 7), 15, 64), ((2, 4, 4), 1, 256), ((1, 1, 1), 16, 320), ((2, 16, 8), 12, 256)])
def test_kernels_stay_inside_their_extents(hip, geom, N, K, pad):
    for kdt in (BF, F32):
        for form, split in (("rows", None), ("planes", None)) + ((("planes", 3),) if N == 15 else ()):
            for fwd in (True, False):
                key = f"{'thin_fwd' if fwd else 'thin_dgrad'}[{geom},{N},{K},{kdt},{form},{split}]"
                problems = run_case(hip, _halo_case(geom, N, K, kdt, form, split, fwd), "cuda", pad, key=key)
                assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_entry_point_refuses_what_the_header_lists(hip):
    M, N, K, R = 32, 15, 64, 16
    X = torch.ones(M, K + 8, device="cuda", dtype=BF)
    W = torch.ones(N + 2, K, device="cuda", dtype=BF)
    Y = torch.full((M * 17 + 4,), 7.0, device="cuda")
    dX = torch.full((M, K + 8), 7.0, device="cuda", dtype=BF)
    d2 = torch.ones(M * 12, device="cuda")
    p = lambda t: t.data_ptr()

    def fwd(A=p(X), B=p(W), C=p(Y), M=M, N=N, K=K, lda=K + 8, ldb=K, ldc=3, splits=1, group=R, flags=0):
        return hip.lib.cs_gemm_nt(A, B, C, None, None, M, N, K, lda, ldb, ldc, 10, splits, group, flags, None)

    def bwd(A=p(Y), B=p(W), C=p(dX), bias=p(d2), extra=None, M=M, N=N, K=K, lda=3, ldb=K, ldc=K + 8, splits=1, group=R, flags=0):
        return hip.lib.cs_gemm_nt(A, B, C, bias, extra, M, N, K, lda, ldb, ldc, 11, splits, group, flags, None)

    def refused(rc):
        return rc == -1 and b"thin" in hip.lib.cs_last_error()

    for call in (fwd, bwd):
        assert refused(call(N=17)) and refused(call(N=0)) and refused(call(K=96)) and refused(call(K=0)) and refused(call(M=0))
        assert refused(call(group=5)) and refused(call(group=-1))                               # M % R != 0
        assert refused(call(splits=2)) and refused(call(splits=0))
        assert refused(call(ldb=K - 8)) and refused(call(ldb=K + 4)) and refused(call(B=p(W) + 2))
    assert refused(fwd(ldc=0)) and refused(fwd(ldc=16))                                         # s outside [1, N]
    assert refused(fwd(group=0, ldc=N - 1))                                                     # rows form: a stride below N
    assert refused(fwd(lda=K - 8)) and refused(fwd(lda=K + 4)) and refused(fwd(A=p(X) + 2)) and refused(fwd(lda=K + 2, flags=1))
    assert refused(fwd(C=p(Y) + 2))
    assert refused(bwd(lda=0)) and refused(bwd(lda=16))
    assert refused(bwd(group=0, lda=N - 1, bias=None))
    assert refused(bwd(ldc=K - 8)) and refused(bwd(ldc=K + 4)) and refused(bwd(C=p(dX) + 2))
    assert refused(bwd(bias=None)) and refused(bwd(lda=N)) and refused(bwd(group=0, lda=N))     # second block <-> s < N; none in the rows form
    assert refused(bwd(extra=p(X) + 2))
    torch.cuda.synchronize()
    assert float(Y.min()) == 7.0 and float(Y.max()) == 7.0 and float(dX.float().min()) == 7.0 and float(dX.float().max()) == 7.0
    assert fwd() == 0                                                                           # and the next valid call succeeds
    torch.cuda.synchronize()
    assert float(Y[:M * N].min()) == float(K) and float(Y[M * N:].min()) == 7.0
    with pytest.raises(AssertionError):
        hip.thin_fwd(X[:, :K], W[:N], None, Y[:M * N], R=R, split=16)
    with pytest.raises(AssertionError):
        hip.thin_dgrad(Y[:M * 3], W[:N], dX[:, :K], R=R)                                        # a split below N needs the second block
    for epi in (12, 13):
        assert hip.lib.cs_gemm_nt(p(X), p(W), p(Y), None, None, M, 16, K, K + 8, K, 16, epi, 1, 0, 0, None) == -1
        assert b"unknown epilogue" in hip.lib.cs_last_error()


# ------------------------------------------------------------------------------------------------ the layers
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_conv1x1thin_against_float64_autograd(hip, shape, layout, dtype, kind):
    check_thin(hip, shape, layout, dtype, kind, device="cuda")


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape,widths", [((105, 64, 15), [3, 12]), ((32, 256, 16), [4, 12]), ((256, 320, 12), [11, 1])])
def test_thin_heads_pair_against_float64_autograd(hip, shape, widths, layout, dtype, kind):
    check_thin(hip, shape, layout, dtype, kind, widths=widths, device="cuda")


def test_the_input_gradient_rounds_dy_to_bf16(hip):
    check_dy_rounding(hip, device="cuda")


# ------------------------------------------------------------------------------------------------ the modules
@pytest.mark.parametrize("kind", ["rpn2", "rpn1", "mask"])
def test_module_exact_operands_bit_for_bit(hip, kind):
    outs = check_exact(kind, hip, device="cuda")
    assert all(o.is_cuda and o.is_contiguous() and o.dtype == F32 for o in outs)


def test_rpn_head_feeds_the_loss_and_the_proposals_without_a_copy(hip):
    """The three-level pyramid [2, 64, 8, 8], [2, 64, 4, 4], [2, 64, 2, 2] of the exact case: the head's outputs go into rpn_loss and
    rpn_proposals as they are, and backward() reaches every parameter and the input maps."""
    from clipself_amd import det_losses, det_proposals
    from clipself_amd.det_backend import f32c
    twin, xs, _, outs, _ = exact_case("rpn2")
    m = copy_state(make_module("rpn2", hip), twin).cuda()
    ins = [x.cuda().requires_grad_(True) for x in xs]
    cls, reg = m(ins)
    A, B = 3, 2
    for i, (c, r) in enumerate(zip(cls, reg)):
        assert c.dtype == F32 and r.dtype == F32 and c.is_contiguous() and r.is_contiguous() and f32c(c) is c and f32c(r) is r
        assert tuple(c.shape) == (B, A, *xs[i].shape[2:]) and tuple(r.shape) == (B, 4 * A, *xs[i].shape[2:])
        same_bits(c, outs[i], f"cls {i}")
        same_bits(r, outs[3 + i], f"reg {i}")
    N = sum(c.shape[2] * c.shape[3] * A for c in cls)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 2, (B, N), generator=g)                    # 0 = object, 1 = background (num_classes = 1)
    lw = (torch.rand(B, N, generator=g) < 0.5).float()
    bt = torch.randn(B, N, 4, generator=g)
    bw = ((labels == 0) & (lw > 0)).float()[..., None].expand(B, N, 4).contiguous()
    losses = det_losses.rpn_loss(cls, reg, labels.cuda(), lw.cuda(), bt.cuda(), bw.cuda(), torch.tensor(float(lw.sum()), device="cuda"),
                                 ops=hip, fused=True)
    assert len(losses["loss_rpn_cls"]) == 3 and len(losses["loss_rpn_bbox"]) == 3
    total = sum(losses["loss_rpn_cls"]) + sum(losses["loss_rpn_bbox"])
    total.backward()
    assert bool(torch.isfinite(total))
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, name
    for t in ins:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().sum()) > 0
    # the same maps, detached, as the proposal stage reads them
    anchors = []
    for lvl, c in enumerate(cls):
        h, w, stride = c.shape[2], c.shape[3], 4 * 2 ** lvl
        ys, xs_ = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        ctr = torch.stack([xs_, ys, xs_, ys], -1).reshape(-1, 1, 4).float() * stride
        half = torch.tensor([[-8.0, -4.0, 8.0, 4.0], [-6.0, -6.0, 6.0, 6.0], [-4.0, -8.0, 4.0, 8.0]]) * 2 ** lvl
        anchors.append((ctr + half[None]).reshape(-1, 4))
    anchors = torch.cat(anchors).cuda()
    cfg = dict(nms_pre=50, max_per_img=20, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)
    props, counts = det_proposals.rpn_proposals([c.detach() for c in cls], [r.detach() for r in reg], anchors, [(64, 64)] * B, cfg, ops=hip, fused=True)
    assert tuple(props.shape) == (B, 20, 5) and int(counts.min()) >= 1 and bool(torch.isfinite(props).all())


@pytest.mark.parametrize("kind", ["rpn2", "mask1"])
def test_module_with_norm_against_the_fp32_twin(hip, kind):
    """Measured on the MI355X: profiles/thin_heads_parity.md (outputs against the plain fp32 twin, gradients against the twin with the
    module's own ReLU gates handed in; threshold 3.4e-3)."""
    worst = parity(kind, hip, device="cuda", tag="MI355X")
    assert max(worst) <= PARITY_REL_L2, (worst, PARITY_REL_L2)


@pytest.mark.parametrize("kind", ["rpn2", "mask"])
def test_module_repeats_its_bits(hip, kind):
    twin, xs, gs, _, _ = exact_case(kind)
    m = copy_state(make_module(kind, hip), twin).cuda()
    first = run_module(m, xs, gs, device="cuda")
    again = run_module(m, xs, gs, device="cuda")
    for a, b in zip(first[0] + first[1] + list(first[2].values()), again[0] + again[1] + list(again[2].values())):
        assert torch.equal(a, b)
