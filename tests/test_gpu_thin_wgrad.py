"""`-m gpu`: epilogue 12 of cs_gemm_nt -- the thin layers' weight and bias gradient -- and the modules built on it, on the MI355X.

The kernel alone (HipOps.thin_wgrad) against the np.float32 restatement of the header's text (tests/_thin_wgrad_ref.RefOpsThinWgrad) and
float64: bit for bit on exact operands, inside 2 * (M + 2) * 2^-24 * sum|terms| on random ones, over every N, K and geometry the code
paths distinguish, rows and planes forms, bf16 and fp32 X, padded strides, NaN-filled dW and workspace, every call twice; more than one
partial and the grid-stride wrap; the poisoned halos of tests/_extents.py; the header's rejections.  Then Conv1x1Thin / thin_heads /
the RPN and mask heads / LinearThin / ConvFCBBoxHead on HipOps with the direct route forced on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fc_ref  # noqa: E402
from _extents import run_case  # noqa: E402
from _thin_ref import BF, F32, LAYER_SHAPES, LAYOUTS, check_exact, check_thin, copy_state, exact_case, make_module, run_module  # noqa: E402
from _thin_wgrad_ref import (RefOpsThinWgrad, U, check_linear, check_result, dy_forms, operands, reference, rounding_case,  # noqa: E402
                             rows_to_planes)

N_SET, K_SET = [1, 3, 4, 12, 15, 16], [64, 256, 320]
# M = 105: no multiple of the 32-row step, R = 35: the element path, runs straddle images | R = 16 | M = 1 | R = 128 | R = 12: % 4 but not % 8
GEOMS = [(3, 5, 7), (2, 4, 4), (1, 1, 1), (2, 16, 8), (2, 3, 4)]
NAN32 = 0x7FA5A5A5


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOpsThinWgrad()


def _nan(shape, dtype=F32):
    if dtype == BF:
        return torch.full(shape, 0x7FA5, dtype=torch.int16).view(BF)
    return torch.full(shape, NAN32, dtype=torch.int32).view(F32)


def _place(data, ld, dtype):
    buf = _nan((data.shape[0], ld), dtype)
    buf[:, :data.shape[1]] = data.to(dtype)
    return buf


def _run(hip, x, dy, form, xdt, ldb, ldc, lda=None):
    """One call into NaN-filled buffers -> (dW buffer [16, ldc], workspace), on the device."""
    name, R, d1, d2 = form
    M, K = x.shape
    N = dy.shape[1]
    X = _place(x, ldb, xdt).cuda()[:, :K]
    d1 = _place(d1, lda, F32).cuda()[:, :N] if (name == "rows" and lda) else d1.cuda()
    dW = _nan((16, ldc)).cuda()
    ws = _nan((hip.thin_wgrad_workspace(M, N, K),)).cuda()
    hip.thin_wgrad(d1, X, dW[:N, :K], R=R, dY2=None if d2 is None else d2.cuda(), workspace=ws)
    return dW, ws


def _check(hip, ref, geom, N, K, kind):
    B, h, w = geom
    M, R = B * h * w, h * w
    x, dy = operands(M, N, K, kind)
    for xdt in (BF, F32):
        xin = x.to(BF).to(F32) if xdt == BF else x
        for ldb, ldc, lda in ((K, K, None), (K + 8, K + 4, N + 3)):
            for form in dy_forms(dy, R, N):
                what = f"thin_wgrad {kind} {geom} N={N} K={K} {xdt} ldb={ldb} ldc={ldc} {form[0]}"
                a, wa = _run(hip, xin, dy, form, xdt, ldb, ldc, lda)
                b, wb = _run(hip, xin, dy, form, xdt, ldb, ldc, lda)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(wa[:16].view(torch.int32), wb[:16].view(torch.int32)), \
                    what + ": two calls, different bits"
                keep = torch.ones(16, ldc, dtype=torch.bool)
                keep[:N, :K] = False
                assert bool((a.cpu().view(torch.int32)[keep] == NAN32).all()), what + ": rows >= N or columns >= K were touched"
                assert float(wa[N:16].abs().sum()) == 0 and not bool(torch.isnan(wa[:16]).any()), what + ": workspace[N .. 16) must hold zeros"
                check_result(a[:N, :K], wa[:N], xin, dy, kind, what)
                if kind == "exact":                                          # and the restatement's own bits
                    want = _nan((16, ldc))
                    wsr = torch.empty(ref.thin_wgrad_workspace(M, N, K))
                    ref.thin_wgrad(form[2], xin.to(xdt), want[:N, :K], R=form[1], dY2=form[3], workspace=wsr)
                    assert torch.equal(a.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(wa[:16].cpu(), wsr[:16]), what


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("K", K_SET)
@pytest.mark.parametrize("N", N_SET)
def test_thin_wgrad_is_the_headers_text(hip, ref, N, K, kind):
    assert hip.THIN_WGRAD
    for geom in GEOMS:
        _check(hip, ref, geom, N, K, kind)


@pytest.mark.parametrize("K", K_SET)
def test_fp32_rows_give_the_bits_of_cast_then_bf16(hip, K):
    M, N, R = 105, 15, 35
    x, dy = operands(M, N, K, "random")
    assert not torch.equal(x.to(BF).to(F32), x)
    pad = torch.zeros(M * K % 8 and 8 - M * K % 8)
    xc = torch.cat([x.reshape(-1), pad]).cuda()
    xb = torch.empty_like(xc, dtype=BF)
    hip.cast_f32_bf16(xc, xb)
    d1, d2 = rows_to_planes(dy, R, 0, 3).cuda(), rows_to_planes(dy, R, 3, N).cuda()
    a, c = _nan((N, K)).cuda(), _nan((N, K)).cuda()
    wa = hip.thin_wgrad(d1, x.cuda(), a, R=R, dY2=d2)
    wc = hip.thin_wgrad(d1, xb[:M * K].view(M, K), c, R=R, dY2=d2)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(wa[:16], wc[:16]) and not bool(torch.isnan(a).any())


def test_dy_is_rounded_to_bf16_for_both_sums(hip):
    x, dy = rounding_case()
    for form in dy_forms(dy, 35, 15):
        dW, ws = _run(hip, x, dy, form, F32, 64, 64)
        check_result(dW[:15, :64], ws[:15], x, dy, "exact", f"dY that bf16 does not hold, {form[0]}")


@pytest.mark.parametrize("tail_only", [False, True])
def test_more_than_one_partial_and_the_wrap(hip, tail_only):
    """M = the rows the capped grid covers in one sweep + one ragged step: every workgroup leaves a partial, workgroup 0 goes round
    again.  tail_only: dY is zero except in the last row, so that a dropped tail shows."""
    from clipself_amd.hip import THIN_WGRAD_BLOCKS_PER_CU, THIN_WGRAD_STEP_ROWS, THIN_WGRAD_WG_ROWS
    N, K = 3, 64
    sweep = THIN_WGRAD_BLOCKS_PER_CU * hip.num_cus * THIN_WGRAD_WG_ROWS
    M = sweep + THIN_WGRAD_STEP_ROWS - 5
    assert hip.thin_wgrad_partials(M) == THIN_WGRAD_BLOCKS_PER_CU * hip.num_cus and M % THIN_WGRAD_STEP_ROWS != 0
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-1, 2, (M, K), generator=g).to(F32)
    dy = torch.randint(-1, 2, (M, N), generator=g).to(F32)
    if tail_only:
        dy[:-1] = 0
        dy[-1] = torch.tensor([1.0, -1.0, 1.0])
        x[-1, ::2] = 1
    dw64, db64 = dy.double().T @ x.double(), dy.double().sum(0)
    assert float((dy.abs().T @ x.abs()).max()) < 2 ** 24                      # every sum is exact in fp32, in any order
    for name, R, d1, d2 in (("rows", 0, dy, None), ("planes", M, rows_to_planes(dy, M, 0, 1), rows_to_planes(dy, M, 1, N))):
        for xdt in (BF, F32):
            dW = _nan((N, K)).cuda()
            ws = _nan((hip.thin_wgrad_workspace(M, N, K),)).cuda()
            hip.thin_wgrad(d1.cuda(), x.to(xdt).cuda(), dW, R=R, dY2=None if d2 is None else d2.cuda(), workspace=ws)
            assert torch.equal(dW.cpu().double(), dw64) and torch.equal(ws[:N].cpu().double(), db64), f"{name} {xdt} tail_only={tail_only}"
            assert float(ws[N:16].abs().sum()) == 0
    assert float(dw64.abs().max()) > 0


def _halo_case(geom, N, K, xdt, form):
    B, h, w = geom
    M, R = B * h * w, h * w

    def fn(ops, a):
        x, dy = operands(M, N, K, "random")
        X = a.inp(x.to(xdt), a.ld(K, 8))
        if form == "rows":
            Rf, d1, d2 = 0, a.inp(dy.contiguous(), a.ld(N)), None
        else:
            s = 3 if form == "planes3" else N
            Rf, d1, d2 = R, a.inp(rows_to_planes(dy, R, 0, s)), (a.inp(rows_to_planes(dy, R, s, N)) if s < N else None)
        dW = a.out((N, K), F32, ld=a.ld(K, 4))
        ws = a.out((ops.thin_wgrad_workspace(M, N, K),), F32, name="workspace", halo=1 << 14)
        ops.thin_wgrad(d1, X, dW, R=Rf, dY2=d2, workspace=ws)
        return {"dW": dW, "db": ws[:16]}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("geom,N,K", [((3, 5, 7), 15, 64), ((2, 4, 4), 1, 256), ((1, 1, 1), 16, 320), ((2, 16, 8), 12, 256)])
def test_kernel_stays_inside_its_extents(hip, geom, N, K, pad):
    for xdt in (BF, F32):
        for form in ("rows", "planes") + (("planes3",) if N == 15 else ()):
            key = f"thin_wgrad[{geom},{N},{K},{xdt},{form}]"
            problems = run_case(hip, _halo_case(geom, N, K, xdt, form), "cuda", pad, key=key)
            assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_entry_point_refuses_what_the_header_lists(hip):
    M, N, K, R = 32, 15, 64, 16
    X = torch.ones(M, K + 8, device="cuda", dtype=BF)
    dY = torch.ones(M * 17 + 4, device="cuda")
    d2 = torch.ones(M * 12, device="cuda")
    dW = torch.full((16, K + 8), 7.0, device="cuda")
    ws = torch.full((hip.thin_wgrad_workspace(M, N, K) + 8,), 7.0, device="cuda")
    p = lambda t: t.data_ptr()

    def call(A=p(dY), B=p(X), C=p(dW), bias=p(d2), extra=p(ws), M=M, N=N, K=K, lda=3, ldb=K + 8, ldc=K + 8, splits=1, group=R, flags=0):
        return hip.lib.cs_gemm_nt(A, B, C, bias, extra, M, N, K, lda, ldb, ldc, 12, splits, group, flags, None)

    def refused(rc):
        return rc == -1 and b"thin weight gradient" in hip.lib.cs_last_error()

    assert refused(call(N=17)) and refused(call(N=0)) and refused(call(K=96)) and refused(call(K=0)) and refused(call(M=0))
    assert refused(call(group=5)) and refused(call(group=-1))                                   # M % R != 0
    assert refused(call(lda=0)) and refused(call(lda=16))                                       # s outside [1, N]
    assert refused(call(bias=None)) and refused(call(lda=N)) and refused(call(group=0, lda=N))  # second block <-> s < N; none in the rows form
    assert refused(call(group=0, lda=N - 1, bias=None))                                         # rows form: a stride below N
    assert refused(call(ldb=K - 8)) and refused(call(ldb=K + 4)) and refused(call(B=p(X) + 2)) and refused(call(ldb=K + 2, flags=1))
    assert refused(call(ldc=K - 4)) and refused(call(ldc=K + 2)) and refused(call(C=p(dW) + 4))
    assert refused(call(extra=None)) and refused(call(extra=p(ws) + 4))
    assert refused(call(splits=2)) and refused(call(splits=0))
    torch.cuda.synchronize()
    assert float(dW.min()) == 7.0 and float(dW.max()) == 7.0 and float(ws.min()) == 7.0 and float(ws.max()) == 7.0
    assert call() == 0                                                                          # and the next valid call succeeds
    torch.cuda.synchronize()
    assert float(dW[:N, :K].min()) == float(M) and float(dW[:N, :K].max()) == float(M) and float(dW[N:].min()) == 7.0 and float(dW[:, K:].min()) == 7.0
    assert ws[:N].tolist() == [float(M)] * N and ws[N:16].tolist() == [0.0] * (16 - N)
    with pytest.raises(ValueError):
        hip.thin_wgrad(dY[:M * N].view(M, N), X[:, :K], dW[:N, :K], workspace=ws[:hip.thin_wgrad_workspace(M, N, K) - 1])
    with pytest.raises(ValueError):
        hip.thin_wgrad(dY[:M * N].view(M, N), X[:, :K], dW[:N, :K], workspace=ws.double())
    with pytest.raises(AssertionError):
        hip.thin_wgrad(dY[:M * 3], X[:, :K], dW[:N, :K], R=5)                                   # M % R != 0


# ------------------------------------------------------------------------------------------------ the layers, both routes
@pytest.fixture(params=[True, False], ids=["direct", "padded"])
def route(request, monkeypatch):
    from clipself_amd import conv
    monkeypatch.setattr(conv, "THIN_WGRAD_DEFAULT", request.param)
    return request.param


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_conv1x1thin_against_float64_autograd(hip, route, shape, layout, dtype, kind):
    check_thin(hip, shape, layout, dtype, kind, device="cuda")


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape,widths", [((105, 64, 15), [3, 12]), ((32, 256, 16), [4, 12]), ((256, 320, 12), [11, 1])])
def test_thin_heads_pair_against_float64_autograd(hip, route, shape, widths, layout, dtype, kind):
    check_thin(hip, shape, layout, dtype, kind, widths=widths, device="cuda")


@pytest.mark.parametrize("kind", ["rpn2", "mask"])
def test_module_exact_operands_bit_for_bit(hip, route, kind):
    check_exact(kind, hip, device="cuda")


@pytest.mark.parametrize("kind", ["rpn2", "mask"])
def test_module_repeats_its_bits(hip, kind):
    from clipself_amd import conv
    assert conv.thin_wgrad_direct(hip) == conv.THIN_WGRAD_DEFAULT
    twin, xs, gs, _, _ = exact_case(kind)
    m = copy_state(make_module(kind, hip), twin).cuda()
    first = run_module(m, xs, gs, device="cuda")
    again = run_module(m, xs, gs, device="cuda")
    for a, b in zip(first[0] + first[1] + list(first[2].values()), again[0] + again[1] + list(again[2].values())):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ LinearThin and the box head
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("inf", [512, 1024])
def test_linear_thin_against_float64_autograd(hip, route, inf, dtype, kind):
    check_linear(hip, (300, inf, 4), kind, dtype, device="cuda")


def test_linear_thin_3d_input(hip):
    check_linear(hip, (300, 512, 4), "exact", F32, device="cuda", view=(2, 150, 512))
    check_linear(hip, (300, 512, 4), "random", BF, device="cuda", view=(2, 150, 512))


def test_head_with_fused_reg_beside_its_torch_twin(hip):
    """ConvFCBBoxHead(fused=True, fused_reg=True) beside fused_reg=False on 6 RoIs: bbox_pred inside 2 * (K + 2) * 2^-24 * sum|terms| of
    the float64 product of the bf16-rounded operands fc_reg saw, its parameter gradients inside the weight-gradient bound."""
    from clipself_amd.bbox_head import ConvFCBBoxHead
    cfg = dict(num_shared_convs=1, in_channels=64, fc_out_channels=64, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1, num_classes=5,
               reg_class_agnostic=True, norm_cfg=dict(type="SyncBN"))
    torch.manual_seed(7)
    head = ConvFCBBoxHead(ops=hip, fused=True, fused_reg=True, **cfg).cuda()
    twin = ConvFCBBoxHead(ops=hip, fused=True, fused_reg=False, **cfg).cuda()
    twin.load_state_dict(head.state_dict(), strict=True)
    with torch.no_grad():
        head.fc_reg.weight.mul_(100)                                         # std 0.001 -> 0.1: the gradients carry more than rounding noise
        twin.fc_reg.weight.copy_(head.fc_reg.weight)
    x = torch.randn(6, 64, 7, 7, generator=torch.Generator().manual_seed(8)).cuda()
    seen = {}
    head.fc_reg.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach().clone(), y=o.detach().clone()))
    g = torch.randn(6, 4, generator=torch.Generator().manual_seed(9)).cuda()
    preds = {}
    for h, tag in ((head, "k"), (twin, "t")):
        _, pred = h(x.clone())
        pred.backward(g)
        preds[tag] = pred.detach()
    assert preds["k"].dtype == F32 and "LinearThin" in type(head.fc_reg(seen["x"]).grad_fn).__name__
    xr, w, b = seen["x"].float().cpu().to(BF).double(), head.fc_reg.weight.detach().cpu().to(BF).double(), head.fc_reg.bias.detach().cpu().double()
    K = xr.shape[1]
    want = xr @ w.T + b
    bound = 2.0 * (K + 2) * U * (xr.abs() @ w.abs().T + b.abs())
    assert bool(((seen["y"].cpu().double() - want).abs() <= bound).all())
    assert float((preds["k"] - preds["t"]).abs().max()) <= 2.0 ** -7 * float(preds["t"].abs().max())          # the twin reads unrounded operands
    gb = g.cpu().to(BF).double()
    M = 6
    for got, ref64, mag in ((head.fc_reg.weight.grad, gb.T @ xr, gb.abs().T @ xr.abs()), (head.fc_reg.bias.grad, gb.sum(0), gb.abs().sum(0))):
        assert bool(((got.cpu().double() - ref64).abs() <= 2.0 * (M + 2) * U * mag).all())
    assert twin.fc_reg.weight.grad is not None
