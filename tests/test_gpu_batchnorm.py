"""`-m gpu`: batch norm (+ ReLU) on channel-last maps (include/clipself_bn.h, clipself_amd/norm_act.py) on the MI355X.

Kernels alone (HipOps.bn_*): outputs are handed in as NaN, every step runs twice with equal bits.  Known answers bit for bit (st, y, dx,
sums, running statistics; fp32 and bf16 maps, with and without the ReLU; three balanced parts against one).  Random operands inside the
derived per-element bounds of tests/_bn_ref.py, the worst error / bound printed as `BN PARITY ...` (profiles/batchnorm_parity.md).  The
offset case, ReLU ties, padded row strides, the read / write extents of all six entry points inside the poisoned halos of
tests/_extents.py, the layer under autograd and a ConvModule stack."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _bn_ref import (BF, EXACT_IDS, EXACT_PARTS, EXACT_SHAPES, F32, REC_EXTRA, SHAPE_IDS, SHAPES, ST_EXTRA, U, all_bits, case,  # noqa: E402
                     check_exact, check_ops, flawed, offset_operands, random_operands, reference, run_exact, run_ops, same_bits)
from _extents import run_case  # noqa: E402
from _neck_ref import check_bound  # noqa: E402
from clipself_amd.norm_act import BatchNormAct2d, ConvModule  # noqa: E402

UNBALANCED = (1, 37, 90)
DT = {F32: "fp32", BF: "bf16"}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _nan(shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(all_bits(a), all_bits(b))), "two runs on equal inputs differ"
    return a


def to_map(rows, geom):
    N, H, W = geom
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------ kernels alone: known answers
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=EXACT_IDS)
def test_known_answers_bit_for_bit(hip, shape, dtype, act):
    assert hip.BATCHNORM
    check_exact(_twice(lambda: run_exact(hip, *shape, act, dtype, dev="cuda")), *shape, act, dtype)
    if shape[0] == sum(EXACT_PARTS):
        one = _twice(lambda: run_exact(hip, *shape, act, dtype, dev="cuda", balanced=EXACT_PARTS))
        three = _twice(lambda: run_exact(hip, *shape, act, dtype, dev="cuda", splits=EXACT_PARTS))
        check_exact(one, *shape, act, dtype, balanced=EXACT_PARTS)
        check_exact(three, *shape, act, dtype, splits=EXACT_PARTS)
        assert torch.equal(all_bits(one)[0], all_bits(three)[0]), "csb_finalize(R = 3) differs from the one-part state"
        cat = lambda ts: torch.cat([t.detach().cpu().float() for t in ts])
        assert torch.equal(cat(one["y"]), cat(three["y"])) and torch.equal(cat(one["dx"]), cat(three["dx"]))


# ------------------------------------------------------------------------------------------------ kernels alone: random operands
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_random_operands_within_the_derived_bounds(hip, shape, dtype, act):
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, act)
    got = _twice(lambda: run_ops(hip, x, gamma, beta, dy, act, dtype, running=running, dev="cuda"))
    check_ops(f"BN PARITY {shape[0]}x{shape[1]} {DT[dtype]} act{act}", got, ref, tol, shape[1])


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [16, 72])
def test_three_unbalanced_parts_against_the_concatenation(hip, C, dtype, act):
    x, gamma, beta, dy, running, ref, tol = case((128, C), dtype, act, splits=UNBALANCED)
    got = _twice(lambda: run_ops(hip, x, gamma, beta, dy, act, dtype, splits=UNBALANCED, running=running, dev="cuda"))
    check_ops(f"BN PARITY 1+37+90x{C} {DT[dtype]} act{act}", got, ref, tol, C)
    assert [int(r[2 * C:2 * C + 1].view(torch.int32)[0]) for r in got["rec"]] == list(UNBALANCED)


def test_offset_case_keeps_its_variance(hip):
    """Channel means 1000 and 10 000, unit variance, fp32: M2 inside the bound derived for the shifted sums -- one that E[x^2] - E[x]^2 in
    np.float32 misses (tests/test_batchnorm_cpu.py shows that on the same operands)."""
    for M, C in ((4096, 8), (5000, 768)):
        x = offset_operands(M, C)
        ref, tol = reference(x, None, None, torch.zeros(M, C), 0)
        naive = torch.empty(2 * C + REC_EXTRA)
        flawed("naive_var").bn_stats(x, naive)                          # E[x^2] - E[x]^2 in np.float32, on the host
        with pytest.raises(AssertionError):
            check_bound(f"naive formula {M}x{C} M2", naive[C:2 * C], ref["M2"], tol["M2"])

        def stats():
            rec = _nan((2 * C + REC_EXTRA,))
            hip.bn_stats(x.cuda(), rec)
            return dict(st=rec, running_mean=None, running_var=None, rec=[], y=[], sums=[], dx=[])
        rec = _twice(stats)["st"]
        check_bound(f"BN PARITY offset {M}x{C} M2", rec[C:2 * C], ref["M2"], tol["M2"])
        check_bound(f"BN PARITY offset {M}x{C} mean", rec[:C], ref["mean"], tol["mean"])


def test_evaluation_mode(hip):
    x, gamma, beta, dy = random_operands(147, 48, F32, 5)
    g = torch.Generator().manual_seed(1)
    running = (torch.randn(48, generator=g), torch.rand(48, generator=g) + 0.5)
    for dtype in (F32, BF):
        xd, dyd = x.to(dtype).to(F32), dy.to(dtype).to(F32)
        ref, tol = reference(xd, gamma, beta, dyd, 1, training=False, running=running, bf16_out=dtype == BF)
        got = _twice(lambda: run_ops(hip, xd, gamma, beta, dyd, 1, dtype, running=running, training=False, dev="cuda"))
        check_ops(f"eval {DT[dtype]}", got, ref, tol, 48, training=False)
        assert torch.equal(got["running_mean"].cpu(), running[0]) and torch.equal(got["running_var"].cpu(), running[1])
        assert float(got["st"][4 * 48]) == 0.0


# ------------------------------------------------------------------------------------------------ ReLU ties
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_relu_ties_and_a_masked_channel(hip, dtype):
    """fmaf(x, scale, shift) exactly +0 (channel 0: 1 * 2 - 2) and -0 (channel 1: -0 * 1 - 0) give y = 0 and g = 0; channel 2 is masked
    everywhere (x * 1 - 8 < 0): dx = 0, dgamma = dbeta = 0.  The state is written by hand: mean 0, rstd 1, 1 / N = 1 / M."""
    M, C = 64, 8
    x = torch.randint(1, 4, (M, C)).float()
    x[:, 0], x[:, 1] = 1.0, -0.0
    scale, shift = torch.ones(C), torch.zeros(C)
    scale[0], shift[0], shift[1], shift[2] = 2.0, -2.0, -0.0, -8.0
    st = torch.cat([torch.zeros(C), torch.ones(C), scale, shift, torch.tensor([1.0 / M, 0, 0, 0])]).cuda()
    dy = torch.randint(1, 5, (M, C)).float()
    X, dY = x.to(dtype).cuda(), dy.to(dtype).cuda()
    y, sums, dx = _nan((M, C), dtype), _nan((2 * C,)), _nan((M, C), dtype)
    hip.bn_apply(X, st, 1, y)
    hip.bn_bwd_reduce(dY, X, st, 1, sums)
    hip.bn_bwd_apply(dY, X, st, 1, sums, None, dx)
    y, sums, dx = y.cpu().float(), sums.cpu(), dx.cpu().float()
    assert bool((y[:, :3] == 0).all()) and not bool(torch.signbit(y[:, :3]).any())
    assert bool((sums[:3] == 0).all()) and bool((sums[C:C + 3] == 0).all())                     # dbeta, dgamma of the three channels
    assert bool((dx[:, :3] == 0).all())
    assert torch.equal(y[:, 3:], x[:, 3:]) and torch.equal(sums[3:C], dy[:, 3:].sum(0))          # the other channels pass: x >= 1
    assert torch.equal(sums[C + 3:], (dy * x)[:, 3:].sum(0))


# ------------------------------------------------------------------------------------------------ row strides, extents, refusals
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(30, 16), (257, 64), (1089, 72)], ids=["30x16", "257x64", "1089x72"])
def test_padded_row_strides(hip, shape, dtype):
    """ld > C: the padding of x and dy holds NaN (never read), the padding of y and dx keeps its fill (never written)."""
    M, C = shape
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, 1)
    want = run_ops(hip, x, gamma, beta, dy, 1, dtype, running=running, dev="cuda")
    Xp, dYp = _nan((M, C + 24), dtype), _nan((M, C + 8), dtype)
    Xp[:, :C], dYp[:, :C] = x.to(dtype).cuda(), dy.to(dtype).cuda()
    Y, dX = (torch.full((M, C + 16), 7.0, dtype=dtype, device="cuda") for _ in range(2))
    Y[:, :C], dX[:, :C] = float("nan"), float("nan")
    rec, st, sums = _nan((2 * C + REC_EXTRA,)), _nan((4 * C + ST_EXTRA,)), _nan((2 * C,))
    hip.bn_stats(Xp[:, :C], rec)
    hip.bn_finalize(rec, C, gamma.cuda(), beta.cuda(), 1e-5, 0.1, None, None, st)
    hip.bn_apply(Xp[:, :C], st, 1, Y[:, :C])
    hip.bn_bwd_reduce(dYp[:, :C], Xp[:, :C], st, 1, sums)
    hip.bn_bwd_apply(dYp[:, :C], Xp[:, :C], st, 1, sums, gamma.cuda(), dX[:, :C])
    same_bits(st, want["st"].cpu(), "st")
    same_bits(Y[:, :C].contiguous(), want["y"][0].cpu(), "y")
    same_bits(sums, want["sums"][0].cpu(), "sums")
    same_bits(dX[:, :C].contiguous(), want["dx"][0].cpu(), "dx")
    assert bool((Y[:, C:] == 7.0).all()) and bool((dX[:, C:] == 7.0).all()), "a kernel wrote into the row padding"


def _extent_case(shape, what, dtype):
    M, C = shape
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, 1)
    mult = 8 if dtype == BF else 4
    st_ref = torch.cat([ref[k].float() for k in ("mean", "rstd", "scale", "shift")] + [torch.tensor([1.0 / M, 0, 0, 0])])

    def fn(ops, a):
        X = a.inp(x.to(dtype), a.ld(C, mult))
        if what == "stats":
            rec = a.out((2 * C + REC_EXTRA,), F32)
            ops.bn_stats(X, rec, a.ws(ops.bn_workspace(M, C)))
            return {"rec": rec}
        if what == "finalize":
            recs = a.inp(torch.cat([ref["mean"].float(), ref["M2"].float(), torch.tensor([M, 0, 0, 0], dtype=torch.int32).view(F32)]).repeat(2))
            rm, rv = a.out((C,), F32, init=running[0]), a.out((C,), F32, init=running[1])
            st = a.out((4 * C + ST_EXTRA,), F32)
            ops.bn_finalize(recs.view(2, -1), C, a.inp(gamma), a.inp(beta), 1e-5, 0.1, rm, rv, st)
            return {"st": st, "running_mean": rm, "running_var": rv}
        st = a.inp(st_ref)
        if what == "apply":
            Y = a.out((M, C), dtype, a.ld(C, mult))
            ops.bn_apply(X, st, 1, Y)
            return {"y": Y}
        dY = a.inp(dy.to(dtype), a.ld(C, mult))
        sums = a.out((2 * C,), F32)
        ops.bn_bwd_reduce(dY, X, st, 1, sums, a.ws(ops.bn_workspace(M, C)))
        if what == "bwd_reduce":
            return {"sums": sums}
        dX = a.out((M, C), dtype, a.ld(C, mult))
        ops.bn_bwd_apply(dY, X, st, 1, sums, a.inp(gamma), dX)
        return {"dx": dX}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("shape", [(30, 16), (147, 48), (1089, 72), (5000, 768)], ids=["30x16", "147x48", "1089x72", "5000x768"])
def test_kernels_stay_inside_their_extents(hip, shape, pad):
    for dtype in (F32, BF):
        for what in ("stats", "finalize", "apply", "bwd_reduce", "bwd_apply"):
            key = f"batchnorm.{what}[{shape},{dtype}]"
            problems = run_case(hip, _extent_case(shape, what, dtype), "cuda", pad, key=key)
            assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_workspace_and_refusals(hip):
    lib, p = hip.lib, (lambda t: t.data_ptr())
    assert hip.bn_workspace(5000, 768) == lib.csb_row_parts(5000, 768) * 2 * 768 * 4 and lib.csb_row_parts(5000, 768) > 1
    assert hip.bn_workspace(2, 8) == 2 * 8 * 4 and hip.bn_workspace(5, 12) == 0 and hip.bn_workspace(1 << 31, 8) == 0
    X, Y = torch.zeros(30, 16, device="cuda"), torch.zeros(30, 16, device="cuda")
    rec, st, ws = torch.zeros(36, device="cuda"), torch.zeros(68, device="cuda"), torch.zeros(4096, device="cuda")
    assert lib.csb_stats(p(X), 16, 0, 30, 12, p(rec), p(ws), None) == 1                                # C % 8: outside the coverage
    assert lib.csb_apply(p(X), 16, 0, p(st), 1, p(Y), 16, 0, 30, 12, None) == 1
    assert lib.csb_stats(p(X), 14, 0, 30, 16, p(rec), p(ws), None) == -1 and b"stride" in lib.cs_last_error()
    assert lib.csb_stats(p(X), 20, 1, 30, 16, p(rec), p(ws), None) == -1                               # bf16 wants ld % 8
    assert lib.csb_stats(p(X) + 4, 16, 0, 30, 16, p(rec), p(ws), None) == -1                           # alignment
    assert lib.csb_stats(p(X), 16, 0, 0, 16, p(rec), p(ws), None) == -1                                # M = 0
    assert lib.csb_stats(p(X), 16, 0, 1 << 31, 16, p(rec), p(ws), None) == -1                          # past CSB_MAX_ROWS
    assert lib.csb_apply(p(X), 16, 0, p(st), 2, p(Y), 16, 0, 30, 16, None) == -1                       # act
    assert lib.csb_finalize(None, 0, 16, None, None, 1e-5, 0.1, None, None, p(st), None) == -1         # evaluation without running statistics
    assert lib.csb_finalize(p(rec), 0, 16, None, None, 1e-5, 0.1, None, None, p(st), None) == -1       # R = 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.bn_stats(X[:, :12], rec)
    with pytest.raises(ValueError):
        hip.bn_stats(X.double(), rec)
    with pytest.raises(ValueError):
        hip.bn_apply(X, st, 1, Y[:29])
    with pytest.raises(ValueError):
        hip.bn_apply(X, st, 3, Y)
    with pytest.raises(ValueError):
        hip.bn_stats(X, rec, ws=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        hip.bn_finalize(None, 16, None, None, 1e-5, 0.1, None, None, st)


# ------------------------------------------------------------------------------------------------ the layer
def _layer(ops, C, gamma, beta, running, **kw):
    m = BatchNormAct2d(C, ops=ops, **kw)
    with torch.no_grad():
        m.weight.copy_(gamma), m.bias.copy_(beta), m.running_mean.copy_(running[0]), m.running_var.copy_(running[1])
    return m.cuda()


def _run(m, x4, dy4):
    m.zero_grad()
    inp = x4.detach().clone().requires_grad_(True)
    y = m(inp)
    y.backward(dy4.to(y.dtype))
    return y.detach(), inp.grad, m.weight.grad, m.bias.grad


@pytest.mark.parametrize("form", ["channel_last_fp32", "channel_last_bf16", "nchw_fp32"])
def test_layer_under_autograd(hip, form):
    """fused=True over two training steps, then evaluation mode; the second step against the reference on the first step's statistics."""
    shape, geom = (147, 48), (3, 7, 7)
    dtype = BF if form.endswith("bf16") else F32
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, 1)
    m = _layer(hip, 48, gamma, beta, running, act="relu", fused=True)
    fmt = torch.contiguous_format if form.startswith("nchw") else torch.channels_last
    x4, dy4 = (to_map(t.to(dtype), geom).contiguous(memory_format=fmt).cuda() for t in (x, dy))
    y, dx, dgamma, dbeta = _run(m, x4, dy4)
    assert y.dtype == dtype and dx.dtype == dtype and dgamma.dtype == F32 and y.permute(0, 2, 3, 1).is_contiguous()
    for k, got in (("y", to_rows(y)), ("dx", to_rows(dx)), ("dgamma", dgamma), ("dbeta", dbeta)):
        check_bound(f"layer {form} {k}", got, ref[k][0] if k in ("dgamma", "dbeta") else ref[k], tol[k][0] if k in ("dgamma", "dbeta") else tol[k])
    check_bound(f"layer {form} running_var", m.running_var, ref["running_var"], tol["running_var"])
    x2, _, _, dy2 = random_operands(*shape, dtype, 11)
    step1 = (m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone())
    ref2, tol2 = reference(x2, gamma, beta, dy2, 1, running=step1, bf16_out=dtype == BF)
    y2, dx2, _, _ = _run(m, to_map(x2.to(dtype), geom).contiguous(memory_format=fmt).cuda(), to_map(dy2.to(dtype), geom).cuda())
    check_bound(f"layer {form} step 2 y", to_rows(y2), ref2["y"], tol2["y"])
    check_bound(f"layer {form} step 2 running_mean", m.running_mean, ref2["running_mean"], tol2["running_mean"])
    assert int(m.num_batches_tracked) == 2
    m.eval()
    step2 = (m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone())
    ref3, tol3 = reference(x, gamma, beta, dy, 1, training=False, running=step2, bf16_out=dtype == BF)
    y3, dx3, _, _ = _run(m, x4, dy4)
    check_bound(f"layer {form} eval y", to_rows(y3), ref3["y"], tol3["y"])
    check_bound(f"layer {form} eval dx", to_rows(dx3), ref3["dx"], tol3["dx"])
    assert int(m.num_batches_tracked) == 2 and torch.equal(m.running_mean.cpu(), step2[0])


def test_layer_on_the_default_backend_and_refusals(hip):
    shape, geom = (30, 16), (2, 3, 5)
    x, gamma, beta, dy, running, ref, tol = case(shape, F32, 1)
    m = _layer(None, 16, gamma, beta, running, act="relu", fused=True)                          # the process-wide HipOps of det_backend
    y, dx, dgamma, dbeta = _run(m, to_map(x, geom).cuda(), to_map(dy, geom).cuda())
    assert "BatchNormAct" in type(m(to_map(x, geom).cuda()).grad_fn).__name__
    check_bound("default backend y", to_rows(y), ref["y"], tol["y"])
    check_bound("default backend dx", to_rows(dx), ref["dx"], tol["dx"])
    with pytest.raises(NotImplementedError):
        BatchNormAct2d(12, ops=hip, fused=True).cuda()(torch.randn(2, 12, 3, 5, device="cuda"))  # C % 8
    with pytest.raises(NotImplementedError):
        m(to_map(x, geom))                                                                      # a CPU tensor
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.train()(torch.randn(1, 16, 1, 1, device="cuda"))
    soft = BatchNormAct2d(12, act="relu", ops=hip).cuda()                                       # outside the coverage: torch
    z = torch.randn(2, 12, 3, 5, device="cuda")
    assert torch.allclose(soft(z), F.relu(F.batch_norm(z, None, None, soft.weight, soft.bias, True, 0.1, 1e-5)), atol=1e-6)


def test_conv_module_stack(hip):
    """Two ConvModule(64, 64) on (N, H, W) = (6, 7, 7) beside the same stack with the norms' fused=False.  The first convolution sees the
    same input in both, so its bits are equal; behind it every norm is isolated: its y, dx, dgamma, dbeta against the float64 reference
    on the convolution output and the output gradient that reached it, inside the norm's bounds.  (The second convolution rounds its
    input to bf16, so the two stacks' second maps may differ by a bf16 ulp where the norms differ by 1e-7: comparing whole stacks would
    test that rounding, not the norm.)"""
    torch.manual_seed(3)
    stack = torch.nn.Sequential(ConvModule(64, 64, ops=hip, fused=True), ConvModule(64, 64, ops=hip, fused=True)).cuda()
    twin = torch.nn.Sequential(ConvModule(64, 64, ops=hip, fused=True), ConvModule(64, 64, ops=hip, fused=True)).cuda()
    twin.load_state_dict(stack.state_dict())
    for m in twin:
        m.bn.fused = False
    x = torch.randn(6, 64, 7, 7, device="cuda").contiguous(memory_format=torch.channels_last)
    dy = torch.randn(6, 64, 7, 7, device="cuda").contiguous(memory_format=torch.channels_last)
    assert torch.equal(stack[0].conv(x), twin[0].conv(x))
    seen = {}

    def hook(name):
        def fwd(mod, inp, out):
            inp[0].retain_grad() if inp[0].requires_grad else None
            out.retain_grad()
            seen[name] = (inp[0], out)
        return fwd
    handles = [stack[i].bn.register_forward_hook(hook(i)) for i in range(2)]
    inp = x.clone().requires_grad_(True)
    out = stack(inp)
    out.backward(dy)
    want = twin(x)
    assert out.permute(0, 2, 3, 1).is_contiguous() and tuple(want.shape) == tuple(out.shape)
    for i in range(2):
        cin, cout = seen[i]
        bn = stack[i].bn
        ref, tol = reference(to_rows(cin.detach()).cpu(), torch.ones(64), torch.zeros(64), to_rows(cout.grad).cpu(), 1)
        check_bound(f"stack norm {i} y", to_rows(cout.detach()), ref["y"], tol["y"])
        check_bound(f"stack norm {i} dx", to_rows(cin.grad), ref["dx"], tol["dx"])
        check_bound(f"stack norm {i} dgamma", bn.weight.grad, ref["dgamma"][0], tol["dgamma"][0])
        check_bound(f"stack norm {i} dbeta", bn.bias.grad, ref["dbeta"][0], tol["dbeta"][0])
        assert stack[i].conv.weight.grad is not None and bool(torch.isfinite(stack[i].conv.weight.grad).all())
        assert int(bn.num_batches_tracked) == 1
    assert inp.grad is not None and inp.grad.permute(0, 2, 3, 1).is_contiguous()
    for h in handles:
        h.remove()
