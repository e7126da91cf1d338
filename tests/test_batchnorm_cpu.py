"""Batch norm (+ ReLU) on channel-last maps without a GPU (clipself_amd/norm_act.py on tests/_bn_ref.RefOpsBN).

The six ops written from include/clipself_bn.h, chained as the layer chains them, stay inside the derived bounds of tests/_bn_ref.py
against F.batch_norm (+ F.relu) under autograd in float64; seven planted errors do not.  Then the layer itself: its autograd function on
the host backend, state dicts to and from nn.BatchNorm2d and nn.SyncBatchNorm, ConvModule's keys, evaluation mode, affine=False,
track_running_stats=False, ranks stood in for without processes, the fall-backs and the fused=True refusals."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _bn_ref import (BF, EPS, EXACT_IDS, EXACT_PARTS, EXACT_SHAPES, F32, MOMENTUM, SHAPE_IDS, SHAPES, RefOpsBN, all_bits, case, check_exact,
                     check_ops, flawed, make_parts_bn, offset_operands, random_operands, reference, run_exact, run_ops)
from _neck_ref import check_bound
from clipself_amd import det_layer, norm_act
from clipself_amd.norm_act import BatchNormAct2d, ConvModule

UNBALANCED = (1, 37, 90)                    # three parts of 128 rows
GEOM = {(30, 16): (2, 3, 5), (147, 48): (3, 7, 7), (64, 8): (1, 8, 8)}      # (M, C) -> (N, H, W)


def to_map(rows, geom):
    N, H, W = geom
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------ the ops against the reference
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES[:7], ids=SHAPE_IDS[:7])
def test_ops_from_the_header_stay_inside_the_bounds(shape, dtype, act):
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, act)
    check_ops(f"{shape} {dtype} act{act}", run_ops(RefOpsBN(), x, gamma, beta, dy, act, dtype, running=running), ref, tol, shape[1])


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_three_unbalanced_parts_against_the_concatenation(dtype, act):
    x, gamma, beta, dy, running, ref, tol = case((128, 16), dtype, act, splits=UNBALANCED)
    got = run_ops(RefOpsBN(), x, gamma, beta, dy, act, dtype, splits=UNBALANCED, running=running)
    check_ops(f"parts {dtype} act{act}", got, ref, tol, 16)
    assert [int(r[32:33].view(torch.int32)[0]) for r in got["rec"]] == list(UNBALANCED)        # the counts, as integer bits


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=EXACT_IDS)
def test_known_answers_bit_for_bit(shape, dtype, act):
    """The closed form the GPU tests hold the kernels to, on the ops written from the header: the answers themselves are right."""
    check_exact(run_exact(RefOpsBN(), *shape, act, dtype), *shape, act, dtype)
    if shape[0] == sum(EXACT_PARTS):
        one = run_exact(RefOpsBN(), *shape, act, dtype, balanced=EXACT_PARTS)
        three = run_exact(RefOpsBN(), *shape, act, dtype, splits=EXACT_PARTS)
        check_exact(one, *shape, act, dtype, balanced=EXACT_PARTS)
        check_exact(three, *shape, act, dtype, splits=EXACT_PARTS)
        assert torch.equal(all_bits(one)[0], all_bits(three)[0])                               # the state: three parts == one part


def test_evaluation_mode_ops():
    x, gamma, beta, dy = random_operands(147, 48, F32, 5)
    running = (torch.randn(48), torch.rand(48) + 0.5)
    ref, tol = reference(x, gamma, beta, dy, 1, training=False, running=running)
    got = run_ops(RefOpsBN(), x, gamma, beta, dy, 1, F32, running=running, training=False)
    check_ops("eval", got, ref, tol, 48, training=False)
    assert torch.equal(got["running_mean"], running[0]) and torch.equal(got["running_var"], running[1])
    assert float(got["st"][4 * 48]) == 0.0                                                      # 1 / N == 0 marks the evaluation state


# ------------------------------------------------------------------------------------------------ planted errors
def _variance_check(ops):
    M, C = 4096, 8
    x = offset_operands(M, C)
    ref, tol = reference(x, None, None, torch.zeros(M, C), 0)
    rec = torch.full((2 * C + 4,), float("nan"))
    ops.bn_stats(x, rec)
    assert float((tol["M2"] / ref["M2"]).max()) < 0.1                   # the bound itself keeps the variance (first row within a few sigma)
    check_bound("offset M2", rec[C:2 * C], ref["M2"], tol["M2"])
    check_bound("offset mean", rec[:C], ref["mean"], tol["mean"])


def _step_check(shape, act, splits=None):
    def check(ops):
        x, gamma, beta, dy, running, ref, tol = case(shape, F32, act, splits=splits)
        check_ops("planted", run_ops(ops, x, gamma, beta, dy, act, F32, splits=splits, running=running), ref, tol, shape[1])
    return check


PLANTED = {
    "naive_var": _variance_check,                                       # 1. E[x^2] - E[x]^2 in np.float32 on the offset case
    "unbiased_norm": _step_check((30, 16), 0),                          # 2. unbiased variance used for normalisation
    "biased_running": _step_check((30, 16), 0),                         # 3. running_var updated with the biased variance
    "mean_of_means": _step_check((128, 16), 0, UNBALANCED),             # 4. parts merged by averaging their means without counts
    "no_mask": _step_check((147, 48), 1),                               # 5. the ReLU mask ignored in the backward
    "no_xhat_term": _step_check((147, 48), 1),                          # 6. the xhat * sum g xhat / N term dropped from dx
}


@pytest.mark.parametrize("flaw", sorted(PLANTED))
def test_checks_reject_the_planted_error(flaw):
    PLANTED[flaw](RefOpsBN())                                           # the ops as the header states them pass ...
    with pytest.raises(AssertionError):
        PLANTED[flaw](flawed(flaw))                                     # ... the copy with one error does not


def _parts_step(rank, act="relu", dtype=F32):
    """Rank `rank` of three unbalanced ranks through PartsBN under autograd -> (y, dx, dgamma, dbeta, module, ref, tol)."""
    C = 16
    x, gamma, beta, dy, running, ref, tol = case((128, C), dtype, 1 if act else 0, splits=UNBALANCED)
    m = make_parts_bn()(C, act=act, ops=RefOpsBN(), fused=True)
    with torch.no_grad():
        m.weight.copy_(gamma), m.bias.copy_(beta), m.running_mean.copy_(running[0]), m.running_var.copy_(running[1])
    xs = [x[p].to(dtype) for p in ref["parts"]]
    dys = [dy[p].to(dtype) for p in ref["parts"]]
    m.set_parts(xs, dys, rank)
    inp = xs[rank].view(-1, C, 1, 1).clone().requires_grad_(True)
    y = m(inp)
    y.backward(dys[rank].view(-1, C, 1, 1))
    return y.detach(), inp.grad, m.weight.grad, m.bias.grad, m, ref, tol


def _check_rank(rank, out):
    y, dx, dgamma, dbeta, m, ref, tol = out
    p = ref["parts"][rank]
    check_bound("rank y", to_rows(y), ref["y"][p], tol["y"][p])
    check_bound("rank dx", to_rows(dx), ref["dx"][p], tol["dx"][p])
    check_bound("rank dgamma", dgamma, ref["dgamma"][rank], tol["dgamma"][rank])               # this rank's own, as torch's SyncBatchNorm
    check_bound("rank dbeta", dbeta, ref["dbeta"][rank], tol["dbeta"][rank])
    check_bound("rank running_mean", m.running_mean, ref["running_mean"], tol["running_mean"])
    check_bound("rank running_var", m.running_var, ref["running_var"], tol["running_var"])


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_layer_as_one_rank_of_three(rank):
    _check_rank(rank, _parts_step(rank))


def test_checks_reject_parameter_gradients_taken_after_the_cross_part_sum(monkeypatch):
    """7. dgamma / dbeta read after the all-reduce are the totals, not this rank's."""
    real = norm_act._BatchNormActFn

    class Late(real):
        @staticmethod
        def backward(ctx, d_out):
            mod, ops, act = ctx.mod, ctx.ops, ctx.act
            N, H, W, C = ctx.geom
            X, st, gamma = ctx.saved_tensors
            dY = det_layer.channel_last_rows(d_out)
            sums = ops.empty((2 * C,), F32)
            ops.bn_bwd_reduce(dY, X, st, act, sums)
            sums = mod._reduce_sums(sums)
            dX = ops.empty((N * H * W, C), X.dtype)
            ops.bn_bwd_apply(dY, X, st, act, sums, gamma, dX)
            return dX.view(N, H, W, C).permute(0, 3, 1, 2), sums[C:].clone(), sums[:C].clone(), None, None, None

    monkeypatch.setattr(norm_act, "_BatchNormActFn", Late)
    with pytest.raises(AssertionError, match="dgamma|dbeta"):
        _check_rank(1, _parts_step(1))


# ------------------------------------------------------------------------------------------------ the layer
def _layer(C, gamma=None, beta=None, running=None, **kw):
    m = BatchNormAct2d(C, ops=RefOpsBN(), **kw)
    with torch.no_grad():
        if gamma is not None and m.weight is not None:
            m.weight.copy_(gamma), m.bias.copy_(beta)
        if running is not None and m.running_mean is not None:
            m.running_mean.copy_(running[0]), m.running_var.copy_(running[1])
    return m


def _run(m, x4, dy4):
    m.zero_grad()
    inp = x4.detach().clone().requires_grad_(True)
    y = m(inp)
    y.backward(dy4.to(y.dtype))
    return y.detach(), inp.grad, None if m.weight is None else m.weight.grad, None if m.bias is None else m.bias.grad


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("shape", [(30, 16), (147, 48)], ids=["30x16", "147x48"])
def test_layer_under_autograd(shape, act, dtype):
    C, geom = shape[1], GEOM[shape]
    x, gamma, beta, dy, running, ref, tol = case(shape, dtype, 1 if act else 0)
    m = _layer(C, gamma, beta, running, act=act, fused=True)
    x4 = to_map(x.to(dtype), geom).contiguous(memory_format=torch.channels_last)
    y, dx, dgamma, dbeta = _run(m, x4, to_map(dy, geom))
    assert y.dtype == dtype and dx.dtype == dtype and dgamma.dtype == F32 and dbeta.dtype == F32
    assert y.permute(0, 2, 3, 1).is_contiguous() and tuple(y.shape) == tuple(x4.shape)
    assert "BatchNormAct" in type(m(x4).grad_fn).__name__ and int(m.num_batches_tracked) == 2
    check_bound("layer y", to_rows(y), ref["y"], tol["y"])
    check_bound("layer dx", to_rows(dx), ref["dx"], tol["dx"])
    check_bound("layer dgamma", dgamma, ref["dgamma"][0], tol["dgamma"][0])
    check_bound("layer dbeta", dbeta, ref["dbeta"][0], tol["dbeta"][0])
    m2 = _layer(C, gamma, beta, running, act=act, fused=True)
    again = _run(m2, to_map(x.to(dtype), geom).contiguous(), to_map(dy, geom).contiguous())     # NCHW-contiguous: made channel-last once
    assert all(torch.equal(a, b) for a, b in zip((y, dx, dgamma, dbeta), again))
    check_bound("layer running_mean", m2.running_mean, ref["running_mean"], tol["running_mean"])
    check_bound("layer running_var", m2.running_var, ref["running_var"], tol["running_var"])


def test_layer_matches_torch_modules_step_by_step():
    """Two training steps and an evaluation pass beside nn.BatchNorm2d + ReLU in float64: outputs, running statistics, the counter."""
    C, geom = 16, (2, 3, 5)
    m = _layer(C, act="relu", fused=True)
    t = nn.BatchNorm2d(C).double()
    for step in range(3):
        if step == 2:
            m.eval(), t.eval()
        x = torch.randn(2, C, 3, 5, generator=torch.Generator().manual_seed(step)) * 2 + 1
        y, want = m(x), F.relu(t(x.double()))
        assert float((y.detach().double() - want.detach()).abs().max()) < 1e-5
    assert int(m.num_batches_tracked) == 2 == int(t.num_batches_tracked)
    assert float((m.running_mean.double() - t.running_mean).abs().max()) < 1e-6
    assert float((m.running_var.double() - t.running_var).abs().max()) < 1e-6


def test_evaluation_mode_affine_false_and_untracked_statistics():
    shape, geom = (30, 16), (2, 3, 5)
    x, gamma, beta, dy, running, _, _ = case(shape, F32, 1)
    x4, dy4 = to_map(x, geom), to_map(dy, geom)
    # evaluation mode: the running statistics normalise, dx = gamma * rstd * g, nothing is updated
    m = _layer(16, gamma, beta, running, act="relu", fused=True).eval()
    ref, tol = reference(x, gamma, beta, dy, 1, training=False, running=running)
    y, dx, dgamma, dbeta = _run(m, x4, dy4)
    check_bound("eval y", to_rows(y), ref["y"], tol["y"])
    check_bound("eval dx", to_rows(dx), ref["dx"], tol["dx"])
    check_bound("eval dgamma", dgamma, ref["dgamma"][0], tol["dgamma"][0])
    assert torch.equal(m.running_mean, running[0]) and int(m.num_batches_tracked) == 0
    # affine=False: no parameters, scale = rstd
    m = _layer(16, running=running, act="relu", affine=False, fused=True)
    assert m.weight is None and m.bias is None
    ref, tol = reference(x, None, None, dy, 1, running=running)
    y, dx, _, _ = _run(m, x4, dy4)
    check_bound("affine=False y", to_rows(y), ref["y"], tol["y"])
    check_bound("affine=False dx", to_rows(dx), ref["dx"], tol["dx"])
    check_bound("affine=False running_var", m.running_var, ref["running_var"], tol["running_var"])
    # track_running_stats=False: no buffers; batch statistics in training and in evaluation mode
    m = _layer(16, gamma, beta, act="relu", track_running_stats=False, fused=True)
    assert m.running_mean is None and m.num_batches_tracked is None
    ref, tol = reference(x, gamma, beta, dy, 1)
    for mode in (m.train(), m.eval()):
        y, dx, _, _ = _run(mode, x4, dy4)
        check_bound("untracked y", to_rows(y), ref["y"], tol["y"])
        check_bound("untracked dx", to_rows(dx), ref["dx"], tol["dx"])


def test_state_dicts_round_trip_with_torch_layers():
    C = 16
    for other_cls in (nn.BatchNorm2d, nn.SyncBatchNorm):
        other, m = other_cls(C), BatchNormAct2d(C, act="relu")
        with torch.no_grad():
            for t in other.state_dict().values():
                t.copy_(torch.rand_like(t.float()) * 5)
        assert list(m.state_dict()) == list(other.state_dict())
        assert not any(m.load_state_dict(other.state_dict(), strict=True))
        back = other_cls(C)
        assert not any(back.load_state_dict(m.state_dict(), strict=True))
        assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), other.state_dict().values()))
    fresh, torch_fresh = BatchNormAct2d(C), nn.BatchNorm2d(C)
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), torch_fresh.state_dict().values()))        # initialisation
    assert fresh.eps == torch_fresh.eps and fresh.momentum == torch_fresh.momentum


def test_conv_module_keys_and_forward():
    m = ConvModule(64, 16, ops=RefOpsBN(), fused=True)
    assert list(m.state_dict()) == ["conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    ckpt = {"conv.weight": torch.randn(16, 64, 3, 3), "bn.weight": torch.rand(16), "bn.bias": torch.randn(16),
            "bn.running_mean": torch.randn(16), "bn.running_var": torch.rand(16) + 0.5, "bn.num_batches_tracked": torch.tensor(7)}
    assert not any(m.load_state_dict(ckpt, strict=True))
    assert list(ConvModule(64, 16, norm=False).state_dict()) == ["conv.weight", "conv.bias"]      # mmcv's bias='auto'
    x = torch.randn(2, 64, 3, 5).to(BF).to(F32).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn(2, 16, 3, 5)
    y = m(x)
    y.backward(dy)
    assert y.permute(0, 2, 3, 1).is_contiguous() and bool((y >= 0).all()) and int(m.bn.num_batches_tracked) == 8
    # the same stack with torch's norm behind the same convolution: the convolution's bits are equal, the norm is isolated
    t = ConvModule(64, 16, ops=RefOpsBN(), fused=True)
    t.load_state_dict(ckpt)
    t.bn.fused = False
    conv_out = t.conv(x.detach())
    assert torch.equal(conv_out, m.conv(x.detach()))
    ref, tol = reference(to_rows(conv_out.detach()), ckpt["bn.weight"], ckpt["bn.bias"], to_rows(dy), 1)
    check_bound("ConvModule y", to_rows(y), ref["y"], tol["y"])
    check_bound("ConvModule dgamma", m.bn.weight.grad, ref["dgamma"][0], tol["dgamma"][0])
    check_bound("ConvModule dbeta", m.bn.bias.grad, ref["dbeta"][0], tol["dbeta"][0])
    assert float((t(x.detach()) - y).detach().abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ dispatch
def test_fall_backs_and_refusals(monkeypatch):
    x = torch.randn(2, 12, 3, 5)
    want = F.relu(F.batch_norm(x, None, None, torch.ones(12), torch.zeros(12), True, 0.1, 1e-5))
    # outside the coverage: torch, or NotImplementedError under fused=True
    cases = [
        (dict(num_features=12), x),                                                                     # C % 8
        (dict(num_features=16, momentum=None), torch.randn(2, 16, 3, 5)),                               # cumulative averaging
        (dict(num_features=16), torch.randn(2, 16, 3, 5, dtype=torch.float64)),                         # neither fp32 nor bf16
        (dict(num_features=16, dtype=torch.bfloat16), torch.randn(2, 16, 3, 5).to(BF)),                 # non-fp32 parameters
    ]
    for kw, inp in cases:
        dtype = kw.pop("dtype", None)
        soft = BatchNormAct2d(act="relu", ops=RefOpsBN(), fused=None, **kw)
        hard = BatchNormAct2d(act="relu", ops=RefOpsBN(), fused=True, **kw)
        if dtype is not None:
            soft, hard = soft.to(dtype), hard.to(dtype)
        if inp.dtype == torch.float64:
            soft = soft.double()
        monkeypatch.setattr(norm_act, "FUSED_BN_DEFAULT", True)
        out = soft(inp)
        assert "BatchNormAct" not in type(out.grad_fn).__name__ and bool((out >= 0).all())
        with pytest.raises(NotImplementedError):
            hard(inp)
    assert torch.allclose(BatchNormAct2d(12, act="relu", ops=RefOpsBN())(x), want, atol=1e-6)
    # fused=None follows FUSED_BN_DEFAULT; fused=False is torch; fused=True on a host tensor without a host backend is refused
    x16 = torch.randn(2, 16, 3, 5)
    for default in (False, True):
        monkeypatch.setattr(norm_act, "FUSED_BN_DEFAULT", default)
        assert ("BatchNormAct" in type(BatchNormAct2d(16, ops=RefOpsBN())(x16).grad_fn).__name__) is default
        assert "BatchNormAct" not in type(BatchNormAct2d(16, ops=RefOpsBN(), fused=False)(x16).grad_fn).__name__
    with pytest.raises(NotImplementedError):
        BatchNormAct2d(16, fused=True)(x16)
    # one value per channel in training mode raises as torch does
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        BatchNormAct2d(16, ops=RefOpsBN(), fused=True)(torch.randn(1, 16, 1, 1))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        nn.BatchNorm2d(16)(torch.randn(1, 16, 1, 1))
    BatchNormAct2d(16, ops=RefOpsBN(), fused=True).eval()(torch.randn(1, 16, 1, 1))                # evaluation mode: fine


def test_flag_default_is_recorded():
    assert norm_act.FUSED_BN_DEFAULT in (True, False) and EPS == 1e-5 and MOMENTUM == 0.1
