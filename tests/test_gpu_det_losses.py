"""`-m gpu`: the detector's losses on the MI355X (csl_rpn_loss / csl_bbox_head_loss, HipOps.rpn_loss / bbox_head_loss).

Every case of tests/_loss_ref.RPN_CASES / HEAD_CASES through the kernels against the closed-form float64 restatement, element by element
inside the bounds its docstring derives, for losses and gradients; acc and the avg used bit for bit.  Cases on dyadic inputs (the L1
parts; uniform logits with a power-of-two avg_factor for the gradients) are bit-equal to the restatement.  Shapes sit around this
layout's boundaries (det_loss.hip): groups of four cells (h * w = 35, 1, 4), 16-byte stores only where the address allows (a
misaligned gradient tensor), one and several workgroups per segment, 64 lanes x 1, 2, 4, ..., 64 classes per lane (C1 = 64 | 65, 1204,
4096), four rows per workgroup (R = 63, 64, 65, 513), ldc > C1.  Outputs are handed in poisoned, so an element the kernels leave
unwritten fails the comparison; every call is made twice and must return equal bits.  The worst fraction of each bound is printed when
the module is done (pytest -s; profiles/det_losses_parity.md)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_ref as R  # noqa: E402

WORST = {}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    yield HipOps()
    for k in sorted(WORST):
        print(f"\nworst fraction of the bound: {k}: {WORST[k]:.4f}", end="")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(shape, misalign=False):
    """A NaN-filled fp32 tensor; misalign: its first element sits 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    flat = torch.full((n + 4,), float("nan"), dtype=torch.float32, device="cuda")
    t = flat[1:n + 1] if misalign else flat[:n]
    assert (t.data_ptr() % 16 == 4) if misalign else (t.data_ptr() % 16 == 0)
    return t.view(shape)


def _np(t):
    return t.cpu().numpy()


def _note(prefix, worst):
    for k, v in worst.items():
        WORST[prefix + k] = max(WORST.get(prefix + k, 0.0), v)


def rpn_kernel(hip, c, grad=True, misalign=False):
    cls, reg = [_dev(v) for v in c["cls"]], [_dev(v) for v in c["reg"]]
    args = (cls, reg, _dev(c["labels"]), _dev(c["lw"]), _dev(c["bt"]), _dev(c["bw"]), torch.tensor([c["avg"]], dtype=torch.float32, device="cuda"))
    runs = []
    for _ in range(2):
        out = (_nan((len(cls), 2)), [_nan(v.shape, misalign) for v in cls] if grad else None, [_nan(v.shape, misalign) for v in reg] if grad else None)
        losses, dcls, dreg = hip.rpn_loss(*args, grad=grad, out=out)
        runs.append((_np(losses), [_np(g) for g in dcls] if grad else None, [_np(g) for g in dreg] if grad else None))
    for l in range(len(cls)):                                  # the predictions are only read
        assert np.array_equal(_np(cls[l]), c["cls"][l], equal_nan=True) and np.array_equal(_np(reg[l]), c["reg"][l], equal_nan=True)
    a, b = runs
    assert R.same_float_bits(a[0], b[0]), "two calls, different losses"
    if grad:
        for l in range(len(cls)):
            assert R.same_float_bits(a[1][l], b[1][l]) and R.same_float_bits(a[2][l], b[2][l]), ("two calls, different gradients", l)
    return a


def head_kernel(hip, c, grad=True):
    R_, C1, pad = c["R"], c["C1"], c["pad"]
    xfull = _dev(c["x"])
    x = xfull[:, :C1]
    avg = None if c["avg"] is None else torch.tensor([c["avg"]], dtype=torch.float32, device="cuda")
    args = (x, _dev(c["labels"]), _dev(c["lw"]), _dev(c["bp"]), _dev(c["bt"]), _dev(c["bw"]), c["bg"], _dev(c["cw"]), avg)
    runs = []
    for _ in range(2):
        dfull = _nan((R_, C1 + pad))
        out = (_nan((4,)), dfull[:, :C1] if grad else None, _nan((R_, 4)) if grad else None)
        o4, dcls, dbbox = hip.bbox_head_loss(*args, grad=grad, out=out)
        if grad and pad:
            assert bool(torch.isnan(dfull[:, C1:]).all()), "the padding columns of dcls were written"
        runs.append((_np(o4), _np(dcls) if grad else None, _np(dbbox) if grad else None))
    assert np.array_equal(_np(xfull), c["x"], equal_nan=True), "the caller's logits were written"
    a, b = runs
    assert R.same_float_bits(a[0], b[0]), "two calls, different outputs"
    if grad:
        assert R.same_float_bits(a[1], b[1]) and R.same_float_bits(a[2], b[2]), "two calls, different gradients"
    return a


def check_rpn(got, want):
    losses, dcls, dreg = got
    worst = {}
    for k, i in (("loss_cls", 0), ("loss_bbox", 1)):
        ok, worst[k] = R.inside(losses[:, i], want["losses"][:, i], want["losses_bound"][:, i])
        print(k, losses[:, i], want["losses"][:, i], want["losses_bound"][:, i])
        assert ok, k
    worst["dcls"] = worst["dreg"] = 0.0
    for l in range(len(dcls)):
        ok, f = R.inside(dcls[l], want["dcls"][l], want["dcls_bound"][l])
        print("dcls level", l, "fraction of the bound", f)
        assert ok, ("dcls", l)
        worst["dcls"] = max(worst["dcls"], f)
        ok, f = R.inside(dreg[l], want["dreg"][l], want["dreg_bound"][l])
        print("dreg level", l, "fraction of the bound", f)
        assert ok, ("dreg", l)
        worst["dreg"] = max(worst["dreg"], f)
    _note("rpn ", worst)


def check_head(got, want):
    out, dcls, dbbox = got
    worst = {}
    print("out", out, "want", want["out"], "bound", want["out_bound"])
    assert R.same_float_bits(out[1], want["out"][1]) and R.same_float_bits(out[3], want["out"][3]), "acc / avg"
    for k, i in (("loss_cls", 0), ("loss_bbox", 2)):
        ok, worst[k] = R.inside(out[i], want["out"][i], want["out_bound"][i])
        assert ok, k
    ok, worst["dcls"] = R.inside(dcls, want["dcls"], want["dcls_bound"])
    print("dcls fraction of the bound", worst["dcls"])
    assert ok, "dcls"
    ok, worst["dbbox"] = R.inside(dbbox, want["dbbox"], want["dbbox_bound"])
    print("dbbox fraction of the bound", worst["dbbox"])
    assert ok, "dbbox"
    _note("head ", worst)


# ------------------------------------------------------------------------------------------------ RPN
@pytest.mark.parametrize("name", sorted(R.RPN_CASES))
def test_rpn_loss_and_gradients_are_inside_the_bounds(hip, name):
    c = R.rpn_case(name)
    got, want = rpn_kernel(hip, c), R.rpn_ref(c)
    check_rpn(got, want)
    if name in R.RPN_EXACT:                                    # dyadic inputs: sums exact in any order, one rounded division
        for l in range(len(c["levels"])):
            assert R.same_float_bits(got[1][l], want["dcls"][l]) and R.same_float_bits(got[2][l], want["dreg"][l]), l
        assert R.same_float_bits(got[0][:, 1], want["losses"][:, 1])
    if name in ("zero", "nonfinite", "hostile"):               # exact zeros wherever the weight is zero or the label is hostile
        off = 0
        for l, (h, w) in enumerate(c["levels"]):
            n = h * w * c["A"]
            lab, lw = c["labels"][:, off:off + n], c["lw"][:, off:off + n]
            dead = R._dense((lw == 0) | ((lab != 0) & (lab != 1)), c["B"], h, w, c["A"])
            assert not got[1][l][dead].any() and not got[2][l][R._dense(c["bw"][:, off:off + n] == 0, c["B"], h, w, 4 * c["A"])].any()
            off += n
    if name == "zero":
        assert not got[0].any()
    if name == "big":
        assert np.isfinite(got[0]).all() and got[0][:, 0].max() > 100


@pytest.mark.parametrize("name", ["five_A3_B3", "one_5x7_A3_B1", "dyadic"])
def test_rpn_forward_only_and_misaligned_gradients_give_the_same_bits(hip, name):
    c = R.rpn_case(name)
    base = rpn_kernel(hip, c)
    fwd = rpn_kernel(hip, c, grad=False)
    assert R.same_float_bits(fwd[0], base[0])
    mis = rpn_kernel(hip, c, misalign=True)                    # scalar stores: the address, not the shape, decides
    assert R.same_float_bits(mis[0], base[0])
    for l in range(len(c["levels"])):
        assert R.same_float_bits(mis[1][l], base[1][l]) and R.same_float_bits(mis[2][l], base[2][l])


def test_rpn_loss_several_workgroups_per_segment(hip):
    """80 x 80 cells, A = 3, B = 2: 38 and 150 workgroups in the two segments, partial sums added by the finishing launch."""
    rng = np.random.default_rng(21)
    B, A, h, w = 2, 3, 80, 80
    N = h * w * A
    c = dict(levels=[(h, w)], A=A, B=B, N=N, cls=[rng.normal(0, 3, (B, A, h, w)).astype(np.float32)],
             reg=[rng.normal(0, 1, (B, 4 * A, h, w)).astype(np.float32)], labels=np.ones((B, N), np.int32), lw=np.zeros((B, N), np.float32),
             bt=np.zeros((B, N, 4), np.float32), bw=np.zeros((B, N, 4), np.float32), avg=512.0)
    for b in range(B):
        pick = rng.choice(N, 256, replace=False)
        c["lw"][b, pick] = 1
        c["labels"][b, pick[:100]] = 0
        c["bw"][b, pick[:100]] = 1
        c["bt"][b, pick[:100]] = rng.normal(0, 1, (100, 4)).astype(np.float32)
    check_rpn(rpn_kernel(hip, c), R.rpn_ref(c))


def test_rpn_autograd_is_the_kernels_gradient_times_the_upstream(hip):
    from clipself_amd import det_losses as D
    c = R.rpn_case("five_A3_B3")
    _, dcls, dreg = rpn_kernel(hip, c)
    cls = [_dev(v).requires_grad_() for v in c["cls"]]
    reg = [_dev(v).requires_grad_() for v in c["reg"]]
    out = D.rpn_loss(cls, reg, _dev(c["labels"]), _dev(c["lw"]), _dev(c["bt"]), _dev(c["bw"]), torch.tensor(int(c["avg"]), device="cuda"),
                     loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=2.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
                     ops=hip, fused=True)
    L = len(cls)
    up_c, up_b = [0.5 * (l + 1) for l in range(L)], [-0.25 * (l + 1) for l in range(L)]
    (sum(u * v for u, v in zip(up_c, out["loss_rpn_cls"])) + sum(u * v for u, v in zip(up_b, out["loss_rpn_bbox"]))).backward()
    for l in range(L):
        assert R.same_float_bits(_np(cls[l].grad), dcls[l] * np.float32(2.0 * up_c[l]))
        assert R.same_float_bits(_np(reg[l].grad), dreg[l] * np.float32(up_b[l]))


# ------------------------------------------------------------------------------------------------ box head
@pytest.mark.parametrize("name", sorted(R.HEAD_CASES))
def test_bbox_head_loss_and_gradients_are_inside_the_bounds(hip, name):
    c = R.head_case(name)
    got, want = head_kernel(hip, c), R.head_ref(c)
    check_head(got, want)
    if name in R.HEAD_EXACT:
        assert R.same_float_bits(got[2], want["dbbox"]) and R.same_float_bits(got[0][2], want["out"][2])
        if name == "uniform":
            assert R.same_float_bits(got[1], want["dcls"])
    if name == "departures":
        assert not got[1][:5].any() and not got[1][c["lw"] == 0].any() and not got[2][c["lw"] == 0].any()
        assert got[1][5].any() and np.isfinite(got[0]).all()
    if name == "nopos":
        assert got[0][2] == 0 and not got[2].any()
    if name == "R0":
        assert got[0].tolist() == [0.0, 0.0, 0.0, 1.0]
    fwd = head_kernel(hip, c, grad=False)
    assert R.same_float_bits(fwd[0], got[0])


def test_bbox_head_autograd_is_the_kernels_gradient_times_the_upstream(hip):
    from clipself_amd import det_losses as D
    c = R.head_case("padded_masked")
    o4, dcls, dbbox = head_kernel(hip, c)
    x = _dev(c["x"])[:, :c["C1"]].clone().requires_grad_()
    bp = _dev(c["bp"]).requires_grad_()
    cfg = dict(type="CustomCrossEntropyLoss", use_sigmoid=False, loss_weight=1.0, class_weight=c["cw"].tolist())
    out = D.bbox_head_loss(x, bp, _dev(c["labels"]), _dev(c["lw"]), _dev(c["bt"]), _dev(c["bw"]), loss_cls=cfg,
                           loss_bbox=dict(type="L1Loss", loss_weight=3.0), num_classes=c["bg"], ops=hip, fused=True)
    (out["loss_cls"] * 0.5 + out["loss_bbox"] + out["acc"]).backward()
    assert R.same_float_bits(_np(out["loss_cls"].detach()), o4[0]) and R.same_float_bits(_np(out["acc"]), o4[1])
    assert R.same_float_bits(_np(x.grad), dcls * np.float32(0.5)) and R.same_float_bits(_np(bp.grad), dbbox * np.float32(3.0))
