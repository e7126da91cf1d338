"""CPU: the detector's losses (clipself_amd/det_losses.py, include/clipself_loss.h).

The two restatements of tests/_loss_ref.py against each other in float64: mmdet 2.28.1's expressions with autograd, and the closed
forms.  The torch route against the closed forms inside the derived bounds, on the whole case table, every departure included.  The
bounds reject four planted errors.  The mmdet-named modules built from the reference configs' dicts; the unsupported keywords;
`rpn_targets -> rpn_loss` and `rcnn_targets -> bbox_head_loss` end to end with backward(); the C ABI: header, table, exports, limits."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _loss_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype) if dtype else torch.from_numpy(np.ascontiguousarray(a))


def rpn_torch_route(c):
    from clipself_amd import det_losses as D
    losses, dcls, dreg = D.rpn_loss_torch([_t(v) for v in c["cls"]], [_t(v) for v in c["reg"]], _t(c["labels"]), _t(c["lw"]), _t(c["bt"]),
                                          _t(c["bw"]), torch.tensor([c["avg"]], dtype=torch.float32))
    return losses.numpy(), [g.numpy() for g in dcls], [g.numpy() for g in dreg]


def head_torch_route(c):
    from clipself_amd import det_losses as D
    x = _t(c["x"])[:, :c["C1"]]
    before = c["x"].copy()
    avg = None if c["avg"] is None else torch.tensor([c["avg"]], dtype=torch.float32)
    out, dcls, dbbox = D.bbox_head_loss_torch(x, _t(c["labels"]), _t(c["lw"]), _t(c["bp"]), _t(c["bt"]), _t(c["bw"]), c["bg"], _t(c["cw"]), avg)
    assert np.array_equal(before, c["x"], equal_nan=True), "the caller's logits were written"
    return out.numpy(), dcls.numpy(), dbbox.numpy()


def check_rpn(got, want, report=None):
    losses, dcls, dreg = got
    worst = {}
    ok, worst["loss_cls"] = R.inside(losses[:, 0], want["losses"][:, 0], want["losses_bound"][:, 0])
    assert ok, ("loss_cls", losses[:, 0], want["losses"][:, 0], want["losses_bound"][:, 0])
    ok, worst["loss_bbox"] = R.inside(losses[:, 1], want["losses"][:, 1], want["losses_bound"][:, 1])
    assert ok, ("loss_bbox", losses[:, 1], want["losses"][:, 1], want["losses_bound"][:, 1])
    worst["dcls"] = worst["dreg"] = 0.0
    for l in range(len(dcls)):
        ok, f = R.inside(dcls[l], want["dcls"][l], want["dcls_bound"][l])
        assert ok, ("dcls", l, f)
        worst["dcls"] = max(worst["dcls"], f)
        ok, f = R.inside(dreg[l], want["dreg"][l], want["dreg_bound"][l])
        assert ok, ("dreg", l, f)
        worst["dreg"] = max(worst["dreg"], f)
    if report is not None:
        for k, v in worst.items():
            report[k] = max(report.get(k, 0.0), v)
    return worst


def check_head(got, want, report=None):
    out, dcls, dbbox = got
    worst = {}
    assert R.same_float_bits(out[1], want["out"][1]) and R.same_float_bits(out[3], want["out"][3]), ("acc / avg", out, want["out"])
    for k, i in (("loss_cls", 0), ("loss_bbox", 2)):
        ok, worst[k] = R.inside(out[i], want["out"][i], want["out_bound"][i])
        assert ok, (k, out[i], want["out"][i], want["out_bound"][i])
    ok, worst["dcls"] = R.inside(dcls, want["dcls"], want["dcls_bound"])
    assert ok, ("dcls", worst["dcls"])
    ok, worst["dbbox"] = R.inside(dbbox, want["dbbox"], want["dbbox_bound"])
    assert ok, ("dbbox", worst["dbbox"])
    if report is not None:
        for k, v in worst.items():
            report[k] = max(report.get(k, 0.0), v)
    return worst


# ------------------------------------------------------------------------------------------------ (a) against (b), float64
@pytest.mark.parametrize("name", R.RPN_PLAIN)
def test_rpn_mmdet_transcription_equals_the_closed_form(name):
    c = R.rpn_case(name)
    losses, dcls, dreg = R.rpn_mmdet(c)
    want = R.rpn_ref(c, den_exact=True)
    np.testing.assert_allclose(losses, want["losses"], rtol=1e-12, atol=1e-300)
    for l in range(len(dcls)):
        np.testing.assert_allclose(dcls[l], want["dcls"][l], rtol=1e-11, atol=1e-18)
        np.testing.assert_allclose(dreg[l], want["dreg"][l], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", R.HEAD_PLAIN)
def test_head_mmdet_transcription_equals_the_closed_form(name):
    c = R.head_case(name)
    out, dcls, dbbox = R.head_mmdet(c)
    want = R.head_ref(c, den_exact=True)
    np.testing.assert_allclose(out[[0, 2, 3]], want["out"][[0, 2, 3]], rtol=1e-11, atol=1e-300)
    assert abs(out[1] - want["out"][1]) < 1e-3                               # mmdet's accuracy is an fp32 product with 100 / R
    np.testing.assert_allclose(dcls, want["dcls"], rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(dbbox, want["dbbox"], rtol=1e-12, atol=0)


def test_a_masked_label_is_nan_in_torch_and_zero_here():
    """The departure the header states: F.cross_entropy on a row whose own label holds -inf is 0 * -inf."""
    c = R.head_case("departures")
    keep = np.array([4, 5, 6])
    c2 = dict(c, R=3, x=c["x"][keep], labels=c["labels"][keep], lw=np.ones(3, np.float32), bp=c["bp"][keep], bt=c["bt"][keep], bw=c["bw"][keep])
    assert c2["cw"][c2["labels"][0]] < 1e-5
    out, _, _ = R.head_mmdet(c2)
    assert np.isnan(out[0])
    want = R.head_ref(c2)
    assert np.isfinite(want["out"]).all() and not want["dcls"][0].any() and want["dcls"][1].any()


# ------------------------------------------------------------------------------------------------ the torch route against (b)
@pytest.mark.parametrize("name", sorted(R.RPN_CASES))
def test_rpn_torch_route_is_inside_the_bounds(name):
    c = R.rpn_case(name)
    got, want = rpn_torch_route(c), R.rpn_ref(c)
    print(name, check_rpn(got, want))
    if name in R.RPN_EXACT:
        for l in range(len(c["levels"])):
            assert R.same_float_bits(got[1][l], want["dcls"][l]) and R.same_float_bits(got[2][l], want["dreg"][l]), l
        assert R.same_float_bits(got[0][:, 1], want["losses"][:, 1])
    if name in ("zero", "nonfinite", "hostile"):
        off = 0
        for l, (h, w) in enumerate(c["levels"]):
            n = h * w * c["A"]
            lab, lw = c["labels"][:, off:off + n], c["lw"][:, off:off + n]
            dead = R._dense((lw == 0) | ((lab != 0) & (lab != 1)), c["B"], h, w, c["A"])
            assert not got[1][l][dead].any() and np.isfinite(got[1][l]).all() and np.isfinite(got[2][l]).all()
            off += n
    if name == "zero":
        assert not got[0].any()


@pytest.mark.parametrize("name", sorted(R.HEAD_CASES))
def test_head_torch_route_is_inside_the_bounds(name):
    c = R.head_case(name)
    got, want = head_torch_route(c), R.head_ref(c)
    print(name, check_head(got, want))
    if name in R.HEAD_EXACT:
        assert R.same_float_bits(got[2], want["dbbox"]) and R.same_float_bits(got[0][2], want["out"][2])
        if name == "uniform":
            assert R.same_float_bits(got[1], want["dcls"])
    if name == "departures":
        assert not got[1][:5].any() and not got[1][c["lw"] == 0].any() and not got[2][c["lw"] == 0].any()
        assert got[1][5].any() and np.isfinite(got[0]).all()
    if name == "nopos":
        assert got[0][2] == 0 and not got[2].any()
    if name == "ties":
        assert want["out"][1] > 0


def test_ties_go_to_the_lowest_index():
    c = R.head_case("ties")
    c["labels"][0], c["lw"][0] = 0, 1                                           # row 0 is all ones: class 0 is its argmax
    base = R.head_ref(c)["out"][1]
    c["labels"][0] = 1
    assert R.head_ref(c)["out"][1] < base
    assert R.same_float_bits(head_torch_route(c)[0][1], R.head_ref(c)["out"][1])


# ------------------------------------------------------------------------------------------------ the bounds are not vacuous
def _rejected(got, want, keys):
    for k in keys:
        g, w, b = got[k], want[k], want[k + "_bound"]
        for gi, wi, bi in (zip(g, w, b) if isinstance(g, list) else [(g, w, b)]):
            if not R.inside(gi, wi, bi)[0]:
                return True
    return False


def test_the_bounds_reject_four_planted_errors():
    """The restatement with one error planted, held against the restatement: each must leave its bound somewhere."""
    hc = R.head_case("C66")
    assert not _rejected(R.head_ref(hc), R.head_ref(hc), ("out", "dcls", "dbbox"))
    assert _rejected(R.head_ref(hc, plant="drop_class"), R.head_ref(hc), ("out", "dcls"))          # one class out of one row's denominator
    rc = R.rpn_case("five_A3_B3")
    assert not _rejected(R.rpn_ref(rc), R.rpn_ref(rc), ("losses", "dcls", "dreg"))
    assert _rejected(R.rpn_ref(rc, plant="shift_anchor"), R.rpn_ref(rc), ("dcls",))                 # anchor (x, a) read as (x, a + 1)
    dc = R.rpn_case("dyadic_5x7")                                                                   # holds exact zeros of pred - target; avg = 1
    assert _rejected(R.rpn_ref(dc, plant="sign0"), R.rpn_ref(dc), ("dreg",))                        # sign(0) taken as 1
    assert _rejected(R.rpn_ref(dc, plant="no_eps"), R.rpn_ref(dc), ("dreg",))                       # the eps left out at avg_factor = 1
    uc = R.head_case("uniform_avg1")
    assert _rejected(R.head_ref(uc, plant="sign0"), R.head_ref(uc), ("dbbox",))


# ------------------------------------------------------------------------------------------------ modules and keywords
def test_modules_build_from_the_reference_configs():
    from clipself_amd import det_losses as D
    class_weight = [1.0] * 48 + [0.0] * 17 + [1.0]                           # the shape of the ov_coco configs' list: novel classes 0
    rpn_cls = dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0)
    l1 = dict(type="L1Loss", loss_weight=1.0)
    coco = dict(type="CustomCrossEntropyLoss", use_sigmoid=False, loss_weight=1.0, class_weight=class_weight)
    m = D.build_loss(rpn_cls)
    assert isinstance(m, D.CrossEntropyLoss) and m.use_sigmoid and m.loss_weight == 1.0 and m.class_weight is None
    assert isinstance(D.build_loss(l1), D.L1Loss)
    m = D.build_loss(coco)
    assert isinstance(m, D.CustomCrossEntropyLoss) and m.class_weight == class_weight and m.bg_weight == 1.0
    assert D.build_loss(m) is m


def test_class_weight_as_a_path_is_read_as_load_class_freq_does(tmp_path):
    from clipself_amd import det_losses as D
    info = [dict(id=3, image_count=0), dict(id=1, image_count=7), dict(id=2, image_count=1)]
    p = tmp_path / "cat_info.json"
    p.write_text(json.dumps(info))
    lvis = dict(type="CustomCrossEntropyLoss", use_sigmoid=False, loss_weight=1.0, bg_weight=0.9, class_weight=str(p))
    m = D.build_loss(lvis)
    assert m.class_weight == pytest.approx([1.0, 1.0, 0.0, 0.9]) and m.bg_weight == 0.9
    assert D.load_class_freq(str(p), freq_weight=0.5).tolist() == pytest.approx([7 ** 0.5, 1.0, 0.0])
    with pytest.raises(ValueError):
        D.CrossEntropyLoss(class_weight=str(p))


@pytest.mark.parametrize("kw", [dict(use_mask=True), dict(reduction="sum"), dict(reduction="none"), dict(avg_non_ignore=True),
                                dict(ignore_index=255), dict(type="FocalLoss"), dict(use_sigmoid=True, class_weight=[1.0, 1.0])])
def test_unsupported_keywords_raise(kw):
    from clipself_amd import det_losses as D
    with pytest.raises(ValueError):
        D.CrossEntropyLoss(**kw)
    if "type" not in kw:
        with pytest.raises(ValueError):
            D.CustomCrossEntropyLoss(**kw)


def test_unsupported_forms_of_the_batched_calls_raise():
    from clipself_amd import det_losses as D
    with pytest.raises(ValueError):
        D.L1Loss(reduction="sum")
    with pytest.raises(ValueError):
        D.build_loss(dict(type="SmoothL1Loss"))
    c = R.head_case("C66")
    args = [_t(c["x"]), _t(c["bp"]), _t(c["labels"]), _t(c["lw"]), _t(c["bt"]), _t(c["bw"])]
    with pytest.raises(ValueError):
        D.bbox_head_loss(*args, loss_cls=D.CrossEntropyLoss(use_sigmoid=True), num_classes=65)
    with pytest.raises(ValueError):
        D.bbox_head_loss(args[0], torch.zeros(9, 4 * 65), *args[2:], num_classes=65)            # class-specific regression
    with pytest.raises(ValueError):
        D.bbox_head_loss(*args, loss_cls=D.CustomCrossEntropyLoss(class_weight=[1.0] * 5), num_classes=65)
    with pytest.raises(NotImplementedError):
        D.bbox_head_loss(*args, num_classes=65, fused=True)                                      # CPU tensors have no kernel route
    rc = R.rpn_case("one_5x7_A3_B1")
    rargs = [[_t(v) for v in rc["cls"]], [_t(v) for v in rc["reg"]], _t(rc["labels"]), _t(rc["lw"]), _t(rc["bt"]), _t(rc["bw"]), 4]
    with pytest.raises(ValueError):
        D.rpn_loss(*rargs, loss_cls=D.CrossEntropyLoss(use_sigmoid=False))
    with pytest.raises(ValueError):
        D.rpn_loss(rargs[0], rargs[1], rargs[2][:, :-1], *rargs[3:])


# ------------------------------------------------------------------------------------------------ autograd and the batched forms
def test_rpn_loss_autograd_is_the_saved_gradient_times_the_upstream():
    from clipself_amd import det_losses as D
    c = R.rpn_case("five_A3_B3")
    cls = [_t(v).requires_grad_() for v in c["cls"]]
    reg = [_t(v).requires_grad_() for v in c["reg"]]
    out = D.rpn_loss(cls, reg, _t(c["labels"]), _t(c["lw"]), _t(c["bt"]), _t(c["bw"]), torch.tensor(int(c["avg"])),
                     loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=2.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0))
    L = len(cls)
    assert len(out["loss_rpn_cls"]) == L and len(out["loss_rpn_bbox"]) == L and out["loss_rpn_cls"][0].dim() == 0
    up_c, up_b = [0.5 * (l + 1) for l in range(L)], [-0.25 * (l + 1) for l in range(L)]
    total = sum(u * v for u, v in zip(up_c, out["loss_rpn_cls"])) + sum(u * v for u, v in zip(up_b, out["loss_rpn_bbox"]))
    total.backward()
    losses, dcls, dreg = rpn_torch_route(c)
    for l in range(L):
        assert R.same_float_bits(out["loss_rpn_cls"][l].detach().numpy(), np.float32(2.0) * losses[l, 0])
        assert R.same_float_bits(cls[l].grad.numpy(), dcls[l] * np.float32(2.0 * up_c[l]))
        assert R.same_float_bits(reg[l].grad.numpy(), dreg[l] * np.float32(up_b[l]))


def test_bbox_head_loss_autograd_and_bf16_inputs():
    from clipself_amd import det_losses as D
    c = R.head_case("padded_masked")
    x = _t(c["x"])[:, :c["C1"]].clone().requires_grad_()
    bp = _t(c["bp"]).requires_grad_()
    cfg = dict(type="CustomCrossEntropyLoss", use_sigmoid=False, loss_weight=1.0, class_weight=c["cw"].tolist())
    out = D.bbox_head_loss(x, bp, _t(c["labels"]), _t(c["lw"]), _t(c["bt"]), _t(c["bw"]), loss_cls=cfg, loss_bbox=dict(type="L1Loss", loss_weight=3.0),
                           num_classes=c["bg"])
    assert set(out) == {"loss_cls", "acc", "loss_bbox"} and not out["acc"].requires_grad
    (out["loss_cls"] * 0.5 + out["loss_bbox"] + out["acc"]).backward()
    o4, dcls, dbbox = head_torch_route(c)
    assert R.same_float_bits(out["loss_cls"].detach().numpy(), o4[0]) and R.same_float_bits(out["acc"].numpy(), o4[1])
    assert R.same_float_bits(x.grad.numpy(), dcls * np.float32(0.5)) and R.same_float_bits(bp.grad.numpy(), dbbox * np.float32(3.0))
    xb = _t(c["x"])[:, :c["C1"]].to(torch.bfloat16).requires_grad_()          # force_fp32: any float dtype goes in, its gradient comes back
    out = D.bbox_head_loss(xb, _t(c["bp"]), _t(c["labels"]).long(), _t(c["lw"]), _t(c["bt"]), _t(c["bw"]), loss_cls=cfg, num_classes=c["bg"])
    out["loss_cls"].backward()
    assert xb.grad.dtype == torch.bfloat16 and xb.grad.abs().sum() > 0


def test_targets_compose_with_the_losses_end_to_end():
    """rpn_targets -> rpn_loss and rcnn_targets -> bbox_head_loss on CPU tensors; backward() reaches the predictions."""
    from clipself_amd import det_losses as D
    from clipself_amd import det_targets as T
    gen = torch.Generator().manual_seed(3)
    side, B, A = 64, 2, 3
    sizes = R.level_sizes(side)
    ag = T.AnchorGenerator(strides=[4, 8, 16, 32, 64], ratios=[0.5, 1.0, 2.0], scales=[8])
    anchors = torch.cat(ag.grid_priors(sizes))
    assert anchors.shape[0] == 1023
    # the anchor order the kernels assume: anchor n of a level is (y * w + x) * A + a
    lvl0 = ag.grid_priors(sizes)[0].reshape(16, 16, A, 4)
    assert torch.equal(lvl0[2, 5, 1] - lvl0[0, 0, 1], torch.tensor([20.0, 8.0, 20.0, 8.0]))
    gts = [torch.tensor([[4.0, 6.0, 40.0, 50.0], [20.0, 10.0, 60.0, 30.0]]), torch.tensor([[8.0, 8.0, 56.0, 56.0]])]
    labels, lw, bt, bw, num = T.rpn_targets(anchors, None, gts, T.MaxIoUAssigner(0.7, 0.3, 0.3, match_low_quality=True),
                                            T.RandomSampler(256, 0.5, add_gt_as_proposals=False), generator=gen)
    cls = [torch.randn(B, A, h, w, generator=gen).requires_grad_() for h, w in sizes]
    reg = [torch.randn(B, 4 * A, h, w, generator=gen).requires_grad_() for h, w in sizes]
    out = D.rpn_loss(cls, reg, labels, lw, bt, bw, num, loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                     loss_bbox=dict(type="L1Loss", loss_weight=1.0))
    total = sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])
    assert torch.isfinite(total) and total > 0
    total.backward()
    assert sum(float(c.grad.abs().sum()) for c in cls) > 0 and sum(float(r.grad.abs().sum()) for r in reg) > 0
    assert sum(int((c.grad != 0).sum()) for c in cls) == int((lw != 0).sum())

    props = [torch.cat([g + 2.0, torch.rand(30, 4, generator=gen).sort(dim=1).values * side]) for g in gts]
    props = [p[:, [0, 1, 2, 3]] for p in props]
    rois, lab, rlw, rbt, rbw = T.rcnn_targets(props, gts, [torch.tensor([3, 7]), torch.tensor([11])], T.MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False),
                                              T.RandomSampler(16, 0.25, add_gt_as_proposals=True), num_classes=65, generator=gen)
    n = rois.shape[0]
    x = torch.randn(n, 66, generator=gen).requires_grad_()
    bp = torch.randn(n, 4, generator=gen).requires_grad_()
    out = D.bbox_head_loss(x, bp, lab, rlw, rbt, rbw, loss_cls=dict(type="CustomCrossEntropyLoss", use_sigmoid=False, loss_weight=1.0,
                                                                     class_weight=[1.0] * 48 + [0.0] * 17 + [1.0]), num_classes=65)
    (out["loss_cls"] + out["loss_bbox"]).backward()
    assert torch.isfinite(out["loss_cls"]) and 0 <= float(out["acc"]) <= 100
    assert float(x.grad.abs().sum()) > 0 and float(bp.grad.abs().sum()) > 0 and not x.grad[:, 48:65].any()


def test_no_host_reads_on_the_kernel_route():
    text = (ROOT / "clipself_amd" / "det_losses.py").read_text()
    for word in (".item()", ".cpu()", "nonzero", ".tolist()"):
        assert word not in text.replace("(load_class_freq(self.class_weight, min_count=0) > 0.0).float().tolist()", ""), word
    src = (ROOT / "clipself_amd" / "csrc" / "det_loss.hip").read_text()
    assert "atomic" not in re.sub(r"//.*", "", src)
    assert "hipMalloc" not in src and "Synchronize" not in src


# ------------------------------------------------------------------------------------------------ the C ABI
def test_limits_are_refused_without_a_device():
    """Argument checks come before any launch, so the -1 cases can be seen here: no pointer is touched."""
    from clipself_amd import hip
    lib = hip.load_library()
    P = 1 << 20

    def levels(*hw, grads=True):
        arr = (hip.LossLevel * len(hw))()
        for i, (h, w) in enumerate(hw):
            arr[i] = hip.LossLevel(P, P, P if grads else None, P if grads else None, h, w)
        return arr

    ws = lib.csl_workspace
    assert ws(None, 0, 1, 1, 0) >= 256 and ws(None, 0, 1, 1, 4096) >= 4096 * 12 and ws(None, 0, 1, 1, -1) == 0 and ws(None, 0, 1, 1, P + 1) == 0
    five = levels(*R.level_sizes(1024))
    blocks = sum(-(-8 * 3 * (h * w // 4) // 256) + -(-8 * 12 * (h * w // 4) // 256) for h, w in R.level_sizes(1024))
    assert ws(five, 5, 8, 3, 0) >= 4 * blocks
    assert ws(five, 9, 8, 3, 0) == 0 and ws(five, 5, 0, 3, 0) == 0 and ws(five, 5, 65536, 3, 0) == 0 and ws(five, 5, 8, 17, 0) == 0
    assert ws(levels((513, 4)), 1, 1, 1, 0) == 0 and ws(levels((4, 0)), 1, 1, 1, 0) == 0 and ws(levels((512, 512)), 1, 65535, 16, 0) == 0

    def rpn(lv=None, L=1, B=1, A=3, labels=P, avg=P, losses=P, w=P):
        return lib.csl_rpn_loss(lv if lv is not None else levels((5, 7)), L, B, A, labels, P, P, P, avg, losses, w, None)

    mixed = levels((5, 7), (3, 4))
    mixed[1].dcls = mixed[1].dreg = None
    half = levels((5, 7))
    half[0].dreg = None
    for kw, word in [(dict(L=0), b"L ="), (dict(L=9), b"L ="), (dict(B=0), b"B ="), (dict(B=65536), b"B ="), (dict(A=0), b"A ="), (dict(A=17), b"A ="),
                     (dict(lv=levels((0, 7))), b"h ="), (dict(lv=levels((5, 513))), b"w ="), (dict(lv=levels((512, 512)), B=65535, A=16), b"2^31"),
                     (dict(lv=mixed, L=2), b"every level"), (dict(lv=half), b"together"), (dict(labels=None), b"targets"), (dict(avg=None), b"avg_factor"),
                     (dict(losses=None), b"losses"), (dict(w=None), b"workspace")]:
        assert rpn(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())

    def head(R_=8, C1=66, ldc=66, x=P, bp=P, out=P, w=P):
        return lib.csl_bbox_head_loss(x, ldc, P, P, None, bp, P, P, R_, C1, 65, None, out, P, P, w, None)

    for kw, word in [(dict(R_=-1), b"R ="), (dict(R_=P + 1), b"R ="), (dict(C1=0, ldc=1), b"C1"), (dict(C1=4097, ldc=4097), b"C1"), (dict(ldc=65), b"ldc"),
                     (dict(x=None), b"cls_score"), (dict(bp=None), b"bbox_pred"), (dict(out=None), b"out"), (dict(w=None), b"workspace")]:
        assert head(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())
    assert ctypes.sizeof(hip.LossLevel) == 40
