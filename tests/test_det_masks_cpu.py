"""CPU: the detector's mask branch (clipself_amd/det_masks.py, include/clipself_mask.h) on the torch route, against the
restatements of tests/_mask_ref.py: the targets inside the derived bound (binary form equal outside the undecided band), the loss and its
gradient inside their bounds and equal to mmdet's expression in torch float64, the paste against F.grid_sample in float64.  The band caps
are asserted from the reference alone, the bounds must reject four planted errors, and `rcnn_targets(return_gt_inds=True)` must name the
ground truth of every positive slot."""
import numpy as np
import pytest
import torch

import _assign_ref as A
import _mask_ref as R
from clipself_amd import det_masks as DM

RAND = [f"rand{i}" for i in range(24)]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _target_torch(c, soft):
    return DM.mask_target(_t(c["rois"]), _t(c["gt_rows"]), _t(c["masks"]), c["M"], soft=soft).numpy()


# ------------------------------------------------------------------------------------------------ targets
def test_scalar_loops_and_vectorised_target_restatements_agree():
    for c in (R.target_case("small"), R.dyadic_case(4)):
        loops = R.target_loops(c["rois"], c["gt_rows"], c["masks"], c["M"])
        assert np.abs(loops - c["ref"]["t"]).max() <= 1e-12
    assert R.target_case("small")["ref"]["t"][[1, 2, 4, 6]].max() == 0          # gt_rows -1 / out of range, zero width, NaN box
    assert R.target_case("large")["ref"]["grids"].max() >= 4


@pytest.mark.parametrize("name", R.TARGET_RANDOM + RAND[:4])
def test_target_torch_route_is_inside_the_bound(name):
    c = R.target_case(name)
    ok, frac = R.inside(_target_torch(c, True), c["ref"]["t"], c["ref"]["bound"])
    print(name, "soft: worst fraction of the bound", frac)
    assert ok
    ok, band = R.binary_check(_target_torch(c, False), c["ref"]["t"], c["ref"]["bound"], 0.5)
    assert ok, (name, band)


@pytest.mark.parametrize("M", [4, 14])
def test_target_dyadic_cases_are_exact(M):
    c = R.dyadic_case(M)
    assert c["ref"]["exact"], "the case must make every partial sum an fp32 number"
    assert R.same_bits(_target_torch(c, True), c["ref"]["t"].astype(np.float32))
    assert R.binary_target_ok(c["ref"], _target_torch(c, False))
    assert (c["ref"]["t"] == 0.5).any(), "the case holds exact ties"


def test_target_known_answers():
    masks = R.blob_masks(1, 60, 60, 9, noise=0.2)
    rois = np.array([[0, 0, 0, 28, 28], [0, 0, 0, 56, 56]], np.float32)
    ref = R.target_vec(rois, np.zeros(2, np.int32), masks, 28)
    corner = (masks[0, :28, :28] != 0)
    assert np.array_equal(ref["t"][0], corner.astype(np.float64))
    quads = (masks[0, :56, :56] != 0).reshape(28, 2, 28, 2).sum(axis=(1, 3)) / 4.0
    assert np.array_equal(ref["t"][1], quads) and (quads == 0.5).any()
    got = DM.mask_target(_t(rois), torch.zeros(2, dtype=torch.int32), _t(masks), 28).numpy()
    assert np.array_equal(got[0], corner.astype(np.uint8)) and np.array_equal(got[1], (quads >= 0.5).astype(np.uint8))


def test_band_caps_hold_from_the_reference_alone():
    """At most 2 % of any one case's outputs and at most 0.1 % of all random outputs lie in the undecided band."""
    tot = band_tot = 0
    for name in R.TARGET_RANDOM + RAND:
        ref = R.target_case(name)["ref"]
        band = int((np.abs(ref["t"] - 0.5) <= ref["bound"]).sum())
        assert band <= 0.02 * ref["t"].size, (name, band)
        tot, band_tot = tot + ref["t"].size, band_tot + band
    print("target: in the band", band_tot, "of", tot)
    assert band_tot <= 1e-3 * tot
    tot = band_tot = 0
    for name in R.PASTE_RANDOM:
        c = R.paste_case(name)
        band = int((np.abs(c["ref"]["v"] - c["thr"]) <= c["ref"]["bound"]).sum())
        assert band <= 0.02 * c["ref"]["v"].size, (name, band)
        tot, band_tot = tot + c["ref"]["v"].size, band_tot + band
    print("paste: in the band", band_tot, "of", tot)
    assert band_tot <= 1e-3 * tot


def test_mask_target_takes_a_list_and_refuses_mixed_sizes():
    c = R.target_case("small")
    whole = _target_torch(c, False)
    parts = DM.mask_target(_t(c["rois"]), _t(c["gt_rows"]), [_t(c["masks"][:2]), _t(c["masks"][2:])], c["M"]).numpy()
    assert np.array_equal(whole, parts)
    with pytest.raises(ValueError):
        DM.mask_target(_t(c["rois"]), _t(c["gt_rows"]), [_t(c["masks"][:2]), _t(c["masks"][2:, :30])], c["M"])
    with pytest.raises(NotImplementedError):
        DM.mask_target(_t(c["rois"]), _t(c["gt_rows"]), _t(c["masks"]), c["M"], fused=True)


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("name", sorted(R.LOSS_CASES))
def test_loss_torch_route_and_the_two_references(name):
    c = R.loss_case(name)
    want = R.loss_ref(c)
    if c["plain"]:
        loss, grad = R.loss_mmdet(c)
        assert abs(loss - want["out"][0]) <= 1e-11 * max(1.0, abs(loss))
        # (a) divides by the exact n * M * M, (b) by its fp32 value: the same number for these shapes
        assert float(np.float32(want["out"][1] * c["M"] ** 2)) == want["out"][1] * c["M"] ** 2
        assert np.abs(grad - want["dpred"]).max(initial=0) <= 1e-11
    out2, dpred = DM.mask_loss_torch(_t(c["pred"]), _t(c["labels"]), _t(c["targets"]), _t(c["w"]))
    ok, frac = R.inside(out2.numpy()[0], want["out"][0], want["out_bound"][0])
    print(name, "loss", out2.numpy(), want["out"], "fraction", frac)
    assert ok and float(out2[1]) == want["out"][1]
    ok, frac = R.inside(dpred.numpy(), want["dpred"], want["dpred_bound"])
    assert ok, frac


def test_mask_loss_autograd_and_config():
    c = R.loss_case("C3_labels")
    pred = _t(c["pred"]).clone().requires_grad_(True)
    cfg = dict(type='CrossEntropyLoss', use_mask=True, loss_weight=2.0)
    out = DM.mask_loss(pred, _t(c["targets"]), _t(c["labels"]), _t(c["w"]), class_agnostic=False, loss_mask=cfg)
    assert set(out) == {"loss_mask"}
    (out["loss_mask"] * 3.0).backward()
    out2, dpred = DM.mask_loss_torch(_t(c["pred"]), _t(c["labels"]), _t(c["targets"]), _t(c["w"]))
    assert torch.equal(out["loss_mask"].detach(), out2[0] * 2.0) and torch.equal(pred.grad, dpred * 6.0)
    agn = DM.mask_loss(_t(c["pred"]), _t(c["targets"]), _t(c["labels"]), _t(c["w"]))["loss_mask"]      # class-agnostic: channel 0 whatever the labels say
    want0 = DM.mask_loss_torch(_t(c["pred"]), None, _t(c["targets"]), _t(c["w"]))[0][0]
    assert torch.equal(agn, want0)


def test_build_loss_accepts_the_config_and_refuses_what_the_kernel_does_not_cover():
    from clipself_amd import det_losses
    m = DM.build_loss(dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0))
    assert isinstance(m, DM.MaskCrossEntropyLoss) and m.use_mask and m.loss_weight == 1.0 and DM.build_loss(m) is m
    for bad in (dict(reduction='sum'), dict(reduction='none'), dict(class_weight=[1.0]), dict(avg_factor=3), dict(avg_non_ignore=True),
                dict(use_sigmoid=True), dict(use_mask=False), dict(type='FocalLoss')):
        with pytest.raises((ValueError, TypeError)) as ei:
            DM.build_loss({**dict(type='CrossEntropyLoss', use_mask=True), **bad})
        assert ei.type is ValueError, bad
    with pytest.raises(ValueError):
        det_losses.CrossEntropyLoss(use_mask=True)                     # unchanged: the mask loss is built through det_masks.build_loss
    with pytest.raises(ValueError):
        det_losses.build_loss(dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0))


# ------------------------------------------------------------------------------------------------ paste
@pytest.mark.parametrize("name", R.PASTE_RANDOM)
def test_paste_torch_route_against_grid_sample(name):
    c = R.paste_case(name)
    out, soft = DM.paste_masks_torch(_t(c["logits"]), _t(c["labels"]), _t(c["boxes"]), c["img_h"], c["img_w"], c["thr"], return_soft=True)
    ok, frac = R.inside(soft.numpy(), c["ref"]["v"], c["ref"]["bound"])
    print(name, "soft: worst fraction of the bound", frac)
    assert ok
    ok, band = R.binary_check(out.numpy(), c["ref"]["v"], c["ref"]["bound"], c["thr"])
    assert ok, band
    assert out.numpy()[c["zero"]].max() == 0 and out.numpy()[c["live"]].max() == 1      # bad label, outside, zero extent, NaN; the live box
    pub = DM.paste_masks(_t(c["logits"]), _t(c["boxes"]), _t(c["labels"]), (c["img_h"], c["img_w"]), class_agnostic=False)
    assert torch.equal(pub, out)
    with pytest.raises(ValueError):
        DM.paste_masks(_t(c["logits"]), _t(c["boxes"]), _t(c["labels"]), (c["img_h"], c["img_w"]), thr=-1)


def test_paste_known_answers_and_get_seg_masks():
    M = 16                                                             # a power of two: (X + 0.5) / M and every later step is exact
    rng = np.random.default_rng(5)
    logits = rng.choice([-np.inf, 0.0, np.inf], size=(2, 1, M, M)).astype(np.float32)
    p = np.where(logits[:, 0] > 0, 1.0, np.where(logits[:, 0] < 0, 0.0, 0.5))
    boxes = np.array([[0, 0, M, M]] * 2, np.float32)
    out, soft = DM.paste_masks_torch(_t(logits), None, _t(boxes), M, M, 0.5, return_soft=True)
    assert np.array_equal(soft.numpy(), p.astype(np.float32)) and np.array_equal(out.numpy(), (p >= 0.5).astype(np.uint8))
    ref = R.paste_ref(logits, None, boxes, M, M)
    assert np.array_equal(ref["v"], p)
    boxes2 = np.array([[0, 0, 2 * M, 2 * M]] * 2, np.float32)
    ref2 = R.paste_ref(logits, None, boxes2, 2 * M, 2 * M)
    out2, soft2 = DM.paste_masks_torch(_t(logits), None, _t(boxes2), 2 * M, 2 * M, 0.5, return_soft=True)
    assert np.array_equal(soft2.numpy().astype(np.float64), ref2["v"]) and (ref2["v"] == 0.5).any()
    assert np.array_equal(out2.numpy(), (ref2["v"] >= 0.5).astype(np.uint8))
    segms = DM.get_seg_masks(_t(logits), _t(boxes2 * 2), torch.tensor([2, 0]), dict(mask_thr_binary=0.5), (2 * M, 2 * M, 3),
                             np.array([2.0, 2.0, 2.0, 2.0], np.float32), True, num_classes=3)
    assert [len(s) for s in segms] == [1, 0, 1] and segms[2][0].dtype == bool and np.array_equal(segms[2][0], out2.numpy()[0].astype(bool))


# ------------------------------------------------------------------------------------------------ rcnn_targets(return_gt_inds=True)
def test_rcnn_targets_returns_the_ground_truth_row_of_every_positive_slot():
    from clipself_amd import det_targets as T
    p, e = A.build_case("prefix_b3"), A.expected("prefix_b3")
    props, gt_list, lab_list = [], [], []
    for b in range(3):
        gs, ge = p["gt_starts"][b], p["gt_starts"][b + 1]
        gt_list.append(_t(p["gts"][gs:ge]))
        lab_list.append(_t(p["gt_labels"][gs:ge]))
        props.append(_t(p["boxes"][p["starts"][b] + (ge - gs):p["starts"][b + 1]]))
    keys = torch.from_numpy(np.ascontiguousarray(p["keys"]).view(np.int32).copy())
    assigner = T.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1)
    mk = lambda: T.RandomSampler(num=128, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    five = T.rcnn_targets(props, gt_list, lab_list, assigner, mk(), keys=keys)
    six = T.rcnn_targets(props, gt_list, lab_list, assigner, mk(), keys=keys, return_gt_inds=True)
    assert len(five) == 5 and len(six) == 6
    for a, b in zip(five, six):
        assert a.dtype == b.dtype and R.same_bits(a.numpy(), b.numpy())
    pos_gt = six[5]
    assert pos_gt.dtype == torch.int32 and tuple(pos_gt.shape) == (3 * 128,)
    want = np.full((3, 128), -1, np.int64)
    for b in range(3):
        n, g = p["starts"][b + 1] - p["starts"][b], p["gt_starts"][b + 1] - p["gt_starts"][b]
        for s in range(128):
            row = int(e["sel"][b, s])
            if 0 <= row < n and 0 < int(e["gt_inds"][b, row]) <= g:
                want[b, s] = p["gt_starts"][b] + int(e["gt_inds"][b, row]) - 1
    assert np.array_equal(pos_gt.numpy().reshape(3, 128), want) and (want >= 0).any() and (want < 0).any()
    gts, glab = np.asarray(p["gts"]), np.asarray(p["gt_labels"])
    posm = want.reshape(-1) >= 0
    assert np.array_equal(six[1].numpy()[posm], glab[want.reshape(-1)[posm]])      # a positive slot carries its ground truth's label
    assert (six[1].numpy()[~posm] == 65).all()


# ------------------------------------------------------------------------------------------------ the bounds are not vacuous
def test_the_bounds_reject_planted_errors():
    c = R.target_case("small")
    wrong = R.target_vec(c["rois"], c["gt_rows"], c["masks"], c["M"], plant="neighbour_plane")
    assert not R.inside(wrong["t"], c["ref"]["t"], c["ref"]["bound"])[0]
    assert not R.binary_check(R.binarize(wrong["t"]), c["ref"]["t"], c["ref"]["bound"], 0.5)[0]
    d = R.dyadic_case(14)
    assert d["ref"]["exact"] and R.binary_target_ok(d["ref"], R.binarize(d["ref"]["t"]))
    assert not R.binary_target_ok(d["ref"], R.binarize(d["ref"]["t"], tie_to_one=False))                               # > instead of >= at the tie
    lc = R.loss_case("R7_C1")
    good, bad = R.loss_ref(lc), R.loss_ref(lc, plant="row_count")
    assert not R.inside(bad["out"][0], good["out"][0], good["out_bound"][0])[0]
    assert not R.inside(bad["dpred"], good["dpred"], good["dpred_bound"])[0]
    pc = R.paste_case("m28")
    off = R.paste_ref(pc["logits"], pc["labels"], pc["boxes"], pc["img_h"], pc["img_w"], plant="no_half")
    assert not R.inside(off["v"], pc["ref"]["v"], pc["ref"]["bound"])[0]
    assert not R.binary_check((off["v"] >= 0.5).astype(np.uint8), pc["ref"]["v"], pc["ref"]["bound"], 0.5)[0]
