"""`-m gpu`: the detector's training targets on the MI355X (csa_assign / csa_sample / csa_targets, HipOps.assign / sample / bbox_targets,
DESIGN.md §3.15).

Every case of tests/_assign_ref.CASES through the three entry points against the float32 numpy restatement: gt_inds, flags, sel, counts,
labels and all weights equal; max_overlaps, the dx / dy targets and rois bit for bit -- every operation on that path is an IEEE operation
with a stated order, so no tolerance applies.  dw / dh against the restatement's float64 value inside the per-element bound derived in
its docstring (the device logf is not the host's); exactly (0 - mean) / std where gwh == pwh.  Shapes sit around this layout's
boundaries (det_assign.hip): 64 lanes, 256 boxes per workgroup of the IoU passes, 1024 rows per round of the sampler's ordered take, all
ground truths of an image in LDS (up to 1024; 257 crosses the 256-thread staging loop).  Outputs are handed in poisoned, so an element
the kernels leave unwritten fails the comparison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _assign_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keys(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy()).cuda()


def _tab(t):
    return None if t is None else torch.tensor(t, dtype=torch.int32, device="cuda")


def _poison(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    return torch.full(shape, 0x5A, dtype=dtype, device="cuda")


def _targets_out(B, S, compact):
    out = (_poison((B, S), torch.int32), _poison((B, S), torch.float32), _poison((B, S, 4), torch.float32), _poison((B, S, 4), torch.float32))
    return ((_poison((B, S, 5), torch.float32),) + out) if compact else out


def _assign(hip, c):
    a = c["assigner"]
    B, Nmax = c["B"], c["Nmax"]
    out = (_poison((B, Nmax), torch.int32), _poison((B, Nmax), torch.float32))
    return hip.assign(_dev(c["boxes"]), _tab(c["starts"]), _dev(c["gts"]), _tab(c["gt_starts"]), B, Nmax, c["Gmax"], a["pos"], a["neg"],
                      a["min_pos"], a["mlq"], a["all"], a["prefix"], _dev(c["valid"]), out=out)


def _sample(hip, gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, ub):
    B, Nmax = gt_inds.shape
    out = (_poison((B, Nmax), torch.uint8), _poison((B, num), torch.int32), _poison((B, 2), torch.int32))
    return hip.sample(gt_inds, keys, _tab(starts), K, _tab(gt_starts), Gtot, Gmax, num, expected_pos, ub, out=out)


def _targets(hip, c, gt_inds, flags=None, sel=None):
    S = c["Nmax"] if sel is None else sel.shape[1]
    return hip.bbox_targets(_dev(c["boxes"]), _tab(c["starts"]), _dev(c["gts"]), _dev(c["gt_labels"]), _tab(c["gt_starts"]), c["Gmax"], gt_inds,
                            flags, sel, c["means"], c["stds"], c["bg_label"], out=_targets_out(c["B"], S, sel is not None))


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _ints(name, got, want):
    got = _np(got)
    assert got.shape == want.shape, name
    bad = np.argwhere(got.astype(np.int64) != want.astype(np.int64))
    assert len(bad) == 0, f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _bits(name, got, want):
    got = _np(got)
    assert got.shape == want.shape, name
    ok = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    bad = np.argwhere(~ok)
    assert len(bad) == 0, f"{name}: {len(bad)} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def _check_targets(name, got, want, compact):
    """-> the worst |device - T64| / bound over the dw, dh of the positives (0 when there are none)"""
    keys = (("rois",) if compact else ()) + ("labels", "label_weights", "bbox_targets", "bbox_weights")
    got = dict(zip(keys, got))
    _ints(f"{name} labels", got["labels"], want["labels"])
    _bits(f"{name} label_weights", got["label_weights"], want["label_weights"])
    _bits(f"{name} bbox_weights", got["bbox_weights"], want["bbox_weights"])
    if compact:
        _bits(f"{name} rois", got["rois"], want["rois"])
    bt, ref = got["bbox_targets"].cpu().numpy(), want["bbox_targets"]
    _bits(f"{name} dx dy", np.ascontiguousarray(bt[..., :2]), np.ascontiguousarray(ref[..., :2]))
    pos = want["pos"]
    _bits(f"{name} dw dh off the positives", np.ascontiguousarray(bt[..., 2:][~pos]), np.zeros_like(bt[..., 2:][~pos]))
    worst = 0.0
    if pos.any():
        d, t64, bound = bt[..., 2:][pos].astype(np.float64), want["t64"][..., 2:][pos], want["bound"][..., 2:][pos]
        finite = np.isfinite(t64)
        assert np.array_equal(d[~finite], t64[~finite], equal_nan=True), f"{name}: non-finite dw / dh differ"
        err = np.abs(d[finite] - t64[finite])
        assert np.all(err <= bound[finite]), f"{name}: dw / dh outside the bound, worst {float((err / np.maximum(bound[finite], 1e-300)).max()):.3f} of it"
        if bound[finite].size and (bound[finite] > 0).any():
            nz = bound[finite] > 0
            worst = float((err[nz] / bound[finite][nz]).max())
    # gwh == pwh: the ratio is 1, logf(1) = 0, and the target is exactly (0 - mean) / std -- the restatement's fp32 value
    unit = want["unit"]
    assert R.same_float_bits(bt[unit], ref[unit]), f"{name}: gwh == pwh must give exactly (0 - mean) / std"
    return worst


@pytest.mark.parametrize("name", list(R.CASES))
def test_pipeline_equals_the_restatement(hip, name):
    c, e = R.build_case(name), R.expected(name)
    gt_inds, max_ov = _assign(hip, c)
    _ints("gt_inds", gt_inds, e["gt_inds"])
    _bits("max_overlaps", max_ov, e["max_overlaps"])
    flags, sel, counts = _sample(hip, gt_inds, _keys(c["keys"]), c["starts"], len(c["boxes"]), c["gt_starts"], len(c["gts"]), c["Gmax"], c["num"],
                                 c["expected_pos"], c["ub"])
    _ints("flags", flags, e["flags"])
    _ints("sel", sel, e["sel"])
    _ints("counts", counts, e["counts"])
    w1 = _check_targets("dense", _targets(hip, c, gt_inds, flags=flags), e["dense"], False)
    w2 = _check_targets("compact", _targets(hip, c, gt_inds, sel=sel), e["compact"], True)
    print(f"{name}: counts {e['counts'].tolist()}, worst dw/dh error = {max(w1, w2):.3f} of the bound")


def test_prefix_rows_have_unit_ratio_targets(hip):
    """gt_prefix rows sampled as positives are their own ground truth: gwh == pwh, so dw, dh are exactly (0 - mean) / std = 0 / 0.2."""
    c, e = R.build_case("prefix_b3"), R.expected("prefix_b3")
    sel = e["sel"]
    own = [(b, t) for b in range(c["B"]) for t in range(sel.shape[1])
           if 0 <= sel[b, t] < c["gt_starts"][b + 1] - c["gt_starts"][b] and e["compact"]["pos"][b, t]]
    assert len(own) == 4                                                    # of the 32 + 32 sampled positives of this seeded case
    got = _targets(hip, c, _dev(e["gt_inds"]), sel=_dev(sel))[3].cpu().numpy()
    for b, t in own:
        assert got[b, t].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("name", list(R.sample_cases()))
def test_sampler_on_hand_made_pools(hip, name):
    s = R.sample_cases()[name]
    n = s["gt_inds"].shape[1]
    want = R.sample(s["gt_inds"], s["keys"], None, n, s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"])
    got = _sample(hip, _dev(s["gt_inds"]), _keys(s["keys"]), None, n, s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"])
    print(f"{name}: counts {want[2].tolist()}")
    for g, w, key in zip(got, want, ("flags", "sel", "counts")):
        _ints(f"{name} {key}", g, w)


def test_targets_range_check_gt_inds_and_sel(hip):
    """gt_inds / sel / flags straight from a hostile caller: values outside [-1, G_b] count as -1, rows outside the image are padding."""
    c = R.build_case("starts_b3")
    rng = np.random.default_rng(9)
    B, Nmax = c["B"], c["Nmax"]
    gt_inds = rng.integers(-3, 70, size=(B, Nmax)).astype(np.int32)
    gt_inds[:, ::5] = 1 << 30
    gt_inds[:, 1::9] = -(1 << 31)
    flags = rng.integers(0, 3, size=(B, Nmax)).astype(np.uint8)
    flags[:, ::13] = 200
    sel = rng.integers(-2, Nmax + 50, size=(B, 96)).astype(np.int32)
    sel[:, ::7] = 1 << 30
    sel[:, 1::7] = -(1 << 31)
    _check_targets("dense", _targets(hip, c, _dev(gt_inds), flags=_dev(flags)), R.targets(c, gt_inds, flags=flags), False)
    _check_targets("compact", _targets(hip, c, _dev(gt_inds), sel=_dev(sel)), R.targets(c, gt_inds, sel=sel), True)


def test_two_launches_give_equal_bits(hip):
    for name in ("shared_b3", "starts_b3", "anchors64"):
        c = R.build_case(name)
        runs = []
        for _ in range(2):
            gi, mo = _assign(hip, c)
            fl, sel, cnt = _sample(hip, gi, _keys(c["keys"]), c["starts"], len(c["boxes"]), c["gt_starts"], len(c["gts"]), c["Gmax"], c["num"],
                                   c["expected_pos"], c["ub"])
            outs = [gi, mo, fl, sel, cnt, *_targets(hip, c, gi, flags=fl), *_targets(hip, c, gi, sel=sel)]
            torch.cuda.synchronize()
            runs.append([t.cpu().numpy() for t in outs])
        for x, y in zip(*runs):
            assert x.tobytes() == y.tobytes(), name


def test_module_routes_cuda_tensors_to_the_kernels(hip, monkeypatch):
    """det_targets.rpn_targets / rcnn_targets on CUDA tensors call HipOps (no quiet torch route) and give the restatement's outputs."""
    from clipself_amd import det_targets as T
    calls = []
    for m in ("assign", "sample", "bbox_targets"):
        real = getattr(type(hip), m)
        monkeypatch.setattr(type(hip), m, (lambda real, m: lambda self, *a, **k: (calls.append(m), real(self, *a, **k))[1])(real, m))
    c, e = R.build_case("anchors64"), R.expected("anchors64")
    gt_list = [_dev(c["gts"][c["gt_starts"][b]:c["gt_starts"][b + 1]]) for b in range(3)]
    rpn = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1)
    out = T.rpn_targets(_dev(c["boxes"]), _dev(c["valid"]), gt_list, T.MaxIoUAssigner(**rpn), T.RandomSampler(256, 0.5, -1, False), keys=_keys(c["keys"]), ops=hip)
    assert calls == ["assign", "sample", "bbox_targets"] and out[4].is_cuda and out[4].dim() == 0 and int(out[4]) == int(e["counts"].sum())
    _check_targets("rpn_targets", out[:4], e["dense"], False)
    p, e = R.build_case("prefix_b3"), R.expected("prefix_b3")
    props, gts, labs = [], [], []
    for b in range(3):
        gs, ge = p["gt_starts"][b], p["gt_starts"][b + 1]
        gts.append(_dev(p["gts"][gs:ge]))
        labs.append(_dev(p["gt_labels"][gs:ge]))
        props.append(_dev(p["boxes"][p["starts"][b] + (ge - gs):p["starts"][b + 1]]))
    rcnn = dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1)
    out = T.rcnn_targets(props, gts, labs, T.MaxIoUAssigner(**rcnn), T.RandomSampler(128, 0.25, -1, True), keys=_keys(p["keys"]), ops=hip)
    assert calls == ["assign", "sample", "bbox_targets"] * 2 and out[0].shape == (384, 5)
    shaped = (out[0].view(3, 128, 5), out[1].view(3, 128), out[2].view(3, 128), out[3].view(3, 128, 4), out[4].view(3, 128, 4))
    _check_targets("rcnn_targets", shaped, e["compact"], True)
    # the per-image mmdet forms on the device: the same decisions as on the CPU
    n, g = p["starts"][1], p["gt_starts"][1]
    res = T.MaxIoUAssigner(**rcnn).assign(_dev(p["boxes"][g:n]), gts[0], None, labs[0].long())
    cpu = T.MaxIoUAssigner(**rcnn).assign(torch.from_numpy(p["boxes"][g:n].copy()), gts[0].cpu(), None, labs[0].long().cpu())
    assert res.gt_inds.is_cuda and torch.equal(res.gt_inds.cpu(), cpu.gt_inds) and torch.equal(res.max_overlaps.cpu(), cpu.max_overlaps)
    k = T.random_keys((1, n), "cuda", torch.Generator(device="cuda").manual_seed(4))
    s_dev = T.RandomSampler(128, 0.25, -1, True).sample(res, _dev(p["boxes"][g:n]), gts[0], labs[0].long(), keys=k)
    s_cpu = T.RandomSampler(128, 0.25, -1, True).sample(cpu, torch.from_numpy(p["boxes"][g:n].copy()), gts[0].cpu(), labs[0].long().cpu(), keys=k.cpu())
    assert torch.equal(s_dev.pos_inds.cpu(), s_cpu.pos_inds) and torch.equal(s_dev.neg_inds.cpu(), s_cpu.neg_inds)
    assert torch.equal(s_dev.pos_gt_bboxes.cpu(), s_cpu.pos_gt_bboxes) and torch.equal(s_dev.pos_gt_labels.cpu(), s_cpu.pos_gt_labels)


def test_wrappers_check_shapes_dtypes_and_limits(hip):
    boxes, gts = torch.zeros(10, 4, device="cuda"), torch.zeros(2, 4, device="cuda")
    gs = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    for bad in (dict(boxes=boxes.double()), dict(boxes=torch.zeros(10, 5, device="cuda")), dict(gt_starts=gs.long()), dict(Gmax=1025),
                dict(Nmax=(1 << 20) + 1), dict(valid=torch.ones(10, device="cuda")), dict(starts=torch.tensor([0, 10, 10], dtype=torch.int32, device="cuda"))):
        kw = dict(boxes=boxes, starts=None, gt_boxes=gts, gt_starts=gs, B=1, Nmax=10, Gmax=2, pos_iou_thr=0.5, neg_iou_thr=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.assign(**kw)
    with pytest.raises(RuntimeError):
        hip.assign(boxes.cpu(), None, gts, gs, 1, 10, 2, 0.5, 0.5)
    gi = torch.zeros(1, 10, dtype=torch.int32, device="cuda")
    keys = torch.zeros(1, 10, dtype=torch.int32, device="cuda")
    for bad in (dict(num=0), dict(num=4097), dict(expected_pos=9, num=8), dict(keys=keys.float()), dict(keys=keys[:, :5]), dict(gt_starts=None)):
        kw = dict(gt_inds=gi, keys=keys, starts=None, K=10, gt_starts=gs, Gtot=2, Gmax=2, num=8, expected_pos=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.sample(**kw)
    with pytest.raises(ValueError):
        hip.bbox_targets(boxes, None, gts, None, gs, 2, gi)                 # neither flags nor sel
    with pytest.raises(ValueError):
        hip.bbox_targets(boxes, None, gts, None, gs, 2, gi, sel=torch.zeros(1, 4, dtype=torch.int32, device="cuda"), pos_weight=1.0)
    assert hip.assign_workspace(1, 10, 2) >= 256 and hip.assign_workspace(1, 10, 1025) == 0
