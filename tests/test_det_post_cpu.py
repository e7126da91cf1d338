"""CPU: detector post-processing (clipself_amd/det_post.py, include/clipself_det.h) without a GPU.

Known answers of the contract; per-list NMS on un-offset boxes against mmcv's offset formulation in float64; the torch route against
the numpy restatement (tests/_nms_ref.py) on every case of the GPU list with at most 130 boxes per image -- indices, labels, counts,
padding and bit-equal dets; delta2bbox inside the bound derived from its rounding count; every -1 case of the header through the raw entry
points; the mmcv / mmdet call signatures and return shapes.  (The header itself is held by tests/test_cabi_symbols.py.)"""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _nms_ref as R

NAN, INF = float("nan"), float("inf")
SMALL = [n for n, sp in R.NMS_CASES.items() if max(sp["ns"]) <= 130]


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))


def _nms(boxes, scores, iou_thr=0.5, score_thr=0.0, max_num=10, group=None, G=0, starts=None):
    """The torch route on one image (or `starts`) -> (inds, labels) of the kept rows as lists, and the raw outputs."""
    from clipself_amd import det_post
    boxes, scores = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), torch.tensor(scores, dtype=torch.float32)
    if scores.dim() == 1:
        scores = scores[:, None]
    K = boxes.shape[0]
    out = det_post.nms_torch(boxes, scores, starts or [0, K], K, score_thr, iou_thr, max_num,
                             None if group is None else torch.tensor(group, dtype=torch.int32), G)
    m = int(out[3][0])
    return out[2][0, :m].tolist(), out[1][0, :m].tolist(), out


# ------------------------------------------------------------------------------------------------ known answers
def test_two_identical_boxes_the_lower_score_goes():
    inds, _, _ = _nms([[0, 0, 10, 10], [0, 0, 10, 10]], [0.6, 0.9])
    assert inds == [1]


def test_iou_exactly_at_the_threshold_is_kept():
    """2 x 1 and 1 x 2 ... here a 3 x 1 pair: [0,3]x[0,1] and [1,4]x[0,1] have inter = 2, union = 4, iou = 0.5 exactly -- not > 0.5."""
    boxes = [[0, 0, 3, 1], [1, 0, 4, 1]]
    assert float(R.iou_matrix(np.array(boxes, np.float32))[0, 1]) == 0.5
    assert _nms(boxes, [0.9, 0.8], iou_thr=0.5)[0] == [0, 1]
    assert _nms(boxes, [0.9, 0.8], iou_thr=0.49)[0] == [0]
    boxes = [[0, 0, 2, 1], [1, 0, 2, 2]]                                    # 2 x 1 and 1 x 2: inter 1, union 3
    assert _nms(boxes, [0.9, 0.8], iou_thr=0.3)[0] == [0] and _nms(boxes, [0.9, 0.8], iou_thr=0.34)[0] == [0, 1]


def test_nested_box():
    boxes = [[0, 0, 10, 10], [2, 2, 8, 8]]                                  # iou = 36 / 100
    assert _nms(boxes, [0.9, 0.8], iou_thr=0.35)[0] == [0]
    assert _nms(boxes, [0.9, 0.8], iou_thr=0.36)[0] == [0, 1]
    assert _nms(boxes, [0.8, 0.9], iou_thr=0.35)[0] == [1]


def test_zero_area_box_neither_suppresses_nor_is_suppressed():
    boxes = [[5, 5, 5, 9], [0, 0, 10, 10], [5, 5, 5, 9]]                    # zero width, inside the big box, and twice: 0 / 0
    assert _nms(boxes, [0.9, 0.8, 0.7], iou_thr=0.0)[0] == [0, 1, 2]


def test_nan_score_is_dropped_nan_coordinates_are_kept_and_harmless():
    boxes = [[0, 0, 10, 10], [NAN, 0, 10, 10], [0, 0, 10, 10], [-INF, -INF, INF, INF], [1, 1, 9, 9]]
    inds, _, out = _nms(boxes, [0.9, 0.95, NAN, 0.97, 0.5], iou_thr=0.5)
    assert inds == [3, 1, 0]                                                # row 2 (NaN score) never a candidate; row 4 goes to row 0 only
    assert torch.isnan(out[0][0, 1, 0]) and out[0][0, 1, 4] == torch.tensor(0.95)


def test_equal_scores_the_lower_row_wins():
    boxes = [[0, 0, 10, 10]] * 3 + [[20, 20, 30, 30]] * 2
    assert _nms(boxes, [0.5] * 5)[0] == [0, 3]
    # the cut: equal scores across classes go by the flat index k * C + c
    inds, labels, _ = _nms([[0, 0, 10, 10], [20, 20, 30, 30]], [[0.5, 0.5], [0.5, 0.5]], max_num=3)
    assert list(zip(inds, labels)) == [(0, 0), (0, 1), (1, 0)]


def test_score_threshold_is_strict_and_the_background_column_is_ignored():
    from clipself_amd import det_post
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert _nms([[0, 0, 10, 10], [20, 20, 30, 30]], [0.5, above], score_thr=0.5)[0] == [1]
    boxes = torch.tensor([[0., 0, 10, 10], [20, 20, 30, 30]])
    scores = torch.tensor([[0.2, 0.1, 0.99], [0.05, 0.6, 0.99]])            # the last column is the background
    dets, labels = det_post.multiclass_nms(boxes, scores, 0.07, dict(type="nms", iou_threshold=0.5), 10)
    assert labels.tolist() == [1, 0, 1] and dets[:, 4].tolist() == pytest.approx([0.6, 0.2, 0.1])
    assert torch.equal(dets[:, :4], boxes[[1, 0, 0]])


def test_padding_and_empty_inputs():
    _, _, (dets, labels, inds, counts) = _nms([[0, 0, 10, 10]], [0.9], max_num=4)
    assert counts.tolist() == [1] and labels[0].tolist() == [0, -1, -1, -1] and inds[0].tolist() == [0, -1, -1, -1]
    assert bool((dets[0, 1:] == 0).all())
    _, _, (dets, labels, inds, counts) = _nms(np.zeros((0, 4)), np.zeros((0, 3)), max_num=4)
    assert counts.tolist() == [0] and bool((labels == -1).all()) and bool((inds == -1).all()) and bool((dets == 0).all())
    _, _, out = _nms([[0, 0, 10, 10]] * 3, [0.9, 0.8, 0.7], starts=[0, 3, 1, 3], max_num=2)        # non-monotone starts: an empty image
    assert out[3].tolist() == [1, 0, 1] and out[2][:, 0].tolist() == [0, -1, 1]


def test_group_form_keeps_lists_apart_and_drops_ids_out_of_range():
    boxes = [[0, 0, 10, 10]] * 4
    inds, labels, _ = _nms(boxes, [0.9, 0.8, 0.7, 0.6], group=[1, 1, 0, 2], G=2)
    assert inds == [0, 2] and labels == [1, 0]                              # row 1 suppressed inside group 1, row 3 (group 2 of 2) dropped
    from clipself_amd import det_post
    with pytest.raises(ValueError):
        det_post.nms_torch(torch.zeros(2, 4), torch.zeros(2, 2), [0, 2], 2, 0.0, 0.5, 4, torch.zeros(2, dtype=torch.int32), 1)


# ------------------------------------------------------------------------------------------------ the algorithm is the reference's
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("iou_thr", [0.4, 0.5, 0.7])
def test_per_list_nms_equals_mmcvs_offset_formulation(seed, iou_thr):
    """mmcv shifts the boxes of class c by c * (max coordinate + 1) and runs one NMS; this project runs one NMS per class on the
    un-offset boxes.  In float64 on lattice inputs (every quantity exact on both sides) the kept sets and their order agree."""
    K, C = 130, 5
    boxes = R.lattice_boxes(K, seed)
    r = np.random.RandomState(seed + 50)
    scores, idxs = r.rand(K).astype(np.float32), r.randint(0, C, K)
    want = R.batched_nms_offset(boxes, scores, idxs, iou_thr, np.float64)
    got = []
    for c in range(C):
        rows = np.nonzero(idxs == c)[0]
        got += [int(rows[j]) for j in R.greedy_nms(boxes[rows], scores[rows], iou_thr, np.float64)]
    got.sort(key=lambda k: (-float(scores[k]), k))
    assert got == want
    d, l, i, c = R.multiclass(boxes, scores[:, None], [0, K], K, -INF, iou_thr, K, idxs.astype(np.int32), C, np.float64)
    assert i[0, :c[0]].tolist() == want and l[0, :c[0]].tolist() == idxs[want].tolist()


# ------------------------------------------------------------------------------------------------ the torch route is the restatement
@pytest.mark.parametrize("name", SMALL)
def test_torch_route_equals_the_restatement(name):
    from clipself_amd import det_post
    c = R.build_case(name)
    if not R.NMS_CASES[name].get("lattice", True):
        for b in range(len(c["starts"]) - 1):
            assert R.min_iou_margin(c["boxes"][c["starts"][b]:c["starts"][b + 1]], c["iou_thr"]) > 1e-5
    got = det_post.nms(_t(c["boxes"]), _t(c["scores"]), c["starts"].tolist(), c["Kmax"], c["score_thr"], c["iou_thr"], c["max_num"],
                       _t(c["group"]), c["G"])
    R.compare(name, [g.numpy() for g in got])
    B, mx = len(c["starts"]) - 1, c["max_num"]
    assert got[0].shape == (B, mx, 5) and got[1].shape == (B, mx) and got[2].shape == (B, mx) and got[3].shape == (B,)
    assert got[1].dtype == got[2].dtype == got[3].dtype == torch.int32


def test_per_class_boxes_take_the_torch_route():
    """multi_bboxes [n, 4 * C]: list (image, c) runs on boxes[:, c] -- equal to C single-class problems."""
    from clipself_amd import det_post
    n, C = 65, 3
    boxes = np.stack([R.lattice_boxes(n, 30 + c) for c in range(C)], 1)                    # [n, C, 4]
    scores = R.scores_matrix(n, C + 1, 3)
    dets, labels, flat = det_post.multiclass_nms(_t(boxes.reshape(n, 4 * C)), _t(scores), 0.3, dict(type="nms", iou_threshold=0.5), 40,
                                                 return_inds=True)
    want = []
    for c in range(C):
        rows = np.nonzero(scores[:, c] > np.float32(0.3))[0]
        want += [(float(scores[rows[j], c]), int(rows[j]) * C + c) for j in R.greedy_nms(boxes[rows, c], scores[rows, c], 0.5)]
    want.sort(key=lambda t: (-t[0], t[1]))
    want = want[:40]
    assert flat.tolist() == [f for _, f in want] and labels.tolist() == [f % C for _, f in want]
    assert np.array_equal(dets[:, :4].numpy(), boxes.reshape(-1, 4)[[f for _, f in want]])


# ------------------------------------------------------------------------------------------------ delta2bbox
def _d2b_case(K=130, seed=3, B=3):
    rois, deltas = R.delta2bbox_inputs(K, seed)
    starts = [0, K // 3, K // 3, K] if B == 3 else [0, K]
    max_shape = [[480.0, 512.0], [300.0, 200.0], [512.0, 333.0]][:B]
    scale = [[1.5, 1.25, 1.5, 1.25], [0.7, 0.7, 0.7, 0.7], [1.6180340051651, 0.3, 1.6180340051651, 0.3]][:B]
    return rois, deltas, starts, max_shape, scale


@pytest.mark.parametrize("form", ["plain", "clip", "clip+scale"])
def test_delta2bbox_torch_route_within_the_derived_bound(form):
    from clipself_amd import det_post
    rois, deltas, starts, max_shape, scale = _d2b_case()
    means, stds = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
    kw = dict(starts=starts, max_shape=max_shape if form != "plain" else None, scale=scale if form == "clip+scale" else None)
    want, bound = R.delta2bbox(rois, deltas, means, stds, 16 / 1000, **kw)
    got = det_post.delta2bbox_torch(_t(rois), _t(deltas), means, stds, 16 / 1000, **kw).double().numpy()
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
    print(f"delta2bbox torch route [{form}]: worst err / bound {ratio.max():.3f}")
    assert got.shape == (len(rois), 4) and bool((np.abs(got - want) <= bound).all()), f"worst err / bound {ratio.max():.3f}"
    # the clamp rows: width = pw * exp(+-|log(16 / 1000)|) = pw * 62.5 and pw / 62.5 before the border clamp
    if form == "plain":
        pw = rois[:2, 2] - rois[:2, 0]
        assert np.allclose(got[:2, 2] - got[:2, 0], pw * np.array([62.5, 1 / 62.5]), rtol=1e-5, atol=1e-3)     # corners near 1e3: ulp 6e-5


def test_delta2bbox_keeps_mmdets_signature_and_clips_to_the_image():
    from clipself_amd import det_post
    assert list(inspect.signature(det_post.delta2bbox).parameters) == ["rois", "deltas", "means", "stds", "max_shape", "wh_ratio_clip"]
    rois, deltas, _, _, _ = _d2b_case(B=1)
    out = det_post.delta2bbox(_t(rois), _t(deltas), (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), max_shape=(300, 200, 3))
    assert out.shape == (len(rois), 4) and float(out[:, [0, 2]].max()) <= 200 and float(out[:, [1, 3]].max()) <= 300 and float(out.min()) >= 0
    assert bool((out[2, :2] == 0).all()) and out[3, 2] == 200 and out[3, 3] == 300      # rows 2 / 3 are pushed across the border
    zero = det_post.delta2bbox(_t(rois), torch.zeros(len(rois), 4))
    assert torch.allclose(zero, _t(rois), atol=1e-4)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_limits_are_refused_without_a_device():
    """Argument checks come before any launch, so the -1 cases can be seen here: no pointer is touched."""
    from clipself_amd import hip
    lib = hip.load_library()
    assert lib.csd_nms_workspace(1, 16385, 1, 10) == 0 and lib.csd_nms_workspace(1, 100, 1, 4097) == 0 and lib.csd_nms_workspace(0, 100, 1, 10) == 0
    assert lib.csd_nms_workspace(2, 130, 3, 100) >= 4 * 2 + 2 * 130 * 3 * 8 + 2 * 3 * 100 * 8

    def call(B=1, C=2, K=10, Kmax=10, max_num=5, ldb=4, lds=2, group=None, G=0, ws=1 << 20):
        return lib.csd_nms(1 << 20, ldb, 1 << 20, lds, C, 1 << 20, group, G, K, B, Kmax, 0.1, 0.5, max_num, 1 << 20, 1 << 20, 1 << 20, 1 << 20, ws, None)

    for kw, word in [(dict(B=0), b"B ="), (dict(C=0, lds=0), b"C ="), (dict(K=-1), b"K ="), (dict(Kmax=16385), b"Kmax"),
                     (dict(Kmax=16384, C=1 << 17, lds=1 << 17), b"Kmax * C"), (dict(max_num=0), b"max_num"), (dict(max_num=4097), b"max_num"),
                     (dict(ldb=3), b"ldb"), (dict(lds=1), b"lds"), (dict(group=1 << 20, G=5), b"group"), (dict(ws=None), b"workspace")]:
        assert call(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())


# ------------------------------------------------------------------------------------------------ mmcv / mmdet call signatures
def test_mmcv_and_mmdet_signatures_and_return_shapes():
    from clipself_amd import det_post
    from clipself_amd.ov_head import OpenVocabBoxScores
    assert list(inspect.signature(det_post.batched_nms).parameters) == ["boxes", "scores", "idxs", "nms_cfg", "class_agnostic"]
    p = list(inspect.signature(det_post.multiclass_nms).parameters)
    assert p[:5] == ["multi_bboxes", "multi_scores", "score_thr", "nms_cfg", "max_num"] and "return_inds" in p
    assert inspect.signature(det_post.multiclass_nms).parameters["max_num"].default == -1
    assert list(inspect.signature(OpenVocabBoxScores.get_bboxes).parameters) == \
        ["self", "rois", "cls_score", "bbox_pred", "img_shape", "scale_factor", "rescale", "cfg"]

    c = R.build_case("group_small")
    n = int(c["starts"][1])
    boxes, scores, idxs = _t(c["boxes"][:n]), _t(c["scores"][:n, 0]), _t(c["group"][:n]).clamp(0, 4).long()
    dets, keep = det_post.batched_nms(boxes, scores, idxs, dict(type="nms", iou_threshold=0.7, split_thr=10000))
    want = R.batched_nms_offset(c["boxes"][:n], c["scores"][:n, 0], idxs.numpy(), 0.7, np.float32)
    assert keep.tolist() == want and keep.dtype == torch.int64 and dets.shape == (len(want), 5)
    assert torch.equal(dets[:, :4], boxes[keep]) and torch.equal(dets[:, 4], scores[keep])
    dets2, keep2 = det_post.batched_nms(boxes, scores, idxs, dict(type="nms", iou_threshold=0.7, max_num=7))
    assert keep2.tolist() == want[:7]
    dets3, keep3 = det_post.batched_nms(boxes, scores, idxs, dict(iou_threshold=0.7), class_agnostic=True)
    assert keep3.tolist() == R.greedy_nms(c["boxes"][:n], c["scores"][:n, 0], 0.7)
    for bad in (dict(type="soft_nms", iou_threshold=0.5), dict(type="nms", iou_threshold=0.5, offset=1), dict(type="nms")):
        with pytest.raises(ValueError):
            det_post.batched_nms(boxes, scores, idxs, bad)
    d0, k0 = det_post.batched_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.long), dict(iou_threshold=0.5))
    assert d0.shape == (0, 5) and k0.shape == (0,)
    out = det_post.multiclass_nms(boxes, torch.rand(n, 4, generator=torch.Generator().manual_seed(1)), 0.05, dict(type="nms", iou_threshold=0.5), 30, return_inds=True)
    assert out[0].shape == (30, 5) and out[1].shape == (30,) and out[2].shape == (30,) and out[1].dtype == torch.int64
    assert torch.equal(out[2] % 3, out[1])


def test_get_bboxes_follows_the_reference():
    from clipself_amd import det_post
    from clipself_amd.ov_head import OpenVocabBoxScores
    from oracle.ops_ref import RefOps
    g = torch.Generator().manual_seed(7)
    head = OpenVocabBoxScores(torch.randn(6, 16, generator=g), ops=RefOps()).eval()
    assert head.target_means == (0., 0., 0., 0.) and head.target_stds == (0.1, 0.1, 0.2, 0.2) and head.reg_class_agnostic is True
    rois_np, deltas_np = R.delta2bbox_inputs(40, 11, side=256.0)
    rois = torch.cat([torch.zeros(40, 1), _t(rois_np)], 1)
    deltas, scores = _t(deltas_np) * 0.3, torch.rand(40, 6, generator=g)
    bboxes, out_scores = head.get_bboxes(rois, scores, deltas, (256, 200, 3), (2.0, 2.0, 2.0, 2.0), rescale=True, cfg=None)
    assert out_scores is scores and bboxes.shape == (40, 4)                 # cfg None: (bboxes, scores), as the reference
    want = det_post.delta2bbox(rois[:, 1:], deltas, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), max_shape=(256, 200, 3)) / 2.0
    assert torch.equal(bboxes, want)
    plain, _ = head.get_bboxes(rois, scores, None, (256, 200, 3), 2.0, rescale=False)
    assert torch.equal(plain, rois[:, 1:])                                  # no bbox_pred: the rois (the reference's clamp_ hits a copy)
    cfg = SimpleNamespace(score_thr=0.2, nms=dict(type="nms", iou_threshold=0.5), max_per_img=15)
    det_bboxes, det_labels = head.get_bboxes(rois, scores, deltas, (256, 200, 3), (2.0, 2.0, 2.0, 2.0), rescale=True, cfg=cfg)
    wd, wl, wi, wc = R.multiclass(bboxes.numpy(), scores[:, :5].numpy(), [0, 40], 40, 0.2, 0.5, 15)
    assert det_bboxes.shape == (int(wc[0]), 5) and det_labels.tolist() == wl[0, :wc[0]].tolist()
    assert np.array_equal(det_bboxes.numpy(), wd[0, :wc[0]])
    # the batched form gives the same detections for the same image
    dets, labels, inds, counts = det_post.detections(rois, scores, deltas, [(256, 200, 3)], [(2.0, 2.0, 2.0, 2.0)], 0.2, 0.5, 15)
    assert counts.tolist() == [int(wc[0])] and np.array_equal(dets.numpy(), wd) and np.array_equal(inds.numpy(), wi)
