"""CPU: RPN proposals (clipself_amd/det_proposals.py, include/clipself_rpn.h) without a GPU.

The torch route (`select_torch`, `rpn_proposals` on CPU tensors) against the numpy restatement (tests/_proposal_ref.py) on every case of the
GPU list: exact anchor indices, starts and decided groups, scores and boxes inside their derived bounds, end-to-end proposals bit-equal;
every -1 case of the header through the raw entry point (the header itself is held by tests/test_cabi_symbols.py) (argument checks come before any launch); cfg validation; `rcnn_targets(proposal_counts=)`; the conditions the GPU
tests rely on, asserted from the restatement alone (no row in the min-size band, score gaps of the end-to-end cases above four bounds);
and the bounds rejecting six planted errors."""
import ctypes

import numpy as np
import pytest
import torch

import _proposal_ref as P

ALL = list(P.SELECT_CASES) + list(P.E2E_CASES)


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))


def _select_torch(c):
    from clipself_amd import det_proposals
    out = det_proposals.select([_t(x) for x in c["cls"]], [_t(x) for x in c["reg"]], _t(c["anchors"]), _t(c["max_shape"]), c["nms_pre"], c["means"],
                               c["stds"], c["wh_ratio_clip"], c["min_bbox_size"])
    return [o.numpy() for o in out]


def _cfg(c, sp):
    return dict(nms_pre=c["nms_pre"], max_per_img=sp["max_per_img"], nms=dict(type="nms", iou_threshold=sp["iou"]), min_bbox_size=c["min_bbox_size"])


# ------------------------------------------------------------------------------------------------ the torch route is the restatement
@pytest.mark.parametrize("name", ALL)
def test_select_torch_equals_the_restatement(name):
    c = P.build_case(name)
    got = _select_torch(c)
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32 and got[0].dtype == np.float32
    bad = P.check_select(P.expected(name), got, name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(P.E2E_CASES))
def test_rpn_proposals_on_cpu_tensors_equal_the_restatement(name):
    from clipself_amd import det_proposals
    c, sp = P.build_case(name), P.E2E_CASES[name]
    want = P.rpn_proposals(c, sp["max_per_img"], sp["iou"], P.expected(name))
    got = det_proposals.rpn_proposals([_t(x) for x in c["cls"]], [_t(x) for x in c["reg"]], _t(c["anchors"]), _t(c["max_shape"]), _cfg(c, sp),
                                      c["means"], c["stds"], return_inds=True)
    B = c["cls"][0].shape[0]
    assert got[0].shape == (B, sp["max_per_img"], 5) and got[1].shape == (B,) and got[1].dtype == torch.int32
    bad = P.check_proposals(want, [g.numpy() for g in got], name)
    assert not bad, "\n".join(bad)
    assert int(want[1].min()) > 0
    two = det_proposals.rpn_proposals([_t(x) for x in c["cls"]], [_t(x) for x in c["reg"]], _t(c["anchors"]), _t(c["max_shape"]), _cfg(c, sp))
    assert len(two) == 2 and torch.equal(two[0], got[0])


def test_get_bboxes_returns_mmdets_lists_and_takes_an_anchor_generator():
    from clipself_amd import det_proposals
    from clipself_amd.det_targets import AnchorGenerator
    gen = AnchorGenerator(strides=[4, 8], ratios=[0.5, 1.0, 2.0], scales=[8])
    g = torch.Generator().manual_seed(3)
    sizes = [(12, 10), (6, 5)]
    cls = [(torch.randint(-512, 513, (2, 3, h, w), generator=g) / 64.0).half() for h, w in sizes]       # any float dtype
    reg = [torch.zeros(2, 12, h, w) for h, w in sizes]
    metas = [dict(img_shape=(48, 40, 3)), dict(img_shape=(40, 36, 3))]
    cfg = dict(nms_pre=50, max_per_img=20, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)
    out = det_proposals.get_bboxes(cls, reg, gen, metas, cfg)
    anchors = torch.cat(gen.grid_priors(sizes), 0)
    dets, counts = det_proposals.rpn_proposals(cls, reg, anchors, [(48, 40), (40, 36)], cfg)
    assert len(out) == 2 and [o.shape for o in out] == [(int(n), 5) for n in counts]
    assert all(torch.equal(o, dets[b, :o.shape[0]]) for b, o in enumerate(out)) and int(counts.min()) > 0
    assert float(out[0][:, 2].max()) <= 40 and float(out[0][:, 3].max()) <= 48 and bool((out[0][:-1, 4] >= out[0][1:, 4]).all())
    with pytest.raises(ValueError):
        det_proposals.get_bboxes(cls, reg, gen, metas[:1], cfg)


# ------------------------------------------------------------------------------------------------ the C ABI
def _levels(hip, dims, cls=1 << 20, reg=1 << 20):
    arr = (hip.RpnLevel * len(dims))()
    for l, (h, w) in enumerate(dims):
        arr[l] = hip.RpnLevel(cls, reg, h, w)
    return arr


def test_limits_are_refused_without_a_device():
    """Argument checks come before any launch, so the -1 cases can be seen here: no pointer is touched."""
    from clipself_amd import hip
    lib = hip.load_library()
    two = _levels(hip, [(64, 64), (5, 7)])
    ws = lib.csp_workspace
    assert ws(two, 2, 8, 3, 2000) >= 256 and ws(_levels(hip, [(1, 1)]), 1, 1, 1, 1) >= 256
    assert ws(two, 2, 8, 3, 2000) >= 8 * (3 * 2048 * 4 + 2 * 6 * 4 + 2000 * 8)          # one long level: histograms, chunk counters, keys
    for args in [(two, 0, 8, 3, 2000), (two, 9, 8, 3, 2000), (None, 2, 8, 3, 2000), (two, 2, 0, 3, 2000), (two, 2, 65536, 3, 2000),
                 (two, 2, 8, 0, 2000), (two, 2, 8, 17, 2000), (two, 2, 8, 3, 0), (two, 2, 8, 3, 4097), (_levels(hip, [(513, 4)]), 1, 1, 1, 10),
                 (_levels(hip, [(4, 0)]), 1, 1, 1, 10), (_levels(hip, [(64, 64)] * 5), 5, 1, 3, 4096)]:
        assert ws(*args) == 0, args[1:]
    assert ws(_levels(hip, [(64, 64)] * 4), 4, 1, 3, 4096) >= 256                       # Ktot = 16384 exactly

    f4 = lambda: (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    ptr = 1 << 20

    def call(levels=two, L=2, B=8, A=3, anchors=ptr, lda=4, nms_pre=2000, means=True, stds=True, clip=0.016, max_shape=None, boxes=ptr, scores=ptr,
             group=ptr, inds=None, starts=ptr, wsp=ptr):
        return lib.csp_select(levels, L, B, A, anchors, lda, nms_pre, f4() if means else None, f4() if stds else None, clip, max_shape, 0.0,
                              boxes, scores, group, inds, starts, wsp, None)

    for kw, word in [(dict(L=0), b"L ="), (dict(L=9), b"L ="), (dict(levels=None), b"levels"), (dict(B=0), b"B ="), (dict(B=65536), b"B ="),
                     (dict(A=0), b"A ="), (dict(A=17), b"A ="), (dict(nms_pre=0), b"nms_pre"), (dict(nms_pre=4097), b"nms_pre"),
                     (dict(lda=3), b"lda"), (dict(clip=0.0), b"wh_ratio_clip"),
                     (dict(levels=_levels(hip, [(0, 4)]), L=1), b"h ="), (dict(levels=_levels(hip, [(4, 513)]), L=1), b"w ="),
                     (dict(levels=_levels(hip, [(4, 4)], cls=None), L=1), b"cls and reg"), (dict(levels=_levels(hip, [(4, 4)], reg=None), L=1), b"cls and reg"),
                     (dict(levels=_levels(hip, [(64, 64)] * 5), L=5, nms_pre=4096), b"Ktot"),
                     (dict(anchors=None), b"anchors"), (dict(means=False), b"means"), (dict(stds=False), b"stds"),
                     (dict(boxes=None), b"boxes"), (dict(scores=None), b"scores"), (dict(group=None), b"group"), (dict(starts=None), b"starts"),
                     (dict(wsp=None), b"workspace")]:
        assert call(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())


# ------------------------------------------------------------------------------------------------ cfg
def test_cfg_validation():
    from clipself_amd import det_proposals as D
    good = dict(nms_pre=2000, max_per_img=1000, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)
    assert D.check_cfg(good) == (2000, 1000, 0.7, 0.0)
    assert D.check_cfg(dict(nms_pre=1, max_per_img=4096, nms=dict(iou_threshold=0.5))) == (1, 4096, 0.5, 0.0)
    assert D.check_cfg(dict(good, min_bbox_size=-1))[3] == -1.0
    for bad in (dict(good, nms=dict(type="soft_nms", iou_threshold=0.7)), dict(good, score_thr=0.1), dict(good, nms_thr=0.7), dict(good, max_num=1000),
                dict(good, nms_pre=0), dict(good, nms_pre=-1), dict(good, nms_pre=4097), dict(good, nms_pre=2.5), dict(good, max_per_img=0),
                dict(good, max_per_img=4097), dict(good, nms=dict(type="nms")), dict(good, nms=dict(type="nms", iou_threshold=0.7, offset=1)),
                dict(good, nms=dict(type="nms", iou_threshold=1.5)), dict(good, nms=0.7), dict(good, min_bbox_size=float("nan")),
                {k: v for k, v in good.items() if k != "nms_pre"}, {k: v for k, v in good.items() if k != "max_per_img"},
                {k: v for k, v in good.items() if k != "nms"}, 7):
        with pytest.raises(ValueError):
            D.check_cfg(bad)
    c = P.build_case("g5x7_a3")
    cls, reg = [_t(x) for x in c["cls"]], [_t(x) for x in c["reg"]]
    with pytest.raises(ValueError):
        D.select(cls, reg, _t(c["anchors"][:-1]), None, 20)                                  # N does not match the maps
    with pytest.raises(ValueError):
        D.select(cls, reg[:0], _t(c["anchors"]), None, 20)
    with pytest.raises(ValueError):
        D.select(cls, reg, _t(c["anchors"]), None, 4097)
    with pytest.raises(ValueError):
        D.select(cls, reg, _t(c["anchors"]), [(10, 10)] * 2, 20)                             # two shapes for one image
    with pytest.raises(NotImplementedError):
        D.select(cls, reg, _t(c["anchors"]), None, 20, fused=True)                           # CPU tensors have no kernel route


# ------------------------------------------------------------------------------------------------ rcnn_targets(proposal_counts=)
def _rcnn_inputs(B=3, P_=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, P_, 2, generator=g) * 200
    props = torch.cat([xy, xy + 10 + torch.rand(B, P_, 2, generator=g) * 80], -1)
    counts = torch.tensor([P_, 17, 0], dtype=torch.int32)[:B]
    for b in range(B):
        props[b, int(counts[b]):] = 0                                         # the padding rows of fixed-shape proposals
    gts, labels = [], []
    for b, n in enumerate([3, 2, 4][:B]):
        src = props[b, :n].clone() if int(counts[b]) >= n else torch.tensor([[10., 10, 60, 60]]).repeat(n, 1) + torch.arange(n)[:, None] * 20.0
        gts.append(src + torch.rand(n, 4, generator=g) * 4)
        labels.append(torch.randint(0, 5, (n,), generator=g))
    return props, counts, gts, labels


@pytest.mark.parametrize("add_gt", [True, False])
def test_rcnn_targets_with_proposal_counts_equals_the_list_form(add_gt):
    from clipself_amd import det_targets as T
    props, counts, gts, labels = _rcnn_inputs()
    B, P_ = props.shape[:2]
    assigner = T.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False)
    sampler = T.RandomSampler(num=16, pos_fraction=0.25, add_gt_as_proposals=add_gt)
    gmax = max(len(g) for g in gts) if add_gt else 0
    keys = T.random_keys((B, P_ + gmax), "cpu", torch.Generator().manual_seed(5))
    fixed = T.rcnn_targets(props, gts, labels, assigner, sampler, num_classes=5, keys=keys, return_gt_inds=True, proposal_counts=counts)
    trimmed = [props[b, :int(counts[b])] for b in range(B)]
    nmax = max(t.shape[0] + (len(gts[b]) if add_gt else 0) for b, t in enumerate(trimmed))
    lists = T.rcnn_targets(trimmed, gts, labels, assigner, sampler, num_classes=5, keys=keys[:, :nmax].contiguous(), return_gt_inds=True)
    assert len(fixed) == len(lists) == 6
    for a, b in zip(fixed, lists):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert int((fixed[1] < 5).sum()) > 0                                      # some positives: the comparison is not empty
    # without the keyword: today's output, where the zero rows of the padding are ordinary (negative) proposals
    plain = T.rcnn_targets(props, gts, labels, assigner, sampler, num_classes=5, keys=keys, return_gt_inds=True)
    again = T.rcnn_targets(props, gts, labels, assigner, sampler, num_classes=5, keys=keys, return_gt_inds=True, proposal_counts=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert not all(torch.equal(a, b) for a, b in zip(plain, fixed))           # the padding rows were sampled as negatives there
    with pytest.raises(ValueError):
        T.rcnn_targets(props, gts, labels, assigner, sampler, num_classes=5, keys=keys, proposal_counts=counts[:2])


# ------------------------------------------------------------------------------------------------ conditions the GPU tests rely on
@pytest.mark.parametrize("name", ALL)
def test_no_selected_row_lies_in_the_min_size_band(name):
    s = P.expected(name)
    assert int(s["band"].sum()) == 0, f"{int(s['band'].sum())} of {s['band'].size} rows are undecided: pick another seed"


@pytest.mark.parametrize("name", list(P.E2E_CASES))
def test_end_to_end_cases_are_decidable(name):
    """Lattice logits k / 64: two distinct scores of one image differ by more than four score bounds; the decode is exact (bound 0), so the
    boxes are on the 1/4 lattice and every IoU is one correctly rounded division."""
    c, s = P.build_case(name), P.expected(name)
    for x in c["cls"]:
        assert np.array_equal(x * 64, np.round(x * 64)) and float(np.abs(x).max()) <= 8
    ratio = P.min_score_gap_ratio(s)
    print(f"{name}: smallest score gap / (4 * bound) = {ratio:.2f}")
    assert ratio > 1
    assert float(s["box_bound"].max()) == 0.0
    assert np.array_equal(s["box"] * 4, np.round(s["box"] * 4)) and float(s["box"].min()) >= 0 and float(s["box"].max()) <= 512
    kept = (s["group"] >= 0).sum(1)
    assert int(kept.min()) > P.E2E_CASES[name]["max_per_img"] // 2            # enough boxes reach the NMS


def test_e2e_zero_has_rows_dropped_by_the_filter():
    s = P.expected("e2e_zero")
    assert 0 < int((s["group"] < 0).sum()) < s["group"].size


# ------------------------------------------------------------------------------------------------ the bounds reject planted errors
def _as_got(s):
    return [s["box"].astype(np.float32), s["score"].astype(np.float32), s["group"], s["anchor_inds"], s["starts"]]


def _known_case(min_size=4.0, logits=None):
    """Zero deltas on dyadic anchors: widths 4, 4.25 and 8 against min_bbox_size = 4; one anchor wholly outside the image."""
    anchors = np.array([[8, 8, 12, 40], [16, 8, 20.25, 40], [32, 8, 40, 12], [600, 8, 640, 40], [-8, -8, 20, 20], [40, 40, 48, 48]], np.float32)
    n = len(anchors)
    x = np.zeros((1, 1, 1, n), np.float32) if logits is None else np.asarray(logits, np.float32).reshape(1, 1, 1, n)
    return dict(cls=[x], reg=[np.zeros((1, 4, 1, n), np.float32)], anchors=anchors, max_shape=np.array([[64.0, 512.0]], np.float32), nms_pre=n,
                means=(0.0,) * 4, stds=(1.0,) * 4, wh_ratio_clip=16 / 1000, min_bbox_size=min_size)


def test_known_answers_of_the_restatement_and_the_torch_route():
    c = _known_case()
    s = P.select(c)
    assert float(s["box_bound"].max()) == 0.0 and int(s["band"].sum()) == 0
    assert s["anchor_inds"].tolist() == [[0, 1, 2, 3, 4, 5]]                   # equal logits: by index
    assert s["group"].tolist() == [[-1, 0, -1, -1, 0, 0]]                       # width == 4 dropped, 4.25 kept, height 4 dropped, outside dropped
    assert s["box"][0, 3].tolist() == [512, 8, 512, 40] and s["box"][0, 4].tolist() == [0, 0, 20, 20]
    assert bool((s["score"] == 0.5).all())
    got = _select_torch(c)
    assert not P.check_select(s, got, "known") and np.array_equal(got[0], s["box"].astype(np.float32)) and bool((got[1] == 0.5).all())
    assert P.select(_known_case(min_size=0.0))["group"].tolist() == [[0, 0, 0, -1, 0, 0]]
    assert P.select(_known_case(min_size=-1.0))["group"].tolist() == [[0] * 6]
    sat = _select_torch(_known_case(logits=[np.inf, -np.inf, 0.0, 17.5, -0.0, np.nan]))
    assert sat[3].tolist() == [[0, 3, 2, 4, 1, 5]] and sat[1][0, :5].tolist() == [1.0, 1.0, 0.5, 0.5, 0.0] and np.isnan(sat[1][0, 5])


@pytest.mark.parametrize("plant,name", [("reg_channel", "g5x7_a3"), ("anchor_order", "g5x7_a3"), ("anchor_order", "g7x5_a3"), ("tie_plus_one", "tierun2"),
                                        ("tie_plus_one", "equal2"), ("no_clamp", "b3")])
def test_planted_errors_are_rejected(plant, name):
    c = P.build_case(name)
    assert not P.check_select(P.expected(name), _as_got(P.expected(name)), name)                  # the restatement passes its own check
    bad = P.check_select(P.expected(name), _as_got(P.select(c, plant)), f"{name}+{plant}")
    assert bad, f"{plant} passes on {name}"


def test_selection_by_the_rounded_score_is_rejected_on_a_saturated_case():
    """Distinct logits above 17 whose scores all round to 1: by score with ties by index the first anchors win, by logit the last."""
    c = dict(_known_case(min_size=0.0), nms_pre=3)
    n = len(c["anchors"])
    c["cls"] = [P._logits("saturated", (1, 1, 1, n), None, 3)]
    want = P.select(c)
    assert want["anchor_inds"].tolist() == [[5, 4, 3]] and bool((want["score"].astype(np.float32) == 1.0).all())
    planted = P.select(c, "score_select")
    assert planted["anchor_inds"].tolist() == [[0, 1, 2]]
    assert P.check_select(want, _as_got(planted), "saturated")
    assert not P.check_select(want, _select_torch(c), "saturated torch")


def test_ge_in_the_size_filter_is_rejected():
    c = _known_case()
    assert P.check_select(P.select(c), _as_got(P.select(c, "ge_filter")), "ge")
