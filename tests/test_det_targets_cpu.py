"""CPU: the detector's training targets (clipself_amd/det_targets.py, include/clipself_assign.h).

The torch route against the numpy restatement (tests/_assign_ref.py) on its whole case table: equal integers, bit-equal floats, dw / dh
included (both sides take libm's double log and round once).  The restatement's scalar-loop form against its vectorised form.
AnchorGenerator against values worked out by hand; bbox2delta inverted by det_post.delta2bbox inside a derived bound; the mmdet-named
classes built from the reference config's dicts; the sampler's invariants and uniformity; the C ABI: header, table, exports, limits."""
import inspect
import math

import numpy as np
import pytest
import torch

import _assign_ref as R



def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _keys_t(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy())


def _bits(name, got, want):
    assert R.same_float_bits(got.numpy() if isinstance(got, torch.Tensor) else got, want), name


def _ints(name, got, want):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), name


# ------------------------------------------------------------------------------------------------ restatement: scalar == vectorised
@pytest.mark.parametrize("name", R.SCALAR_CASES)
def test_restatement_scalar_loops_equal_the_vectorised_form(name):
    c, e = R.build_case(name), R.expected(name)
    gi, mo = R.assign(c, form="scalar")
    assert np.array_equal(gi, e["gt_inds"]) and R.same_float_bits(mo, e["max_overlaps"])
    out = R.sample(gi, c["keys"], c["starts"], len(c["boxes"]), c["gt_starts"], len(c["gts"]), c["Gmax"], c["num"], c["expected_pos"], c["ub"],
                   form="scalar")
    for got, key in zip(out, ("flags", "sel", "counts")):
        assert np.array_equal(got, e[key]), key


def test_restatement_sampler_forms_agree_on_the_hand_made_pools():
    for name, s in R.sample_cases().items():
        a = R.sample(s["gt_inds"], s["keys"], None, s["gt_inds"].shape[1], s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"])
        b = R.sample(s["gt_inds"], s["keys"], None, s["gt_inds"].shape[1], s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"],
                     form="scalar")
        for x, y in zip(a, b):
            assert np.array_equal(x, y), name


def test_lattice_cases_decide_what_the_header_says():
    """The hand-made geometry, checked against decisions worked out by hand (gt_inds is 1-based)."""
    e = R.expected("lattice_rpn_all")
    gi, mo = e["gt_inds"][0], e["max_overlaps"][0]
    assert mo[1] == np.float32(0.5) and mo[4] == np.float32(0.7) and mo[5] == np.float32(0.6) and mo[6] == np.float32(0.9)
    assert gi[0] == 2                      # identical gts 0 / 1: the positive rule gives 1, the later low-quality match overwrites with 2
    assert gi[1] == 3                      # 0.5 < 0.7, but it is gt 2's maximum >= min_pos_iou
    assert gi[2] == 4 and gi[3] == 4       # both share gt 3's maximum: gt_max_assign_all
    assert gi[4] == 5                      # 7/10 rounds to the float 0.7: positive
    assert gi[5] == 7                      # the maximum of gts 5 and 6: the later one wins
    assert gi[6] == 9                      # 0.9 with gt 7, overwritten by gt 8's low-quality match
    assert gi[7] == 0 and gi[8] == 0 and gi[10] == 0 and mo[7] == 0       # zero area, far away
    assert gi[9] == -1                     # 0.5 with gts 0 / 1, not their maximum: between the thresholds
    first = R.expected("lattice_rpn_first")["gt_inds"][0]
    assert first[2] == 4 and first[3] == -1                                 # without gt_max_assign_all only the lowest row
    rcnn = R.expected("lattice_rcnn")["gt_inds"][0]
    assert rcnn[0] == 1 and rcnn[1] == 3 and rcnn[2] == 4 and rcnn[3] == 4 and rcnn[9] == 1      # exactly 0.5 is positive, not negative
    assert rcnn[6] == 8                    # no low-quality matches: the positive stays


# ------------------------------------------------------------------------------------------------ torch route == restatement
@pytest.mark.parametrize("name", list(R.CASES))
def test_torch_route_equals_the_restatement(name):
    from clipself_amd import det_targets as T
    c, e = R.build_case(name), R.expected(name)
    a = c["assigner"]
    boxes, gts = _t(c["boxes"]), _t(c["gts"])
    gi, mo = T.assign(boxes, c["starts"], gts, c["gt_starts"], c["B"], c["Nmax"], c["Gmax"], a["pos"], a["neg"], a["min_pos"], a["mlq"], a["all"],
                      a["prefix"], _t(c["valid"]))
    assert gi.dtype == torch.int32 and mo.dtype == torch.float32
    _ints("gt_inds", gi, e["gt_inds"])
    _bits("max_overlaps", mo, e["max_overlaps"])
    flags, sel, counts = T.sample(gi, _keys_t(c["keys"]), c["starts"], len(c["boxes"]), c["gt_starts"], len(c["gts"]), c["Gmax"], c["num"],
                                  c["expected_pos"], c["ub"])
    _ints("flags", flags, e["flags"])
    _ints("sel", sel, e["sel"])
    _ints("counts", counts, e["counts"])
    dense = T.bbox_targets(boxes, c["starts"], gts, _t(c["gt_labels"]), c["gt_starts"], c["Gmax"], gi, flags, None, c["means"], c["stds"], c["bg_label"])
    for got, key in zip(dense, ("labels", "label_weights", "bbox_targets", "bbox_weights")):
        (_ints if key == "labels" else _bits)(f"dense {key}", got, e["dense"][key])
    compact = T.bbox_targets(boxes, c["starts"], gts, _t(c["gt_labels"]), c["gt_starts"], c["Gmax"], gi, None, sel, c["means"], c["stds"], c["bg_label"])
    for got, key in zip(compact, ("rois", "labels", "label_weights", "bbox_targets", "bbox_weights")):
        (_ints if key == "labels" else _bits)(f"compact {key}", got, e["compact"][key])


def test_torch_sampler_equals_the_restatement_on_the_hand_made_pools():
    from clipself_amd import det_targets as T
    for name, s in R.sample_cases().items():
        n = s["gt_inds"].shape[1]
        want = R.sample(s["gt_inds"], s["keys"], None, n, s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"])
        got = T.sample(_t(s["gt_inds"]), _keys_t(s["keys"]), None, n, s["gt_starts"], s["Gtot"], s["Gmax"], s["num"], s["expected_pos"], s["ub"])
        for g, w, key in zip(got, want, ("flags", "sel", "counts")):
            _ints(f"{name} {key}", g, w)


# ------------------------------------------------------------------------------------------------ anchors
CFG_ANCHORS = dict(scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64])


def test_anchor_generator_base_anchors_order_and_valid_flags():
    from clipself_amd.det_targets import AnchorGenerator
    assert list(inspect.signature(AnchorGenerator.__init__).parameters)[1:] == \
        ["strides", "ratios", "scales", "base_sizes", "scale_major", "octave_base_scale", "scales_per_octave", "centers", "center_offset"]
    gen = AnchorGenerator(**CFG_ANCHORS)
    assert gen.num_base_priors == [3] * 5 and gen.num_levels == 5
    # by hand: stride s, scale 8 -> side 8 s; ratio r = h / w: half-sides (4 s / sqrt(r), 4 s sqrt(r)).  stride 4: 16 x 16, ...
    for lvl, s in enumerate(CFG_ANCHORS["strides"]):
        half = 4.0 * s
        want = [[-half * math.sqrt(2), -half / math.sqrt(2), half * math.sqrt(2), half / math.sqrt(2)],
                [-half, -half, half, half],
                [-half / math.sqrt(2), -half * math.sqrt(2), half / math.sqrt(2), half * math.sqrt(2)]]
        got = gen.base_anchors[lvl]
        assert got.dtype == torch.float32 and torch.allclose(got, torch.tensor(want), rtol=0, atol=half * 4 * 2.0 ** -24 * 4)     # a few roundings of fp32
    assert gen.base_anchors[0][1].tolist() == [-16.0, -16.0, 16.0, 16.0]
    # count and order on a 3 x 5 map: location-major (row by row, x fastest), base anchors innermost
    sizes = [(3, 5), (2, 3), (1, 2), (1, 1), (1, 1)]
    pri = gen.grid_priors(sizes)
    assert [p.shape for p in pri] == [(h * w * 3, 4) for h, w in sizes]
    p0 = pri[0].view(3, 5, 3, 4)
    for y in range(3):
        for x in range(5):
            assert torch.equal(p0[y, x], gen.base_anchors[0] + torch.tensor([4.0 * x, 4.0 * y, 4.0 * x, 4.0 * y]))
    assert gen.grid_priors(sizes)[0] is pri[0]                              # cached
    assert np.array_equal(torch.cat(pri).numpy(), R.anchors_np(sizes))
    # valid_flags: a padded image of 9 x 14 pixels covers ceil(9 / 4) = 3 rows and ceil(14 / 4) = 4 of the 5 columns at stride 4
    vf = gen.valid_flags(sizes, (9, 14, 3))
    v0 = vf[0].view(3, 5, 3)
    assert v0.dtype == torch.bool and bool(v0[:, :4].all()) and not bool(v0[:, 4].any())
    assert vf[1].view(2, 3, 3)[:, :2].all() and not vf[1].view(2, 3, 3)[:, 2].any()          # ceil(14 / 8) = 2 of 3 columns
    assert all(bool(v.all()) for v in gen.valid_flags(sizes, (640, 640, 3)))
    oct_gen = AnchorGenerator(strides=[8], ratios=[1.0], octave_base_scale=4, scales_per_octave=3)
    assert oct_gen.num_base_priors == [3] and torch.allclose(oct_gen.base_anchors[0][:, 2], torch.tensor([16.0, 16 * 2 ** (1 / 3), 16 * 2 ** (2 / 3)]))
    with pytest.raises(ValueError):
        AnchorGenerator(strides=[8], ratios=[1.0])
    with pytest.raises(ValueError):
        AnchorGenerator(strides=[8], ratios=[1.0], scales=[8], octave_base_scale=4, scales_per_octave=3)


# ------------------------------------------------------------------------------------------------ bbox2delta <-> delta2bbox
@pytest.mark.parametrize("stds", [(1., 1., 1., 1.), (.1, .1, .2, .2)])
def test_bbox2delta_is_inverted_by_delta2bbox(stds):
    """delta2bbox(p, bbox2delta(p, g)) returns g.  Bound, with u = 2^-24, coordinates below X = 512, widths in [8, 200] so that
    |log(gw / pw)| <= log(25) < 3.3 and |gx - px| / pw < 64: encoding makes each delta with a relative error of a few u (one subtraction of
    rounded centres, one division, the log at <= 2 u of |dw| + the ratio's u, the normalisation's two roundings); decoding repeats as
    many.  A relative error e in dxy moves the centre by e |gx - px| < e X, one in dw of absolute size a scales the width by exp(a), so
    corners move by less than (12 u) X + (12 u)(1 + 3.3) * 200 / 2 + 4 u X (the centre's and the corner's own roundings)
    < 16 u X + 5200 u < 14000 u = 8.4e-4.  max_shape is off (None) and wh_ratio_clip = 16 / 1000 allows |dw| <= 4.13 > 3.3."""
    from clipself_amd import det_post
    from clipself_amd.det_targets import bbox2delta, delta2bbox
    assert delta2bbox is det_post.delta2bbox                                # imported, not copied
    rng = np.random.default_rng(3)
    xy, wh = rng.uniform(0, 300, (500, 2)), rng.uniform(8, 200, (500, 2))
    p = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32))
    xy, wh = rng.uniform(0, 300, (500, 2)), rng.uniform(8, 200, (500, 2))
    g = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32))
    d = bbox2delta(p, g, (0., 0., 0., 0.), stds)
    want, _, _ = R.bbox2delta(p.numpy(), g.numpy(), (0., 0., 0., 0.), stds)
    assert R.same_float_bits(d.numpy(), want)
    back = det_post.delta2bbox(p, d, (0., 0., 0., 0.), stds)
    err = float((back - g).abs().max())
    print(f"stds {stds}: max corner error {err:.3e} (bound 8.4e-4)")
    assert err < 14000 * 2.0 ** -24
    same = bbox2delta(p, p, (0., 0., 0., 0.), stds)
    assert bool((same == 0).all())                                          # gwh == pwh: exactly (0 - mean) / std


# ------------------------------------------------------------------------------------------------ mmdet's classes from the config's dicts
RPN_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1),
               sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
               allowed_border=-1, pos_weight=-1, debug=False)
RCNN_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1),
                sampler=dict(type='RandomSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True),
                pos_weight=-1, debug=False)


def test_config_dicts_build_the_classes_and_unsupported_keywords_raise():
    from clipself_amd.det_targets import MaxIoUAssigner, RandomSampler
    a, s = MaxIoUAssigner(**RPN_CFG["assigner"]), RandomSampler(**RPN_CFG["sampler"])
    assert (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.match_low_quality, a.gt_max_assign_all) == (0.7, 0.3, 0.3, True, True)
    assert (s.num, s.expected_pos, s.neg_pos_ub, s.add_gt_as_proposals) == (256, 128, -1, False)
    a2, s2 = MaxIoUAssigner(**RCNN_CFG["assigner"]), RandomSampler(**RCNN_CFG["sampler"])
    assert a2.match_low_quality is False and (s2.num, s2.expected_pos, s2.add_gt_as_proposals) == (512, 128, True)
    assert list(inspect.signature(MaxIoUAssigner.assign).parameters) == ["self", "bboxes", "gt_bboxes", "gt_bboxes_ignore", "gt_labels"]
    assert list(inspect.signature(RandomSampler.sample).parameters)[:6] == ["self", "assign_result", "bboxes", "gt_bboxes", "gt_labels", "generator"]
    for bad in (dict(ignore_iof_thr=0.5), dict(gpu_assign_thr=100), dict(iou_calculator=dict(type="BboxOverlaps3D")), dict(type="ATSSAssigner")):
        with pytest.raises(ValueError):
            MaxIoUAssigner(0.5, 0.5, **bad)
    for bad in (dict(pos_weight=2.0), dict(type="OHEMSampler"), dict(context=None)):
        with pytest.raises(ValueError):
            RandomSampler(16, 0.5, **bad)


def test_per_image_methods_return_mmdets_result_objects():
    from clipself_amd.det_targets import MaxIoUAssigner, RandomSampler
    c, e = R.build_case("starts_b3"), R.expected("starts_b3")
    n, g = c["starts"][1], c["gt_starts"][1]
    boxes, gts, labels = _t(c["boxes"][:n]), _t(c["gts"][:g]), _t(c["gt_labels"][:g]).long()
    res = MaxIoUAssigner(**RCNN_CFG["assigner"]).assign(boxes, gts, None, labels)
    assert res.num_gts == g and res.gt_inds.dtype == torch.int64 and np.array_equal(res.gt_inds.numpy(), e["gt_inds"][0, :n])
    _bits("max_overlaps", res.max_overlaps, e["max_overlaps"][0, :n])
    pos = res.gt_inds > 0
    assert bool((res.labels[~pos] == -1).all()) and torch.equal(res.labels[pos], labels[res.gt_inds[pos] - 1])
    sampler = RandomSampler(**RCNN_CFG["sampler"])
    out = sampler.sample(res, boxes, gts, labels, generator=torch.Generator().manual_seed(3))
    assert res.gt_inds.shape[0] == n + g and res.gt_inds[:g].tolist() == list(range(1, g + 1)) and bool((res.max_overlaps[:g] == 1).all())
    assert out.pos_inds.dtype == torch.int64 and out.num_gts == g
    assert len(out.pos_inds) == min(128, int((res.gt_inds > 0).sum())) and len(out.pos_inds) + len(out.neg_inds) == 512
    assert bool((res.gt_inds[out.pos_inds] > 0).all()) and bool((res.gt_inds[out.neg_inds] == 0).all())
    assert torch.equal(out.pos_assigned_gt_inds, res.gt_inds[out.pos_inds] - 1) and torch.equal(out.pos_gt_bboxes, gts[out.pos_assigned_gt_inds])
    assert torch.equal(out.pos_gt_labels, labels[out.pos_assigned_gt_inds]) and out.pos_bboxes.shape == (len(out.pos_inds), 4)
    assert out.neg_bboxes.shape == (len(out.neg_inds), 4) and bool(out.pos_is_gt[out.pos_inds < g].all())


def test_batched_forms_have_fixed_shapes_and_agree_with_the_pieces():
    from clipself_amd import det_targets as T
    c, e = R.build_case("anchors64"), R.expected("anchors64")
    gt_list = [_t(c["gts"][c["gt_starts"][b]:c["gt_starts"][b + 1]]) for b in range(3)]
    out = T.rpn_targets(_t(c["boxes"]), _t(c["valid"]), gt_list, T.MaxIoUAssigner(**RPN_CFG["assigner"]), T.RandomSampler(**RPN_CFG["sampler"]),
                        keys=_keys_t(c["keys"]))
    for got, key in zip(out[:4], ("labels", "label_weights", "bbox_targets", "bbox_weights")):
        (_ints if key == "labels" else _bits)(key, got, e["dense"][key])
    assert out[4].dim() == 0 and int(out[4]) == int(e["counts"].sum())
    p, e = R.build_case("prefix_b3"), R.expected("prefix_b3")
    props, gt_list, lab_list = [], [], []
    for b in range(3):
        gs, ge = p["gt_starts"][b], p["gt_starts"][b + 1]
        gt_list.append(_t(p["gts"][gs:ge]))
        lab_list.append(_t(p["gt_labels"][gs:ge]))
        props.append(_t(p["boxes"][p["starts"][b] + (ge - gs):p["starts"][b + 1]]))
    sampler = T.RandomSampler(num=128, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    rois, labels, lw, bt, bw = T.rcnn_targets(props, gt_list, lab_list, T.MaxIoUAssigner(**RCNN_CFG["assigner"]), sampler, keys=_keys_t(p["keys"]))
    assert rois.shape == (3 * 128, 5) and labels.shape == (384,) and bt.shape == (384, 4)
    _bits("rois", rois.view(3, 128, 5), e["compact"]["rois"])
    _ints("labels", labels.view(3, 128), e["compact"]["labels"])
    _bits("bbox_targets", bt.view(3, 128, 4), e["compact"]["bbox_targets"])
    _bits("bbox_weights", bw.view(3, 128, 4), e["compact"]["bbox_weights"])
    _bits("label_weights", lw.view(3, 128), e["compact"]["label_weights"])


# ------------------------------------------------------------------------------------------------ the sampler's invariants and uniformity
def test_sampler_invariants_over_200_seeds():
    from clipself_amd import det_targets as T
    gi = torch.tensor([[1, 0, 0, 2, -1, 0, 1, 0, 0, 3, 0, -1, 0, 2, 0, 0, 1, 0, 0, 0]], dtype=torch.int32)       # 6 positives, 12 negatives, 2 ignored
    pos_pool, neg_pool = set(torch.nonzero(gi[0] > 0)[:, 0].tolist()), set(torch.nonzero(gi[0] == 0)[:, 0].tolist())
    for seed in range(200):
        keys = T.random_keys((1, 20), "cpu", torch.Generator().manual_seed(seed))
        for num, epos, ub, want in ((8, 4, -1.0, (4, 4)), (16, 8, -1.0, (6, 10)), (20, 2, -1.0, (2, 12)), (16, 4, 1.0, (4, 4)), (16, 8, 0.5, (6, 3)),
                                    (4, 0, -1.0, (0, 4)), (4, 0, 1.0, (0, 1))):
            flags, sel, counts = T.sample(gi, keys, None, 20, [0, 3], 3, 3, num, epos, ub)
            assert tuple(counts[0].tolist()) == want, (seed, num, epos, ub)
            p, n = sel[0, :want[0]].tolist(), sel[0, want[0]:want[0] + want[1]].tolist()
            assert p == sorted(set(p)) and n == sorted(set(n)) and set(p) <= pos_pool and set(n) <= neg_pool
            assert bool((sel[0, want[0] + want[1]:] == -1).all())
            assert bool((flags[0][p] == 1).all()) and bool((flags[0][n] == 2).all()) and int((flags != 0).sum()) == sum(want)
            if want[0] == len(pos_pool):
                assert set(p) == pos_pool                                   # a short pool is taken whole


def test_sampler_is_uniform_over_a_fixed_pool():
    """10 positives, 3 drawn, T trials: each row is drawn with probability 3 / 10, so its count is Binomial(T, 0.3).  With T = 2000 the
    standard deviation is sqrt(T * 0.3 * 0.7) = 20.5; a 5 sigma interval on each of 10 rows fails by chance less than 1e-5 of the time, and
    the seeds are fixed."""
    from clipself_amd import det_targets as T_
    trials = 2000
    gi = torch.ones(1, 10, dtype=torch.int32)
    gen = torch.Generator().manual_seed(11)
    hits = np.zeros(10)
    for _ in range(trials):
        _, sel, counts = T_.sample(gi, T_.random_keys((1, 10), "cpu", gen), None, 10, [0, 1], 1, 1, 6, 3, -1.0)
        assert counts[0].tolist() == [3, 0]
        hits[sel[0, :3].numpy()] += 1
    sigma = math.sqrt(trials * 0.3 * 0.7)
    print("draws per row:", hits.tolist(), "expected", trials * 0.3, "+-", 5 * sigma)
    assert np.all(np.abs(hits - trials * 0.3) < 5 * sigma)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_limits_are_refused_without_a_device():
    """Argument checks come before any launch, so the -1 cases can be seen here: no pointer is touched."""
    from clipself_amd import hip
    lib = hip.load_library()
    ws = lib.csa_workspace
    assert ws(0, 10, 1, 1) == 0 and ws(65536, 10, 1, 1) == 0 and ws(1, -1, 1, 1) == 0 and ws(1, (1 << 20) + 1, 1, 1) == 0
    assert ws(1, 10, 1025, 1) == 0 and ws(1, 10, -1, 1) == 0 and ws(1, 10, 1, 0) == 0 and ws(1, 10, 1, 4097) == 0
    assert ws(8, 1 << 20, 1024, 4096) >= 8 * 8 * 1024 and ws(1, 0, 0, 1) >= 256
    P = 1 << 20

    def assign(B=1, Nmax=10, Gmax=4, K=10, Gtot=4, ldb=4, ldg=4, gt_starts=P, w=P):
        return lib.csa_assign(P, ldb, None, K, P, ldg, gt_starts, Gtot, None, B, Nmax, Gmax, 0.7, 0.0, 0.3, 0.3, 1, 1, 0, P, P, w, None)

    for kw, word in [(dict(B=0), b"B ="), (dict(B=65536), b"B ="), (dict(Nmax=-1), b"Nmax"), (dict(Nmax=(1 << 20) + 1), b"Nmax"),
                     (dict(Gmax=1025), b"Gmax"), (dict(Gmax=-1), b"Gmax"), (dict(K=-1), b"K ="), (dict(Gtot=-1), b"Gtot"), (dict(ldb=3), b"ldb"),
                     (dict(ldg=2), b"ldg"), (dict(gt_starts=None), b"gt_starts"), (dict(w=None), b"workspace")]:
        assert assign(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())

    def sample(B=1, Nmax=10, Gmax=4, num=8, epos=4):
        return lib.csa_sample(P, P, None, 10, P, 4, B, Nmax, Gmax, num, epos, -1.0, P, P, P, None)

    for kw, word in [(dict(B=0), b"B ="), (dict(Nmax=(1 << 20) + 1), b"Nmax"), (dict(num=0), b"num"), (dict(num=4097), b"num"),
                     (dict(epos=-1), b"expected_pos"), (dict(epos=9), b"expected_pos")]:
        assert sample(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())

    import ctypes
    f4 = (ctypes.c_float * 4)(0, 0, 0, 0)

    def targets(B=1, Gmax=4, num=8, sel=P, flags=P, means=f4, pos_weight=-1.0, rois=P):
        return lib.csa_targets(P, 4, None, 10, P, 4, None, P, 4, B, 10, Gmax, P, flags, sel, num, means, f4, 1, pos_weight, rois, P, P, P, P, None)

    for kw, word in [(dict(B=0), b"B ="), (dict(Gmax=2000), b"Gmax"), (dict(num=4097), b"num"), (dict(pos_weight=1.0), b"pos_weight"),
                     (dict(means=None), b"means"), (dict(sel=None, flags=None), b"flags"), (dict(rois=None), b"rois")]:
        assert targets(**kw) == -1, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())
