"""`-m gpu`: RPN proposals on the MI355X (csp_select, HipOps.rpn_select, det_proposals).

Every case of tests/_proposal_ref.SELECT_CASES and E2E_CASES against the numpy restatement: anchor_inds, starts and the decided part of
`group` exact, scores and boxes inside their derived bounds (the worst ratio is printed).  Outputs are handed in as NaN / 0xFF, every call
runs twice and must give equal bits.  List lengths at which det_proposal.hip changes path, each with a case on either side (B = 1, L = 1):
n = nms_pre (a list no longer than nms_pre skips the select: pre{1,7,64,2000}_n*, n4096 / n4097_pre4096), n = 2048 (one or two workgroups
per list in the select passes: n2048_pre64 / n2050_pre64 -- 2049 = 3 * 683 is no h * w * A inside the limits) and k = 2048 (one or two
rounds of the 1024 sorting threads: pre2000_n2001 / n2050_pre2049).  1999 is a prime above 512, so 1998 stands in for nms_pre - 1 at
nms_pre = 2000.  Known answers bit for bit; end to end through HipOps and through det_proposals.rpn_proposals with call counters; the chain
into rcnn_targets(proposal_counts=) without a read-back; read / write extents inside the poisoned halos of tests/_extents.py.  The two
callers of det_common.h's decode_box (csp_select, csd_delta2bbox) are held to equal bits on clamped and clipped rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _proposal_ref as P  # noqa: E402
from _extents import run_case  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(hip, c, once=False):
    """HipOps.rpn_select on a case, outputs handed in as NaN / 0xFF, twice with equal bits -> (boxes, scores, group, inds, starts) numpy
    in the [B, Ktot] layout."""
    cls, reg = [_dev(x) for x in c["cls"]], [_dev(x) for x in c["reg"]]
    anchors, ms = _dev(c["anchors"]), _dev(c["max_shape"])
    B = c["cls"][0].shape[0]
    Ktot = sum(min(c["nms_pre"], int(np.prod(x.shape[1:]))) for x in c["cls"])
    runs = []
    for _ in range(1 if once else 2):
        out = (torch.full((B * Ktot, 4), float("nan"), device="cuda"), torch.full((B * Ktot,), float("nan"), device="cuda"),
               torch.full((B * Ktot,), -1, dtype=torch.int32, device="cuda"), torch.full((B * Ktot,), -1, dtype=torch.int32, device="cuda"),
               torch.full((B + 1,), -1, dtype=torch.int32, device="cuda"))           # 0xFF bytes: an unwritten row shows as NaN box / score, index -1
        got = hip.rpn_select(cls, reg, anchors, c["nms_pre"], c["means"], c["stds"], c["wh_ratio_clip"], ms, c["min_bbox_size"], out=out)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in got])
    if not once:
        for x, y in zip(*runs):
            assert np.array_equal(_bits(x), _bits(y)), "two launches differ in bits"
    b, s, g, i, st = runs[0]
    return [b.reshape(B, Ktot, 4), s.reshape(B, Ktot), g.reshape(B, Ktot), i.reshape(B, Ktot), st]


# ------------------------------------------------------------------------------------------------ select against the restatement
@pytest.mark.parametrize("name", list(P.SELECT_CASES) + list(P.E2E_CASES))
def test_select_equals_the_restatement(hip, name):
    c, want = P.build_case(name), P.expected(name)
    assert int(want["band"].sum()) == 0
    bad = P.check_select(want, _run(hip, c), name)
    assert not bad, "\n".join(bad)


def test_anchor_inds_may_be_null(hip):
    c = P.build_case("b3")
    cls, reg = [_dev(x) for x in c["cls"]], [_dev(x) for x in c["reg"]]
    want = P.expected("b3")
    B, Ktot = want["anchor_inds"].shape
    out = (torch.empty(B * Ktot, 4, device="cuda"), torch.empty(B * Ktot, device="cuda"), torch.empty(B * Ktot, dtype=torch.int32, device="cuda"), None,
           torch.empty(B + 1, dtype=torch.int32, device="cuda"))
    hip.rpn_select(cls, reg, _dev(c["anchors"]), c["nms_pre"], c["means"], c["stds"], c["wh_ratio_clip"], _dev(c["max_shape"]), c["min_bbox_size"], out=out)
    torch.cuda.synchronize()
    full = _run(hip, c, once=True)
    assert np.array_equal(_bits(out[0].cpu().numpy().reshape(B, Ktot, 4)), _bits(full[0])) and np.array_equal(out[2].cpu().numpy().reshape(B, Ktot), full[2])


# ------------------------------------------------------------------------------------------------ known answers, bit for bit
def _known_case(min_size, logits=None):
    anchors = np.array([[8, 8, 12, 40], [16, 8, 20.25, 40], [32, 8, 40, 12], [600, 8, 640, 40], [-8, -8, 20, 20], [40, 40, 48, 48]], np.float32)
    n = len(anchors)
    x = np.zeros((1, 1, 1, n), np.float32) if logits is None else np.asarray(logits, np.float32).reshape(1, 1, 1, n)
    return dict(cls=[x], reg=[np.zeros((1, 4, 1, n), np.float32)], anchors=anchors, max_shape=np.array([[64.0, 512.0]], np.float32), nms_pre=n,
                means=(0.0,) * 4, stds=(1.0,) * 4, wh_ratio_clip=16 / 1000, min_bbox_size=min_size)


def test_known_answers_bit_for_bit(hip):
    """Zero deltas on dyadic anchors: the boxes are the clamped anchors exactly.  Width exactly 4 against min_bbox_size = 4 is dropped, 4.25
    kept; an anchor wholly outside the image is dropped at min_bbox_size = 0 and kept at -1.  Logit 0 -> 0.5, +inf -> 1, -inf -> 0."""
    c = _known_case(4.0)
    boxes, scores, group, inds, starts = _run(hip, c)
    clamped = np.array([[8, 8, 12, 40], [16, 8, 20.25, 40], [32, 8, 40, 12], [512, 8, 512, 40], [0, 0, 20, 20], [40, 40, 48, 48]], np.float32)
    assert np.array_equal(_bits(boxes[0]), _bits(clamped))
    assert inds.tolist() == [[0, 1, 2, 3, 4, 5]] and starts.tolist() == [0, 6] and bool((scores == 0.5).all())
    assert group.tolist() == [[-1, 0, -1, -1, 0, 0]]
    assert _run(hip, _known_case(0.0))[2].tolist() == [[0, 0, 0, -1, 0, 0]]
    assert _run(hip, _known_case(-1.0))[2].tolist() == [[0] * 6]
    boxes, scores, group, inds, _ = _run(hip, _known_case(0.0, [np.inf, -np.inf, 0.0, 17.5, -0.0, np.nan]))
    assert inds.tolist() == [[0, 3, 2, 4, 1, 5]]
    assert scores[0, :5].tolist() == [1.0, 1.0, 0.5, 0.5, 0.0] and np.isnan(scores[0, 5])
    assert np.array_equal(_bits(boxes[0]), _bits(clamped[[0, 3, 2, 4, 1, 5]]))
    sat = dict(_known_case(0.0), nms_pre=3, cls=[P._logits("saturated", (1, 1, 1, 6), None, 3)])
    assert _run(hip, sat)[3].tolist() == [[5, 4, 3]]                                    # by logit, though every score is 1
    no_clamp = dict(_known_case(-1.0), max_shape=None)
    assert np.array_equal(_bits(_run(hip, no_clamp)[0][0]), _bits(c["anchors"]))


# ------------------------------------------------------------------------------------------------ the two callers of decode_box
DECODE_SEED = 0          # chosen on the CPU with select_torch / delta2bbox_torch: both lists of both nms_pre hold clamped and clipped rows


def _decode_case():
    """Two levels (4 x 4 and 2 x 3), A = 3, B = 2; unscaled randn deltas against wh_ratio_clip = 0.5 (the clamp is at |d| = ln 2, so about
    half of dw / dh hit it); anchors that reach past the small max_shape; min_bbox_size = -1 keeps every row."""
    g = torch.Generator().manual_seed(DECODE_SEED)
    dims, A, B = [(4, 4), (2, 3)], 3, 2
    cls = [torch.randn(B, A, h, w, generator=g) for h, w in dims]
    reg = [torch.randn(B, 4 * A, h, w, generator=g) for h, w in dims]
    N = sum(h * w * A for h, w in dims)
    ctr, half = torch.rand(N, 2, generator=g) * 64.0, torch.rand(N, 2, generator=g) * 20.0 + 2.0
    anchors = torch.cat([ctr - half, ctr + half], dim=1)
    return dict(cls=cls, reg=reg, anchors=anchors, max_shape=torch.tensor([[40.0, 48.0], [36.0, 44.0]]), means=(0.05, -0.1, 0.2, -0.15),
                stds=(0.5, 0.6, 1.1, 0.9), wh_ratio_clip=0.5, A=A)


def _gather_deltas(reg, inds, A):
    """The four raw deltas of anchor inds[b, t] (index into the concatenated anchor list) from the [B, 4A, h, w] maps -> [B, Ktot, 4]."""
    flat = torch.cat([r.reshape(r.shape[0], A, 4, -1).permute(0, 3, 1, 2).reshape(r.shape[0], -1, 4) for r in reg], dim=1)     # [B, N, 4]
    return torch.gather(flat, 1, inds.long().unsqueeze(-1).expand(-1, -1, 4))


@pytest.mark.parametrize("nms_pre", [64, 8])          # every list short (no select) / every list long (the select path)
def test_select_and_delta2bbox_decode_to_the_same_bits(hip, nms_pre):
    """prop_rows_kernel and delta2bbox_kernel both call decode_box of det_common.h: every row of csp_select equals csd_delta2bbox of that
    row's anchor and its four deltas, bit for bit -- and some of the rows are clamped at max_ratio, some clipped at max_shape."""
    c = _decode_case()
    cls, reg = [x.cuda() for x in c["cls"]], [x.cuda() for x in c["reg"]]
    anchors, ms = c["anchors"].cuda(), c["max_shape"].cuda()
    boxes, _, _, inds, starts = hip.rpn_select(cls, reg, anchors, nms_pre, c["means"], c["stds"], c["wh_ratio_clip"], ms, -1.0)
    B = ms.shape[0]
    Ktot = boxes.shape[0] // B
    assert Ktot == sum(min(nms_pre, x[0].numel()) for x in c["cls"])
    rows = inds >= 0
    assert bool(rows.all())                                                                # no anchor index is out of range
    rois = anchors[inds.long()]
    deltas = _gather_deltas(reg, inds.view(B, Ktot), c["A"]).reshape(B * Ktot, 4).contiguous()
    want = hip.delta2bbox(rois, deltas, torch.empty_like(boxes), c["means"], c["stds"], c["wh_ratio_clip"], starts, ms, None)
    free = hip.delta2bbox(rois, deltas, torch.empty_like(boxes), c["means"], c["stds"], c["wh_ratio_clip"])
    torch.cuda.synchronize()
    bad = torch.nonzero((boxes != want).any(dim=1) & rows)[:, 0].tolist()
    assert torch.equal(boxes[rows], want[rows]), f"rows {bad[:8]}: select {boxes[bad[:8]].tolist()} delta2bbox {want[bad[:8]].tolist()}"
    f = lambda v: torch.tensor(v, device="cuda")
    d = deltas * f(c["stds"]) + f(c["means"])
    clamped = (d[:, 2:].abs() > abs(np.log(c["wh_ratio_clip"])) + 1e-3).any(dim=1)
    clipped = (free != want).any(dim=1)
    print(f"nms_pre {nms_pre}: {B * Ktot} rows, {int(clamped.sum())} clamped, {int(clipped.sum())} clipped")
    assert int(clamped.sum()) >= 1 and int(clipped.sum()) >= 1 and int((~clamped).sum()) >= 1 and int((~clipped).sum()) >= 1


# ------------------------------------------------------------------------------------------------ end to end
def _cfg(c, sp):
    return dict(nms_pre=c["nms_pre"], max_per_img=sp["max_per_img"], nms=dict(type="nms", iou_threshold=sp["iou"]), min_bbox_size=c["min_bbox_size"])


@pytest.mark.parametrize("name", list(P.E2E_CASES))
def test_end_to_end_equals_the_restatement(hip, name, monkeypatch):
    from clipself_amd import det_proposals
    c, sp = P.build_case(name), P.E2E_CASES[name]
    sel = P.expected(name)
    assert P.min_score_gap_ratio(sel) > 1 and float(sel["box_bound"].max()) == 0.0
    want = P.rpn_proposals(c, sp["max_per_img"], sp["iou"], sel)
    L, (B, Ktot) = len(c["cls"]), sel["anchor_inds"].shape
    cls, reg, anchors, ms = [_dev(x) for x in c["cls"]], [_dev(x) for x in c["reg"]], _dev(c["anchors"]), _dev(c["max_shape"])
    # through HipOps
    boxes, scores, group, inds, starts = hip.rpn_select(cls, reg, anchors, c["nms_pre"], c["means"], c["stds"], c["wh_ratio_clip"], ms, c["min_bbox_size"])
    dets, labels, rows, counts = hip.nms(boxes, scores.view(-1, 1), starts, Ktot, -1.0, sp["iou"], sp["max_per_img"], group, L)
    ai = torch.where(rows >= 0, inds[rows.clamp(min=0).long()], torch.full_like(rows, -1))
    torch.cuda.synchronize()
    bad = P.check_proposals(want, [t.cpu().numpy() for t in (dets, counts, labels, ai)], name + " HipOps")
    assert not bad, "\n".join(bad)
    # through the module: one rpn_select and one nms, no quiet torch route
    calls = []
    real_sel, real_nms = type(hip).rpn_select, type(hip).nms
    monkeypatch.setattr(type(hip), "rpn_select", lambda self, *a, **k: (calls.append("select"), real_sel(self, *a, **k))[1])
    monkeypatch.setattr(type(hip), "nms", lambda self, *a, **k: (calls.append("nms"), real_nms(self, *a, **k))[1])
    got = det_proposals.rpn_proposals(cls, reg, anchors, ms, _cfg(c, sp), c["means"], c["stds"], ops=hip, return_inds=True)
    torch.cuda.synchronize()
    assert calls == ["select", "nms"]
    assert got[0].shape == (B, sp["max_per_img"], 5) and got[0].is_cuda
    bad = P.check_proposals(want, [t.cpu().numpy() for t in got], name + " module")
    assert not bad, "\n".join(bad)
    print(f"{name}: counts {got[1].tolist()}")
    # the torch route of the module on the same device gives the same proposals
    ref = det_proposals.rpn_proposals(cls, reg, anchors, ms, _cfg(c, sp), c["means"], c["stds"], ops=hip, fused=False, return_inds=True)
    assert calls == ["select", "nms", "nms"]
    # torch's device exp and division are not the device library's expf and IEEE division: a few ulps each, 1e-6 relative covers them
    assert torch.equal(ref[0][..., :4], got[0][..., :4]) and all(torch.equal(a, b) for a, b in zip(ref[1:], got[1:]))
    assert torch.allclose(ref[0][..., 4], got[0][..., 4], rtol=1e-6, atol=0)
    metas = [dict(img_shape=(float(h), float(w), 3)) for h, w in c["max_shape"]]
    lists = det_proposals.get_bboxes(cls, reg, anchors, metas, _cfg(c, sp), c["means"], c["stds"], ops=hip)
    assert [tuple(t.shape) for t in lists] == [(int(n), 5) for n in want[1]]
    assert all(torch.equal(t, got[0][b, :t.shape[0]]) for b, t in enumerate(lists))


def test_maps_of_any_float_dtype_are_converted(hip):
    from clipself_amd import det_proposals
    c = P.build_case("e2e_small")
    cls, reg = [_dev(x).half() for x in c["cls"]], [_dev(x).bfloat16() for x in c["reg"]]       # lattice values: exact in both formats
    got = det_proposals.select(cls, reg, _dev(c["anchors"]), _dev(c["max_shape"]), c["nms_pre"], c["means"], c["stds"], ops=hip)
    torch.cuda.synchronize()
    bad = P.check_select(P.expected("e2e_small"), [t.cpu().numpy() for t in got], "half maps")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the chain
def test_proposals_feed_rcnn_targets_without_a_read_back(hip, monkeypatch):
    from clipself_amd import det_proposals
    from clipself_amd import det_targets as T
    c, sp = P.build_case("e2e_cut"), P.E2E_CASES["e2e_cut"]
    cls, reg, anchors, ms = [_dev(x) for x in c["cls"]], [_dev(x) for x in c["reg"]], _dev(c["anchors"]), _dev(c["max_shape"])
    mx = 120
    cfg = dict(_cfg(c, sp), max_per_img=mx, nms=dict(type="nms", iou_threshold=0.1))
    B = c["cls"][0].shape[0]
    want = P.rpn_proposals(c, mx, 0.1, P.expected("e2e_cut"))
    assert int(want[1].min()) >= 5 and int(want[1].max()) < mx and len(set(want[1].tolist())) > 1     # ragged counts below the fixed shape
    gts = [_dev(want[0][b, [0, 3], :4] + np.float32(1.0)) for b in range(B)]
    labels = [torch.tensor([1, 2], device="cuda") for _ in range(B)]
    assigner = T.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False)
    sampler = T.RandomSampler(num=16, pos_fraction=0.25, add_gt_as_proposals=True)
    keys = T.random_keys((B, mx + 2), "cuda", torch.Generator(device="cuda").manual_seed(3))
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a read-back inside the chain")

    with monkeypatch.context() as m:
        for fn in ("item", "cpu", "tolist", "numpy"):
            m.setattr(torch.Tensor, fn, boom)
        props, counts = det_proposals.rpn_proposals(cls, reg, anchors, ms, cfg, c["means"], c["stds"], ops=hip)
        fixed = T.rcnn_targets(props[..., :4], gts, labels, assigner, sampler, num_classes=5, keys=keys, ops=hip, return_gt_inds=True,
                               proposal_counts=counts)
    torch.cuda.synchronize()
    assert counts.tolist() == want[1].tolist()
    trimmed = [props[b, :int(n), :4] for b, n in enumerate(counts.tolist())]
    nmax = max(t.shape[0] for t in trimmed) + 2
    lists = T.rcnn_targets(trimmed, gts, labels, assigner, sampler, num_classes=5, keys=keys[:, :nmax].contiguous(), ops=hip, return_gt_inds=True)
    for a, b in zip(fixed, lists):
        assert torch.equal(a, b)
    assert int((fixed[1] < 5).sum()) > 0


# ------------------------------------------------------------------------------------------------ extents
def _extent_case(name):
    c = P.build_case(name)

    def fn(ops, a):
        cls, reg = [a.inp(torch.from_numpy(x.copy())) for x in c["cls"]], [a.inp(torch.from_numpy(x.copy())) for x in c["reg"]]
        anchors = a.inp(torch.from_numpy(c["anchors"].copy()), a.ld(4))                    # a padded lda
        ms = None if c["max_shape"] is None else a.inp(torch.from_numpy(c["max_shape"].copy()))
        B = c["cls"][0].shape[0]
        Ktot = sum(min(c["nms_pre"], int(np.prod(x.shape[1:]))) for x in c["cls"])
        out = (a.out((B * Ktot, 4), torch.float32), a.out((B * Ktot,), torch.float32), a.out((B * Ktot,), torch.int32), a.out((B * Ktot,), torch.int32),
               a.out((B + 1,), torch.int32))
        ws = a.ws(ops.rpn_select_workspace(cls, reg, c["nms_pre"]))                         # exactly csp_workspace bytes
        ops.rpn_select(cls, reg, anchors, c["nms_pre"], c["means"], c["stds"], c["wh_ratio_clip"], ms, c["min_bbox_size"], out=out, workspace=ws)
        return dict(boxes=out[0], scores=out[1], group=out[2], anchor_inds=out[3], starts=out[4])
    return fn


EXTENT_CASES = ["ragged5", "b3", "special", "n2050_pre64", "n4097_pre4096", "pre7_n6", "tierun2"]


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("name", EXTENT_CASES)
def test_select_extents(hip, name, pad):
    """The padded rows of `anchors` are neither read as data nor written; nothing outside the five outputs and the workspace is written; the
    workspace's stale contents change nothing."""
    problems = run_case(hip, _extent_case(name), "cuda", pad, key=f"csp_select.{name}")
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------ the -1 cases
def test_a_refused_call_writes_nothing(hip):
    from clipself_amd.hip import RpnLevel
    import ctypes
    c = P.build_case("b3")
    cls, reg = [_dev(x) for x in c["cls"]], [_dev(x) for x in c["reg"]]
    anchors = _dev(c["anchors"])
    B, Ktot = P.expected("b3")["anchor_inds"].shape
    outs = [torch.full((B * Ktot, 4), -7.0, device="cuda"), torch.full((B * Ktot,), -7.0, device="cuda"),
            torch.full((B * Ktot,), -7, dtype=torch.int32, device="cuda"), torch.full((B * Ktot,), -7, dtype=torch.int32, device="cuda"),
            torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")]
    ws = torch.full((hip.rpn_select_workspace(cls, reg, c["nms_pre"]),), 0x5A, dtype=torch.uint8, device="cuda")
    arr = (RpnLevel * 2)(*[RpnLevel(x.data_ptr(), r.data_ptr(), x.shape[2], x.shape[3]) for x, r in zip(cls, reg)])
    f4 = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    stream = torch.cuda.current_stream().cuda_stream

    def call(L=2, B=B, A=3, lda=4, nms_pre=c["nms_pre"], clip=0.016, boxes=outs[0], wsp=ws):
        rc = hip.lib.csp_select(arr, L, B, A, anchors.data_ptr(), lda, nms_pre, f4, f4, clip, None, 0.0, None if boxes is None else boxes.data_ptr(),
                                outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), None if wsp is None else wsp.data_ptr(), stream)
        return rc, hip.lib.cs_last_error()

    for kw, word in [(dict(L=0), b"L ="), (dict(B=0), b"B ="), (dict(A=17), b"A ="), (dict(lda=3), b"lda"), (dict(nms_pre=0), b"nms_pre"),
                     (dict(nms_pre=4097), b"nms_pre"), (dict(clip=0.0), b"wh_ratio_clip"), (dict(boxes=None), b"boxes"), (dict(wsp=None), b"workspace")]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0x5A).all()), "a refused call wrote something"
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and outs[4].tolist() == [0, Ktot, 2 * Ktot, 3 * Ktot]
