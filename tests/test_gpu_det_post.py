"""`-m gpu`: detector post-processing on the MI355X (csd_nms / csd_delta2bbox, HipOps.nms / delta2bbox).

Every case of tests/_nms_ref.NMS_CASES against the float32 numpy restatement: exact inds, labels and counts, bit-equal dets.  Lattice
inputs make every area, intersection and union exact in fp32, so the kernel has to take the restatement's decisions; the random cases
(at most 130 boxes) assert min |iou64 - thr| > 1e-5 on the CPU first.  Boundaries of this layout (det_post.hip): 64 boxes per bitset
word; 4096 boxes per bitset register of a lane -- the 4100-box case crosses it; 2048 keys sorted in LDS by a scanning wave -- the 2040-
and 2500-box RPN cases sit on either side, both with one 2000-box list; max_num keeps per list end a scan early.  delta2bbox inside the
bound derived from its rounding count; read / write extents inside the poisoned halos of tests/_extents.py; equal bits from equal inputs;
every -1 case of the header through the raw entry point; and the batched `detections` behind OpenVocabBoxScores on the backbone fixture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _nms_ref as R  # noqa: E402
from _backbone_ref import FIXTURES, load_fixture  # noqa: E402
from _extents import run_case  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _run(hip, c, **kw):
    out = hip.nms(_dev(c["boxes"]), _dev(c["scores"]), _dev(c["starts"]), c["Kmax"], c["score_thr"], c["iou_thr"], c["max_num"],
                  _dev(c["group"]), c["G"], **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", list(R.NMS_CASES))
def test_nms_equals_the_restatement(hip, name):
    c = R.build_case(name)
    if not R.NMS_CASES[name].get("lattice", True):
        for b in range(len(c["starts"]) - 1):
            margin = R.min_iou_margin(c["boxes"][c["starts"][b]:c["starts"][b + 1]], c["iou_thr"])
            print(f"{name} image {b}: min |iou64 - thr| = {margin:.3e}")
            assert margin > 1e-5
    got = _run(hip, c)
    print(f"{name}: counts {got[3].tolist()}")
    R.compare(name, got)


def test_two_launches_give_equal_bits(hip):
    for name in ("c67", "rpn2500", "n1000"):
        c = R.build_case(name)
        a, b = _run(hip, c), _run(hip, c)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), name


def test_module_routes_cuda_tensors_to_the_kernels(hip, monkeypatch):
    """det_post.nms / multiclass_nms / batched_nms on CUDA tensors call HipOps.nms (no quiet torch route) and agree with the restatement."""
    from clipself_amd import det_post
    calls = []
    real = type(hip).nms
    monkeypatch.setattr(type(hip), "nms", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    c = R.build_case("c65")
    n, C = c["boxes"].shape[0], c["scores"].shape[1]
    multi = np.concatenate([c["scores"], np.full((n, 1), 0.99, np.float32)], 1)
    dets, labels, flat = det_post.multiclass_nms(_dev(c["boxes"]), _dev(multi), c["score_thr"], dict(type="nms", iou_threshold=c["iou_thr"]),
                                                 c["max_num"], return_inds=True)
    wd, wl, wi, wc = R.expected("c65")
    m = int(wc[0])
    assert len(calls) == 1 and dets.shape == (m, 5) and labels.tolist() == wl[0, :m].tolist()
    assert np.array_equal(dets.cpu().numpy().view(np.int32), wd[0, :m].view(np.int32)) and flat.tolist() == (wi[0, :m].astype(np.int64) * C + wl[0, :m]).tolist()
    g = R.build_case("group_small")
    k = int(g["starts"][1])
    idxs = np.clip(g["group"][:k], 0, 4)
    dets, keep = det_post.batched_nms(_dev(g["boxes"][:k]), _dev(g["scores"][:k, 0]), _dev(idxs).long(), dict(type="nms", iou_threshold=0.7))
    assert len(calls) == 2 and keep.tolist() == R.batched_nms_offset(g["boxes"][:k], g["scores"][:k, 0], idxs, 0.7, np.float32)
    assert torch.equal(dets[:, :4].cpu(), torch.from_numpy(g["boxes"][:k].copy())[keep.cpu()])
    with pytest.raises(ValueError, match="max_num"):
        det_post.batched_nms(torch.zeros(5000, 4, device="cuda"), torch.zeros(5000, device="cuda"), torch.zeros(5000, dtype=torch.long, device="cuda"),
                             dict(type="nms", iou_threshold=0.7))


# ------------------------------------------------------------------------------------------------ delta2bbox
@pytest.mark.parametrize("form", ["plain", "clip", "clip+scale"])
@pytest.mark.parametrize("K", [0, 1, 130, 1000])
def test_delta2bbox_within_the_derived_bound(hip, form, K):
    """Rows 0 / 1 sit at the wh_ratio_clip clamp, rows 2 / 3 cross the image border (tests/_nms_ref.delta2bbox_inputs); three ragged images."""
    rois, deltas = R.delta2bbox_inputs(K, 3 + K)
    starts = [0, K // 3, K // 3, K]
    max_shape = [[480.0, 512.0], [300.0, 200.0], [512.0, 333.0]] if form != "plain" else None
    scale = [[1.5, 1.25, 1.5, 1.25], [0.7, 0.7, 0.7, 0.7], [1.6180340051651, 0.3, 1.6180340051651, 0.3]] if form == "clip+scale" else None
    means, stds = (0.01, -0.02, 0.0, 0.03), (0.1, 0.1, 0.2, 0.2)
    want, bound = R.delta2bbox(rois, deltas, means, stds, 16 / 1000, starts, max_shape, scale)
    rois5 = torch.cat([torch.zeros(K, 1), torch.from_numpy(rois)], 1).cuda()                   # the [K, 5] layout: rois + 1, ldr = 5
    out = torch.full((K, 6), -7.0, device="cuda")
    hip.delta2bbox(rois5[:, 1:], _dev(deltas), out[:, :4], means, stds, 16 / 1000, _dev(np.array(starts, np.int32)),
                   None if max_shape is None else torch.tensor(max_shape, device="cuda"), None if scale is None else torch.tensor(scale, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out[:, 4:] == -7.0).all()), "the padding of the output rows was written"
    got = out[:, :4].double().cpu().numpy()
    err = np.abs(got - want)
    print(f"delta2bbox [{form}, K={K}]: worst err / bound {float((err / np.maximum(bound, 1e-300)).max()) if K else 0.0:.3f}")
    assert bool((err <= bound).all())


def test_module_delta2bbox_uses_the_kernel_and_matches_the_torch_route_up_to_expf(hip):
    from clipself_amd import det_post
    rois, deltas = R.delta2bbox_inputs(130, 9)
    got = det_post.delta2bbox(_dev(rois), _dev(deltas), (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), max_shape=(480, 512, 3))
    want, bound = R.delta2bbox(rois, deltas, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), 16 / 1000, [0, 130], [[480.0, 512.0]])
    assert got.is_cuda and bool((np.abs(got.double().cpu().numpy() - want) <= bound).all())


# ------------------------------------------------------------------------------------------------ extents
def _nms_extent_case(name, starts=None, group_edit=None):
    c = R.build_case(name)

    def fn(ops, a):
        K, C = c["scores"].shape
        st = c["starts"] if starts is None else np.array(starts, np.int32)
        B = len(st) - 1
        boxes = a.inp(torch.from_numpy(c["boxes"].copy()), a.ld(4))
        scores = a.inp(torch.from_numpy(c["scores"].copy()), a.ld(C))
        group = None
        if c["group"] is not None:
            g = c["group"].copy()
            if group_edit:
                group_edit(g)
            group = a.inp(torch.from_numpy(g))
        L = c["G"] if group is not None else C
        mx = c["max_num"]
        out = (a.out((B, mx, 5), torch.float32), a.out((B, mx), torch.int32), a.out((B, mx), torch.int32), a.out((B,), torch.int32))
        ws = a.ws(ops.nms_workspace(B, c["Kmax"], L, mx))
        ops.nms(boxes, scores, a.inp(torch.from_numpy(st.copy())), c["Kmax"], c["score_thr"], c["iou_thr"], mx, group, c["G"], out=out, workspace=ws)
        return dict(dets=out[0], labels=out[1], inds=out[2], counts=out[3])
    return fn


def _far_groups(g):
    g[::7], g[3::11] = 1 << 30, -(1 << 30)


EXTENT_CASES = {
    "ragged_b": _nms_extent_case("ragged_b"), "c67": _nms_extent_case("c67"), "n1000": _nms_extent_case("n1000"),
    "kmax_clamp": _nms_extent_case("kmax_clamp"), "rpn2500": _nms_extent_case("rpn2500"), "nonfinite": _nms_extent_case("nonfinite"),
    # starts is device data: past K, negative and non-monotone entries are clamped / give empty images, never an access outside the arrays
    "wild_starts": _nms_extent_case("ragged_a", starts=[-5, 130, 60, 1 << 30]),
    "wild_groups": _nms_extent_case("group_small", group_edit=_far_groups),
}


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("name", list(EXTENT_CASES))
def test_nms_extents(hip, name, pad):
    """Padded ldb / lds rows are neither read as data nor written; nothing outside the four outputs and the workspace is written; the
    workspace's stale contents change nothing."""
    problems = run_case(hip, EXTENT_CASES[name], "cuda", pad, key=f"csd_nms.{name}")
    assert not problems, "\n".join(problems)


def test_wild_starts_and_groups_follow_the_contract(hip):
    c = R.build_case("ragged_a")
    starts = np.array([-5, 130, 60, 1 << 30], np.int32)           # image 0: rows 0..129; image 1: empty; image 2: rows 60..192, Kmax = 130 of them
    want = R.multiclass(c["boxes"], c["scores"], starts, c["Kmax"], c["score_thr"], c["iou_thr"], c["max_num"])
    got = _run(hip, dict(c, starts=starts))
    assert got[3][1] == 0 and got[3][0] > 0 and got[3][2] > 0
    R.compare("wild_starts", got, want)
    g = R.build_case("group_small")
    grp = g["group"].copy()
    _far_groups(grp)
    want = R.multiclass(g["boxes"], g["scores"], g["starts"], g["Kmax"], g["score_thr"], g["iou_thr"], g["max_num"], grp, g["G"])
    got = _run(hip, dict(g, group=grp))
    R.compare("wild_groups", got, want)
    kept = got[2][got[2] >= 0]
    assert not np.isin(kept, np.nonzero((grp < 0) | (grp >= g["G"]))[0]).any()


def _delta_extent_case(K):
    def fn(ops, a):
        rois, deltas = R.delta2bbox_inputs(K, 5)
        r = a.inp(torch.from_numpy(rois), a.ld(4))
        d = a.inp(torch.from_numpy(deltas), a.ld(4))
        st = a.inp(torch.tensor([0, K // 2, K], dtype=torch.int32))
        ms, sc = a.inp(torch.tensor([[480.0, 512.0], [300.0, 200.0]])), a.inp(torch.tensor([[1.5, 1.25, 1.5, 1.25], [0.7, 0.7, 0.7, 0.7]]))
        out = a.out((K, 4), torch.float32, a.ld(4))
        ops.delta2bbox(r, d, out, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), 16 / 1000, st, ms, sc)
        return dict(out=out)
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("K", [1, 259])
def test_delta2bbox_extents(hip, K, pad):
    problems = run_case(hip, _delta_extent_case(K), "cuda", pad, key=f"csd_delta2bbox[{K}]")
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------ the -1 cases
def test_every_limit_returns_minus_one_and_writes_nothing(hip):
    c = R.build_case("n65")
    K, C, mx = 65, 2, 8
    boxes, scores, starts = _dev(c["boxes"]), _dev(c["scores"]), _dev(c["starts"])
    group = torch.zeros(K, dtype=torch.int32, device="cuda")
    outs = [torch.full((1, mx, 5), -7.0, device="cuda"), torch.full((1, mx), -7, dtype=torch.int32, device="cuda"),
            torch.full((1, mx), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")]
    ws = torch.full((hip.nms_workspace(1, K, C, mx),), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(B=1, C=C, K=K, Kmax=K, max_num=mx, ldb=4, lds=C, group=None, G=0, ws=ws):
        rc = hip.lib.csd_nms(boxes.data_ptr(), ldb, scores.data_ptr(), lds, C, starts.data_ptr(), None if group is None else group.data_ptr(), G, K,
                             B, Kmax, 0.1, 0.5, max_num, *[o.data_ptr() for o in outs], None if ws is None else ws.data_ptr(), stream)
        return rc, hip.lib.cs_last_error()

    for kw, word in [(dict(B=0), b"B ="), (dict(C=0, lds=0), b"C ="), (dict(K=-1), b"K ="), (dict(Kmax=16385), b"Kmax"),
                     (dict(Kmax=16384, C=1 << 17, lds=1 << 17), b"Kmax * C"), (dict(max_num=0), b"max_num"), (dict(max_num=4097), b"max_num"),
                     (dict(ldb=3), b"ldb"), (dict(lds=1), b"lds"), (dict(group=group, G=5), b"group"), (dict(ws=None), b"workspace")]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0x5A).all()), "a refused call wrote something"
    rc, _ = call()                                              # the same arguments inside the limits run
    torch.cuda.synchronize()
    assert rc == 0 and int(outs[3][0]) == mx


# ------------------------------------------------------------------------------------------------ end to end on the backbone fixture
def test_detections_on_the_backbone_fixture(hip):
    """The fixture's dense map -> OpenVocabBoxScores(fused=False) -> det_post.detections (decode, rescale, NMS, cut; nothing read back)
    against the restatement fed the same scores and the float64 decode: decoded boxes inside the derived bound, the NMS on the kernel's
    own decoded boxes exact."""
    from clipself_amd import det_post
    from clipself_amd.ov_head import OpenVocabBoxScores
    _, _, fmap, _ = load_fixture(FIXTURES[0])
    Bn, E, h, w = fmap.shape
    stride, C1 = 8, 7
    g = torch.Generator().manual_seed(5)
    side = float(h * stride)
    ns = [23, 17]
    xy = torch.rand(sum(ns), 2, generator=g) * (side - 12)
    rois = torch.cat([torch.repeat_interleave(torch.arange(Bn), torch.tensor(ns)).float()[:, None], xy, xy + 4 + torch.rand(sum(ns), 2, generator=g) * 8], 1)
    head = OpenVocabBoxScores(torch.randn(C1, E, generator=g), alpha=0.3, featmap_stride=stride, ops=hip, fused=False).cuda().eval()
    det_logits = torch.randn(sum(ns), C1, generator=g) * 2
    bbox_pred = torch.randn(sum(ns), 4, generator=g)
    scores = head(det_logits.cuda(), fmap.cuda(), rois.cuda())
    img_shapes, scales = [(32, 32, 3), (30, 28, 3)], [(1.5, 1.5, 1.5, 1.5), (0.8, 0.75, 0.8, 0.75)]
    dets, labels, inds, counts = det_post.detections(rois.cuda(), scores, bbox_pred.cuda(), img_shapes, scales, 0.02, 0.5, 20, head.target_means,
                                                     head.target_stds, Kmax=32)
    torch.cuda.synchronize()
    starts = [0, ns[0], sum(ns)]
    want_boxes, bound = R.delta2bbox(rois[:, 1:].numpy(), bbox_pred.numpy(), head.target_means, head.target_stds, 16 / 1000, starts,
                                     [s[:2] for s in img_shapes], scales)
    boxes = torch.empty(sum(ns), 4, device="cuda")
    hip.delta2bbox(rois.cuda()[:, 1:], bbox_pred.cuda(), boxes, head.target_means, head.target_stds, 16 / 1000, _dev(np.array(starts, np.int32)),
                   torch.tensor([s[:2] for s in img_shapes], dtype=torch.float32, device="cuda"), torch.tensor(scales, device="cuda"))
    assert bool((np.abs(boxes.double().cpu().numpy() - want_boxes) <= bound).all())
    want = R.multiclass(boxes.cpu().numpy(), scores[:, :C1 - 1].cpu().numpy(), starts, 32, 0.02, 0.5, 20)
    assert int(want[3].min()) > 0
    R.compare("fixture", [t.cpu().numpy() for t in (dets, labels, inds, counts)], want)


# ------------------------------------------------------------------------------------------------ the shared workspace of HipOps
def _boxes(g, n, side=64.0):
    xy = torch.rand(n, 2, generator=g) * (side - 24)
    return torch.cat([xy, xy + 2 + torch.rand(n, 2, generator=g) * 20], 1)


def test_one_workspace_per_header_serves_small_large_small():
    """HipOps keeps one grow-only workspace per header and device.  A small call, a large one and the small one again, on one stream,
    each give the bits of the same call with a fresh workspace of exactly the size the library asks for: a grown buffer carries nothing
    into a smaller call, and a small buffer is never handed to a larger one.  Afterwards there is one buffer per header, not per shape."""
    from clipself_amd.hip import HipOps
    ops = HipOps()                                                 # its own caches: the count at the end is exact
    g = torch.Generator().manual_seed(11)
    dev = torch.device("cuda", torch.cuda.current_device())
    fresh = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)

    def same(a, b, what):
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), what

    largest = {}

    def nms(B, Kmax):
        boxes, scores = _boxes(g, B * Kmax).cuda(), torch.rand(B * Kmax, 2, generator=g).cuda()
        starts = (torch.arange(B + 1, dtype=torch.int32) * Kmax).cuda()
        need = ops.nms_workspace(B, Kmax, 2, 10)
        largest["clipself_det.h"] = max(largest.get("clipself_det.h", 0), need)
        same(ops.nms(boxes, scores, starts, Kmax, 0.05, 0.5, 10), ops.nms(boxes, scores, starts, Kmax, 0.05, 0.5, 10, workspace=fresh(need)),
             f"nms B = {B}, Kmax = {Kmax}")

    def assign(Nmax, Gmax=3):
        boxes, gts = _boxes(g, Nmax).cuda(), _boxes(g, Gmax).cuda()
        gs = torch.tensor([0, Gmax], dtype=torch.int32, device=dev)
        need = ops.assign_workspace(1, Nmax, Gmax)
        largest["clipself_assign.h"] = max(largest.get("clipself_assign.h", 0), need)
        same(ops.assign(boxes, None, gts, gs, 1, Nmax, Gmax, 0.5, 0.4, 0.1), ops.assign(boxes, None, gts, gs, 1, Nmax, Gmax, 0.5, 0.4, 0.1, workspace=fresh(need)),
             f"assign Nmax = {Nmax}")

    def roi_bwd(K, P=2, C=8):
        grids, scales = [(4, 4), (2, 2)], [0.25, 0.125]           # a 16 x 16 image at strides 4 and 8; boxes of both levels
        half = torch.where(torch.arange(K) % 2 == 0, 1.5, 5.0)[:, None]
        ctr = 6 + torch.rand(K, 2, generator=g) * 4
        rois = torch.cat([torch.zeros(K, 1), ctr - half, ctr + half], 1).cuda()
        dout = torch.randn(K * P * P, C, generator=g).cuda()
        need = ops.roi_extract_workspace(K)
        largest["clipself_roi.h"] = max(largest.get("clipself_roi.h", 0), need)
        run = lambda **kw: ops.roi_extract_bwd(dout, rois, [torch.zeros(h * w, C, device=dev) for h, w in grids], grids, scales, 1, P, 0, 4.0, **kw)
        a, b = run(), run(workspace=fresh(need))
        same(a, b, f"roi_extract_bwd K = {K}")
        assert all(bool(t.abs().sum() > 0) for t in a), "both levels must receive gradient"

    for B, Kmax in ((1, 8), (2, 300), (1, 8)):
        nms(B, Kmax)
    for Nmax in (16, 600, 16):
        assign(Nmax)
    for K in (3, 70, 3):
        roi_bwd(K)
    assert {k: v.numel() for k, v in ops._ws.items()} == {(h, dev): n for h, n in largest.items()}
