"""TEST INFRASTRUCTURE -- numpy restatement of the detector tail the kernels of det_post.hip replace, in float32 and float64.

What is restated, by the published function names (mmcv 1.x / mmdet 2.x; neither package nor its source is available to this project,
so this boundary is parity-unpinned in the sense of DESIGN.md §3.13: the restatement follows the published sources as read, it was not
run against them):

  mmcv.ops.nms (`nms`, offset=0; the CUDA kernel's `devIoU`):  area = (x1 - x0) * (y1 - y0), iw = max(min(x1a, x1b) - max(x0a, x0b), 0),
      inter = iw * ih, iou = inter / (area_a + area_b - inter); greedy in score order, b goes iff iou > iou_threshold   -> iou_matrix, greedy_nms
  mmcv.ops.batched_nms:  boxes + idxs * (boxes.max() + 1), one nms over everything                                     -> batched_nms_offset
  mmdet.core.post_processing.multiclass_nms:  drop the background column, valid = score > score_thr, batched_nms by label,
      then the first max_num                                                                                           -> multiclass
  mmdet.core.bbox.coder.delta_xywh_bbox_coder.delta2bbox (add_ctr_clamp=False, clip_border=True) and the rescale division of the
      reference's F-ViT/models/fvit_head.py:153-156                                                                    -> delta2bbox

`multiclass` is the contract of include/clipself_det.h (per-list NMS on un-offset boxes, ties to the lower row, per-image cut with ties to
the lower flat index, padded fixed-shape outputs); test_det_post_cpu.py pins that it equals the offset formulation in float64 on lattice
inputs.  numpy evaluates every float32 product and sum as an operation of its own, which is the arithmetic the header prescribes.

delta2bbox also returns the bound an fp32 evaluation is held to.  With u = 2^-24 and every magnitude taken from the float64 values:
  d = fl(fl(delta * std) + mean)          e_d  = u (|delta * std| + |d|)
  p = fl(fl(x0 + x1) * 0.5)               e_p  = u |p|                 (the product with 0.5 is exact)
  w = fl(x1 - x0)                         e_w  = u |w|
  t = fl(w * dxy)                         e_t  = 2 u |w dxy| + |w| e_d (the rounding of w, of the product, and d's error)
  g = fl(p + t)                           e_g  = e_p + e_t + u |g|
  clamp is 1-Lipschitz with the same fp32 bound on both sides: e stays e_d
  E = expf(dwh): 1 ulp = 2 u relative, and exp turns e_d into a relative error        rel_E = e_d + 2 u
  s = fl(w * E): rounding of w and of the product                                     rel_s = rel_E + 2 u = e_d + 4 u
  h = fl(s * 0.5) exact;  c = fl(g -+ h)  e_c  = e_g + 0.5 |s| (e_d + 4 u) + u |c|
  the clamp to the image is 1-Lipschitz with exact bounds;  out = fl(c / scale)        e_out = e_c / |scale| + u |out|
times (1 + 2^-10) for the second-order terms.  No constant is tuned.
"""
import numpy as np

U = 2.0 ** -24


# ================================================================================================ generators
def lattice_boxes(K, seed, side=512, smin=8, smax=160):
    """Coordinates on multiples of 1/4 in [0, side], sides smin..smax; the last quarter are copies of the first quarter jittered by up to
    2 px on the lattice.  Every area, intersection and union is below 2^24 / 16 in units of 1/16: exact in fp32, so the IoU is one
    correctly rounded division and an fp32 implementation must reproduce the float32 restatement's decisions exactly."""
    r = np.random.RandomState(seed)
    cx, cy = r.randint(0, side * 4, K) / 4.0, r.randint(0, side * 4, K) / 4.0
    w, h = r.randint(smin * 4, smax * 4, K) / 4.0, r.randint(smin * 4, smax * 4, K) / 4.0
    b = np.stack([cx, cy, cx + w, cy + h], 1).clip(0, side).astype(np.float32)
    q = K // 4
    if q:
        b[K - q:] = (b[:q] + (r.randint(-8, 9, (q, 4)) / 4.0).astype(np.float32)).clip(0, side)
    return b


def random_boxes(K, seed, side=512, smin=8, smax=160):
    """Off the lattice: the caller asserts min_iou_margin() > 1e-5 before it trusts an fp32 decision."""
    r = np.random.RandomState(seed)
    cx, cy = r.rand(K) * side, r.rand(K) * side
    w, h = smin + r.rand(K) * (smax - smin), smin + r.rand(K) * (smax - smin)
    b = np.stack([cx, cy, cx + w, cy + h], 1).clip(0, side).astype(np.float32)
    q = K // 4
    if q:
        b[K - q:] = (b[:q] + (r.randn(q, 4) * 2).astype(np.float32)).clip(0, side)
    return b


def scores_matrix(K, C, seed, tie_blocks=False):
    """fp32 scores in (0, 1), one column per class; tie_blocks: runs of 5 rows share exactly one score per class."""
    r = np.random.RandomState(seed + 1000)
    s = r.rand(K, C).astype(np.float32)
    if tie_blocks and K:
        s = s[(np.arange(K) // 5) * 5]
    return np.ascontiguousarray(s)


# ================================================================================================ IoU and greedy NMS
def iou_matrix(boxes, dtype=np.float32):
    b = np.asarray(boxes).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), dtype(0))
        ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), dtype(0))
        inter = iw * ih
        return inter / ((area[:, None] + area[None, :]) - inter)


def min_iou_margin(boxes, thr):
    """min |iou64 - fp32(thr)| over all pairs of different boxes (inf when there is none)."""
    u = iou_matrix(boxes, np.float64)
    np.fill_diagonal(u, np.nan)
    d = np.abs(u - float(np.float32(thr)))
    return float(np.nanmin(d)) if np.isfinite(d).any() else float("inf")


def greedy_nms(boxes, scores, iou_thr, dtype=np.float32, limit=None):
    """-> kept rows in greedy order: score descending, ties by ascending row; b is suppressed by a kept a iff iou(a, b) > iou_thr."""
    with np.errstate(invalid="ignore"):
        m = iou_matrix(boxes, dtype) > dtype(np.float32(iou_thr))
    return _greedy_on_mask(m, scores, limit)


def _greedy_on_mask(m, scores, limit=None):
    scores = np.asarray(scores)
    order = np.argsort(-scores, kind="stable")
    sup = np.zeros(len(scores), bool)
    keep = []
    for i in order:
        if sup[i]:
            continue
        keep.append(int(i))
        if limit is not None and len(keep) >= limit:
            break
        sup |= m[i]
    return keep


def batched_nms_offset(boxes, scores, idxs, iou_thr, dtype=np.float64):
    """mmcv's batched_nms: one NMS over boxes + idxs * (max coordinate + 1) -> kept rows, score descending (ties: ascending row)."""
    b = np.asarray(boxes).astype(dtype)
    off = np.asarray(idxs).astype(dtype) * (b.max() + dtype(1))
    return greedy_nms(b + off[:, None], scores, iou_thr, dtype)


def multiclass(boxes, scores, starts, Kmax, score_thr, iou_thr, max_num, group=None, G=0, dtype=np.float32):
    """The contract of include/clipself_det.h on numpy arrays: boxes [K, 4], scores [K, C] (foreground columns), starts [B + 1].
    -> dets [B, max_num, 5] f32, labels, inds [B, max_num] i32, counts [B] i32."""
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    K, C = scores.shape
    B = len(starts) - 1
    L = G if group is not None else C
    dets = np.zeros((B, max_num, 5), np.float32)
    labels, inds = np.full((B, max_num), -1, np.int32), np.full((B, max_num), -1, np.int32)
    counts = np.zeros(B, np.int32)
    thr = np.float32(score_thr)
    for b in range(B):
        s, e = min(max(int(starts[b]), 0), K), min(max(int(starts[b + 1]), 0), K)
        n = min(e - s, Kmax) if e > s else 0
        if n == 0:
            continue
        bx, sc = boxes[s:s + n], scores[s:s + n]
        with np.errstate(invalid="ignore"):
            mask = iou_matrix(bx, dtype) > dtype(np.float32(iou_thr))    # class-agnostic boxes: one matrix per image serves every list
        kept = []                                                     # (score, flat index, row, label)
        for l in range(L):
            col = sc[:, 0] if group is not None else sc[:, l]
            with np.errstate(invalid="ignore"):
                cand = col > thr
            if group is not None:
                cand = cand & (np.asarray(group)[s:s + n] == l)
            idx = np.nonzero(cand)[0]
            for j in _greedy_on_mask(mask[np.ix_(idx, idx)], col[idx], limit=max_num):
                k = int(idx[j])
                kept.append((float(col[k]), k if group is not None else k * C + l, k, l))
        kept.sort(key=lambda t: (-t[0], t[1]))
        kept = kept[:max_num]
        for r, (_, _, k, l) in enumerate(kept):
            dets[b, r, :4] = bx[k]
            dets[b, r, 4] = sc[k, 0] if group is not None else sc[k, l]
            labels[b, r], inds[b, r] = l, s + k
        counts[b] = len(kept)
    return dets, labels, inds, counts


# ================================================================================================ delta2bbox
def delta2bbox(rois, deltas, means, stds, wh_ratio_clip=16 / 1000, starts=None, max_shape=None, scale=None):
    """float64 evaluation on the fp32 inputs (means, stds, the clamp bound and the scale as the fp32 numbers the kernel receives).
    rois [K, 4], deltas [K, 4]; max_shape [B, 2] = (h, w), scale [B, 4] per image with starts [B + 1] -> (boxes [K, 4], bound [K, 4])."""
    r, dl = np.asarray(rois, np.float32).astype(np.float64), np.asarray(deltas, np.float32).astype(np.float64)
    mu, sd = np.asarray(means, np.float32).astype(np.float64), np.asarray(stds, np.float32).astype(np.float64)
    K = r.shape[0]
    max_ratio = float(np.float32(abs(np.log(float(np.float32(wh_ratio_clip))))))
    ds = dl * sd
    d = ds + mu
    e_d = U * (np.abs(ds) + np.abs(d))
    p = (r[:, :2] + r[:, 2:]) * 0.5
    w = r[:, 2:] - r[:, :2]
    t = w * d[:, :2]
    g = p + t
    e_g = U * np.abs(p) + 2 * U * np.abs(t) + np.abs(w) * e_d[:, :2] + U * np.abs(g)
    s = w * np.exp(np.clip(d[:, 2:], -max_ratio, max_ratio))
    c = np.concatenate([g - 0.5 * s, g + 0.5 * s], 1)
    e_s = 0.5 * np.abs(s) * (e_d[:, 2:] + 4 * U)
    e_c = np.concatenate([e_g + e_s, e_g + e_s], 1) + U * np.abs(c)
    if max_shape is not None or scale is not None:
        st = np.asarray(starts, np.int64)
        B = len(st) - 1
        img = np.searchsorted(st[1:B], np.arange(K), side="right") if B > 1 else np.zeros(K, np.int64)
        if max_shape is not None:
            hw = np.asarray(max_shape, np.float32).astype(np.float64).reshape(B, 2)[img]
            hi = np.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], 1)
            c = np.minimum(np.maximum(c, 0.0), hi)
        if scale is not None:
            sf = np.asarray(scale, np.float32).astype(np.float64).reshape(B, 4)[img]
            c = c / sf
            e_c = e_c / np.abs(sf) + U * np.abs(c)
    return c, e_c * (1 + 2.0 ** -10)


def delta2bbox_inputs(K, seed, side=512.0):
    """rois inside a side x side image and deltas at the scale of stds (0.1, 0.1, 0.2, 0.2); row 0 / 1 sit at +- the wh_ratio_clip clamp
    (|dwh * std| far above |log(16 / 1000)| = 4.135), rows 2 / 3 are pushed across the image border."""
    r = np.random.RandomState(seed)
    xy = r.rand(K, 2) * (side - 64)
    rois = np.concatenate([xy, xy + 8 + r.rand(K, 2) * 56], 1).astype(np.float32)
    deltas = (r.randn(K, 4) * np.array([2.0, 2.0, 3.0, 3.0])).astype(np.float32)
    if K > 3:
        deltas[0, 2:], deltas[1, 2:] = 60.0, -60.0
        deltas[2, :2], deltas[3, :2] = -2000.0, 2000.0                 # centre moved by 200 box sides (>= 1600 px)
    return rois, deltas


# ================================================================================================ the case table of the NMS tests
# name -> spec.  ns: boxes per image; lattice inputs unless lattice=False (then the caller asserts min_iou_margin() > 1e-5).
# The shapes are the smallest at which the kernels of det_post.hip take another path: 63 / 64 / 65 / 130 boxes = under, at and over one
# bitset word and two words; 1000 = several mask workgroups; 4100 = more than one bitset register per lane (the boundary is 4096 bits) and
# an image past the 2048 keys a wave sorts in LDS; C = 65 / 67 / 1203 = many lists; ragged batches with an empty image; max_num 1, 100 and
# more than everything kept; one class alone past max_num keeps (the early stop).
def _spec(ns, C=2, max_num=100, iou=0.5, thr=0.05, **kw):
    return dict(ns=tuple(ns), C=C, max_num=max_num, iou=iou, thr=thr, **kw)


NMS_CASES = {
    "n0": _spec([0]), "n1": _spec([1]), "n63": _spec([63]), "n64": _spec([64]), "n65": _spec([65]), "n130": _spec([130]),
    "n1000": _spec([1000]),
    "n4100_c1": _spec([4100], C=1, iou=0.7),
    "c1": _spec([130], C=1), "c65": _spec([130], C=65), "c67": _spec([130], C=67), "c1203_n40": _spec([40], C=1203, thr=0.5),
    "ragged_a": _spec([63, 130, 0]), "ragged_b": _spec([0, 130, 65], C=3, iou=0.4),
    "max1": _spec([130], max_num=1), "max_all": _spec([130], max_num=4096),
    "early_stop": _spec([1000], iou=0.7, max_num=20),
    "none_pass": _spec([130], thr=2.0),
    "ties": _spec([130], ties=True), "ties_c1_max7": _spec([65], C=1, ties=True, max_num=7, iou=0.9),
    "kmax_clamp": _spec([130, 40], Kmax=100),
    "neg_thr": _spec([65], thr=-0.25, shift=-0.5),
    "nonfinite": _spec([65], nonfinite=True),
    "rand65_iou0.4": _spec([65], iou=0.4, lattice=False, seed=0),
    "rand130_iou0.5": _spec([130], iou=0.5, lattice=False, seed=1),
    "rand130_iou0.7": _spec([130, 100], iou=0.7, lattice=False, seed=2),
    "group_small": _spec([130, 65], C=1, G=5, max_num=50, iou=0.7),
    # the RPN form: 2000 boxes of one image in one level (a list longer than 1024) + 40 in the others: sorted in LDS (2040 <= 2048 keys) ...
    "rpn2040": _spec([2040], C=1, G=5, big_level=(3, 2000), max_num=1000, iou=0.7),
    # ... and 2500 boxes: past the LDS share, the list sorts in the workspace
    "rpn2500": _spec([2500], C=1, G=5, big_level=(3, 2000), max_num=1000, iou=0.7),
}

_built, _expected = {}, {}


def build_case(name):
    """-> dict(boxes [K, 4], scores [K, C], starts [B + 1], Kmax, score_thr, iou_thr, max_num, group, G), numpy, memoised and read-only."""
    if name in _built:
        return _built[name]
    sp = NMS_CASES[name]
    ns, C, seed = sp["ns"], sp["C"], sp.get("seed", 0)
    gen = lattice_boxes if sp.get("lattice", True) else random_boxes
    boxes = np.concatenate([gen(n, seed + 17 * i) for i, n in enumerate(ns)] + [np.zeros((0, 4), np.float32)], 0)
    K = boxes.shape[0]
    scores = scores_matrix(K, C, seed, sp.get("ties", False)) + np.float32(sp.get("shift", 0.0))
    group, G = None, sp.get("G", 0)
    if G:
        r = np.random.RandomState(seed + 5)
        group = r.randint(0, G, K).astype(np.int32)
        if "big_level" in sp:
            lvl, cnt = sp["big_level"]
            group[:] = np.where(group == lvl, (lvl + 1) % G, group)
            group[r.permutation(K)[:cnt]] = lvl
        if K > 8:
            group[K // 2], group[K // 3] = -1, G                       # out of range: dropped
    if sp.get("nonfinite"):
        scores[3, 0], scores[7, :] = np.nan, np.nan                    # NaN scores: never candidates
        boxes[5] = np.nan                                              # NaN coordinates: kept, suppress nobody
        boxes[6, 2] = np.inf
        boxes[9] = (-np.inf, -np.inf, np.inf, np.inf)
        boxes[11, 2:] = boxes[11, :2]                                  # zero area
        boxes[12] = boxes[11]                                          # ... twice: 0 / 0
        scores[[5, 6, 9, 11, 12], :] = np.float32(0.99)
    starts = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    case = dict(boxes=boxes, scores=np.ascontiguousarray(scores, np.float32), starts=starts, Kmax=sp.get("Kmax", max(max(ns), 0)),
                score_thr=sp["thr"], iou_thr=sp["iou"], max_num=sp["max_num"], group=group, G=G)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _built[name] = case
    return case


def expected(name):
    """The float32 restatement's answer for a case, computed once."""
    if name not in _expected:
        c = build_case(name)
        _expected[name] = multiclass(c["boxes"], c["scores"], c["starts"], c["Kmax"], c["score_thr"], c["iou_thr"], c["max_num"], c["group"], c["G"])
    return _expected[name]


def compare(name, got, want=None):
    """got = (dets, labels, inds, counts) as numpy: exact equality of inds, labels, counts; bit equality of dets."""
    want = expected(name) if want is None else want
    d, l, i, c = (np.asarray(x) for x in got)
    assert np.array_equal(c, want[3]), f"{name}: counts {c.tolist()} != {want[3].tolist()}"
    assert np.array_equal(i, want[2]), f"{name}: inds differ at {np.argwhere(i != want[2])[:4].tolist()}"
    assert np.array_equal(l, want[1]), f"{name}: labels differ at {np.argwhere(l != want[1])[:4].tolist()}"
    db, wb = np.ascontiguousarray(d, np.float32).view(np.int32), want[0].view(np.int32)
    assert np.array_equal(db, wb), f"{name}: dets differ in bits at {np.argwhere(db != wb)[:4].tolist()}"
