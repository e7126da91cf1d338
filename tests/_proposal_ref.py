"""TEST INFRASTRUCTURE -- numpy restatement of the RPN proposal step the kernels of det_proposal.hip replace (include/clipself_rpn.h).

What is restated, by the published function names (mmdet 2.28.1; neither the package nor its source is available to this project, so this
boundary is parity-unpinned in the sense of DESIGN.md §3.13: the restatement follows the published sources as read, it was not run against
them):

  mmdet.models.dense_heads.rpn_head.RPNHead._get_bboxes_single:  per level, rpn_cls_score.permute(1, 2, 0).reshape(-1).sigmoid(),
      rpn_bbox_pred.permute(1, 2, 0).reshape(-1, 4), `if 0 < nms_pre < scores.shape[0]: ranked_scores, rank_inds = scores.sort(descending=True);
      topk_inds = rank_inds[:nms_pre]`, the gathers, level_ids = idx                                                          -> select
  mmdet.core.bbox.coder.delta_xywh_bbox_coder.delta2bbox (through bbox_coder.decode(anchors, rpn_bbox_pred, max_shape=img_shape))
                                                                                                      -> _nms_ref.delta2bbox, called by select
  RPNHead._bbox_post_process:  `if cfg.min_bbox_size >= 0: valid_mask = (w > cfg.min_bbox_size) & (h > cfg.min_bbox_size)`, then
      `dets, _ = batched_nms(proposals, scores, ids, cfg.nms)` and `dets[:cfg.max_per_img]`                  -> select's group, rpn_proposals

Selection works on the integer keys of the header (~ord(logit), NaN = 0xFFFFFFFF, ties to the lower anchor index) and is exact: anchor_inds,
starts and the row layout are compared for equality.

Bounds (u = 2^-24, the fp32 unit roundoff; no constant is tuned):
  score = 1 / (1 + e) or e / (1 + e), e = expf(-|x|).  The device library documents expf at 1 ulp = 2u relative.  fl(1 + e) errs by
    2u e + u (1 + e) <= 3u (1 + e); the division adds u; for x < 0 the numerator e adds 2u: relative 6u, as _loss_ref derives for the same
    expression.  Times (1 + 2^-10) for second-order terms, plus TINY = 2^-100 for an expf flushed to zero.
  box: _nms_ref.delta2bbox returns (want, bound) for the same arithmetic before the clamp to the image.  The clamp itself is exact, and a
    coordinate that lies past a border by more than its bound is that border on both sides: bound 0.  A row whose decode is exact in fp32 has bound 0: means 0,
    stds 1, dw = dh = 0, anchors on multiples of 1/4 below 2^12 and dx, dy on multiples of 1/16 with |d| <= 16 -- every intermediate is a
    multiple of 1/64 below 2^17, so each operation is exact and expf(0) = 1.
  The min-size filter compares extent = fl(x1 - x0) with min_bbox_size: its bound is eb = bound(x1) + bound(x0) + u |extent|.  A row with
    eb > 0 and |extent - min_bbox_size| <= eb (either axis) is in the undecided band and left out of the `group` comparison; an exact row
    (eb = 0) is always decided.  The tests assert from this file alone that their cases have no row in the band.

rpn_proposals continues with _nms_ref.multiclass (the contract of csd_nms' group form) on the fp32 roundings of the float64 boxes and
scores: exact on cases whose decode is exact and whose distinct scores are further apart than four score bounds (asserted by the tests).

CASES are generated from seeds; nothing is read from outside the repository.
"""
import numpy as np

import _nms_ref as N

U = 2.0 ** -24
TINY = 2.0 ** -100
NAN, INF = float("nan"), float("inf")


# ================================================================================================ keys and lists
def keys(x):
    """fp32 logits -> uint32 keys, smallest = best: ~ord(x); NaN -> 0xFFFFFFFF."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    o = np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000))
    k = ~o
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def list_logits(cls_l, b, plant=None):
    """cls [B, A, h, w] -> the n logits of image b in anchor order i = (y * w + x) * A + a."""
    if plant == "anchor_order":
        return np.ascontiguousarray(cls_l[b]).reshape(-1)                       # (a * h + y) * w + x
    return np.ascontiguousarray(cls_l[b].transpose(1, 2, 0)).reshape(-1)


def list_deltas(reg_l, b, A, plant=None):
    """reg [B, 4A, h, w] -> [n, 4]: delta j of anchor (y, x, a) is channel 4a + j."""
    _, h, w = reg_l[b].shape
    if plant == "reg_channel":
        return np.ascontiguousarray(reg_l[b].reshape(4, A, h, w).transpose(2, 3, 1, 0)).reshape(-1, 4)        # channel j * A + a
    r = reg_l[b].reshape(A, 4, h, w)
    if plant == "anchor_order":
        return np.ascontiguousarray(r.transpose(0, 2, 3, 1)).reshape(-1, 4)
    return np.ascontiguousarray(r.transpose(2, 3, 0, 1)).reshape(-1, 4)


def sigmoid64(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def score_bound(sig):
    with np.errstate(invalid="ignore"):
        return 6 * U * np.abs(sig) * (1 + 2.0 ** -10) + TINY


def _exact_rows(anchors, deltas, means, stds):
    """Rows whose fp32 decode is exact (module docstring)."""
    if tuple(float(v) for v in means) != (0.0,) * 4 or tuple(float(v) for v in stds) != (1.0,) * 4:
        return np.zeros(len(anchors), bool)
    a, d = anchors.astype(np.float64), deltas.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a).all(1) & np.isfinite(d).all(1)
        ok &= (np.abs(a) < 4096).all(1) & (a * 4 == np.round(a * 4)).all(1)
        ok &= (d[:, 2:] == 0).all(1) & (np.abs(d[:, :2]) <= 16).all(1) & (d[:, :2] * 16 == np.round(d[:, :2] * 16)).all(1)
    return ok


# ================================================================================================ select
def select(c, plant=None):
    """The contract of csp_select on a case dict (build_case) -> dict of
    anchor_inds [B, Ktot] i32, starts [B + 1] i32, score / score_bound [B, Ktot] f64, box / box_bound [B, Ktot, 4] f64,
    group [B, Ktot] i32, band [B, Ktot] bool (the filter is undecided), logit [B, Ktot] f32, ks (k_l per level)."""
    cls, reg, anchors = c["cls"], c["reg"], c["anchors"]
    L, B, A, pre = len(cls), cls[0].shape[0], cls[0].shape[1], c["nms_pre"]
    ns = [cl.shape[2] * cl.shape[3] * A for cl in cls]
    ks = [min(pre, n) for n in ns]
    Ktot = sum(ks)
    rows_i, rows_l, rows_x, rows_d = [], [], [], []
    for b in range(B):
        ri, rl, rx, rd = [], [], [], []
        anc0 = 0
        for l in range(L):
            x = list_logits(cls[l], b, plant)
            d = list_deltas(reg[l], b, A, plant)
            if plant == "score_select":                                            # mmdet's sort of the rounded score, made stable
                key = keys(sigmoid64(x).astype(np.float32))
            else:
                key = keys(x)
            order = np.argsort(key, kind="stable")                                 # ties by ascending anchor index
            k = ks[l]
            if plant == "tie_plus_one" and k < ns[l] and key[order[k]] == key[order[k - 1]]:
                k += 1
            order = order[:k]
            ri.append(order + anc0)
            rl.append(np.full(k, l))
            rx.append(x[order])
            rd.append(d[order])
            anc0 += ns[l]
        cat = lambda v: np.concatenate(v, 0)[:Ktot]
        rows_i.append(cat(ri)), rows_l.append(cat(rl)), rows_x.append(cat(rx)), rows_d.append(cat(rd))
    inds = np.stack(rows_i).astype(np.int32)
    lev = np.stack(rows_l).astype(np.int32)
    logit = np.stack(rows_x).astype(np.float32)
    deltas = np.stack(rows_d).astype(np.float32).reshape(B * Ktot, 4)
    rois = np.ascontiguousarray(anchors[:, :4][inds.reshape(-1)], np.float32)
    starts = (np.arange(B + 1) * Ktot).astype(np.int32)
    ms = None if (c["max_shape"] is None or plant == "no_clamp") else c["max_shape"]
    with np.errstate(invalid="ignore", over="ignore"):
        box, bb = N.delta2bbox(rois, deltas, c["means"], c["stds"], c["wh_ratio_clip"])
        bb = np.where(_exact_rows(rois, deltas, c["means"], c["stds"])[:, None], 0.0, bb)
        if ms is not None:                                                     # the clamp is exact; a coordinate past the border by more than
            hw = np.asarray(ms, np.float32).astype(np.float64)[np.repeat(np.arange(B), Ktot)]      # its bound is the border on both sides
            hi = np.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], 1)
            bb = np.where((box - bb >= hi) | (box + bb <= 0), 0.0, bb)
            box = np.minimum(np.maximum(box, 0.0), hi)
    sig = sigmoid64(logit)
    mn = float(np.float32(c["min_bbox_size"]))
    with np.errstate(invalid="ignore"):
        ext = np.stack([box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1)
        eb = np.stack([bb[:, 2] + bb[:, 0], bb[:, 3] + bb[:, 1]], 1)
        eb = np.where(eb > 0, eb + U * np.abs(ext), 0.0)
        if mn < 0:
            keep, band = np.ones(B * Ktot, bool), np.zeros(B * Ktot, bool)
        else:
            keep = ((ext >= mn) if plant == "ge_filter" else (ext > mn)).all(1)
            band = ((eb > 0) & (np.abs(ext - mn) <= eb)).any(1)
    group = np.where(keep, lev.reshape(-1), -1).astype(np.int32)
    return dict(anchor_inds=inds, starts=starts, score=sig, score_bound=score_bound(sig), box=box.reshape(B, Ktot, 4),
                box_bound=bb.reshape(B, Ktot, 4), group=group.reshape(B, Ktot), band=band.reshape(B, Ktot), logit=logit, ks=ks)


def check_select(want, got, who=""):
    """got = (boxes [B, Ktot, 4], scores [B, Ktot], group [B, Ktot], anchor_inds [B, Ktot][, starts]) as numpy -> list of problems,
    and prints the worst error / bound ratios."""
    boxes, scores, group, inds = (np.asarray(g) for g in got[:4])
    B, Ktot = want["anchor_inds"].shape
    bad = []
    if inds.shape != (B, Ktot) or boxes.shape != (B, Ktot, 4) or scores.shape != (B, Ktot) or group.shape != (B, Ktot):
        return [f"{who}: shapes {boxes.shape} {scores.shape} {group.shape} {inds.shape} for B = {B}, Ktot = {Ktot}"]
    if not np.array_equal(inds, want["anchor_inds"]):
        at = np.argwhere(inds != want["anchor_inds"])
        bad.append(f"{who}: anchor_inds differ in {len(at)} rows, first {at[:3].tolist()}: got {inds[tuple(at[0])]}, want {want['anchor_inds'][tuple(at[0])]}")
    if len(got) > 4 and got[4] is not None and not np.array_equal(np.asarray(got[4]), want["starts"]):
        bad.append(f"{who}: starts {np.asarray(got[4]).tolist()} != {want['starts'].tolist()}")
    dec = ~want["band"]
    if not np.array_equal(group[dec], want["group"][dec]):
        at = np.argwhere((group != want["group"]) & dec)
        bad.append(f"{who}: group differs in {len(at)} decided rows, first {at[:3].tolist()}")
    s64, w = scores.astype(np.float64), want["score"]
    with np.errstate(invalid="ignore"):
        nan_ok = np.isnan(s64) == np.isnan(w)
        err = np.where(np.isnan(w), 0.0, np.abs(s64 - w))
        ratio_s = float((err / want["score_bound"].clip(1e-300))[~np.isnan(w)].max()) if (~np.isnan(w)).any() else 0.0
    if not nan_ok.all() or not (err <= np.where(np.isnan(w), 0.0, want["score_bound"])).all():
        bad.append(f"{who}: scores outside the bound, worst err / bound {ratio_s:.3f}, NaN pattern equal: {bool(nan_ok.all())}")
    b64, wb, bb = boxes.astype(np.float64), want["box"], want["box_bound"]
    with np.errstate(invalid="ignore"):
        same = (b64 == wb) | (np.isnan(b64) & np.isnan(wb))
        errb = np.where(same, 0.0, np.abs(b64 - wb))
        fin = np.isfinite(errb)
        okb = same | (fin & (errb <= bb))
        ratio_b = float((errb[fin & ~same] / bb[fin & ~same].clip(1e-300)).max()) if (fin & ~same).any() else 0.0
    if not okb.all():
        at = np.argwhere(~okb)
        bad.append(f"{who}: boxes outside the bound in {len(at)} cells, first {at[:3].tolist()}, worst err / bound {ratio_b:.3f}")
    print(f"{who}: worst err / bound: score {ratio_s:.3f}, box {ratio_b:.3f}; rows {B * Ktot}, in the band {int(want['band'].sum())}")
    return bad


# ================================================================================================ end to end
def rpn_proposals(c, max_per_img, iou_thr, sel=None):
    """select + the group form of _nms_ref.multiclass (score_thr = -1, G = L, Kmax = Ktot) on the fp32 roundings.
    -> dets [B, max_per_img, 5] f32, counts, levels, anchor_inds [B, max_per_img] i32 (-1 past the count), score_bound [B, max_per_img]."""
    s = select(c) if sel is None else sel
    B, Ktot = s["anchor_inds"].shape
    boxes = s["box"].reshape(-1, 4).astype(np.float32)
    sc32 = s["score"].reshape(-1, 1).astype(np.float32)
    dets, labels, rows, counts = N.multiclass(boxes, sc32, s["starts"], Ktot, -1.0, iou_thr, max_per_img, s["group"].reshape(-1), len(c["cls"]))
    flat_inds, flat_sb = s["anchor_inds"].reshape(-1), s["score_bound"].reshape(-1)
    ainds = np.where(rows >= 0, flat_inds[np.maximum(rows, 0)], -1).astype(np.int32)
    sb = np.where(rows >= 0, flat_sb[np.maximum(rows, 0)], 0.0)
    return dets, counts, labels, ainds, sb


def check_proposals(want, got, who=""):
    """got = (proposals, counts, levels, anchor_inds) as numpy: counts, levels, anchor indices equal; boxes bit-equal; scores in the bound."""
    wd, wc, wl, wi, sb = want
    d, cnt, lev, ai = (np.asarray(g) for g in got)
    bad = []
    if not np.array_equal(cnt, wc):
        bad.append(f"{who}: counts {cnt.tolist()} != {wc.tolist()}")
    if not np.array_equal(lev, wl):
        bad.append(f"{who}: levels differ at {np.argwhere(lev != wl)[:3].tolist()}")
    if not np.array_equal(ai, wi):
        bad.append(f"{who}: anchor_inds differ at {np.argwhere(ai != wi)[:3].tolist()}")
    if d.shape != wd.shape or not np.array_equal(np.ascontiguousarray(d[..., :4], np.float32).view(np.int32), np.ascontiguousarray(wd[..., :4]).view(np.int32)):
        bad.append(f"{who}: proposal boxes differ in bits")
    elif not (np.abs(d[..., 4].astype(np.float64) - wd[..., 4].astype(np.float64)) <= sb + U * np.abs(wd[..., 4])).all():
        bad.append(f"{who}: the score column is outside its bound")
    return bad


def min_score_gap_ratio(s):
    """min over images of (smallest gap between two distinct scores) / (4 * the larger score bound of the pair); inf without a pair."""
    worst = INF
    for b in range(s["score"].shape[0]):
        v, bd = s["score"][b], s["score_bound"][b]
        keep = ~np.isnan(v)
        order = np.argsort(v[keep], kind="stable")
        v, bd = v[keep][order], bd[keep][order]
        gap = np.diff(v)
        pos = gap > 0
        if pos.any():
            worst = min(worst, float((gap[pos] / (4 * np.maximum(bd[1:], bd[:-1])[pos])).min()))
    return worst


# ================================================================================================ generators
def lattice_anchors(n, seed, side=512):
    """x0, y0 on multiples of 1/4, sides on multiples of 4 in [8, 160]; the last quarter are copies of the first quarter moved by up to
    2 px on the lattice.  With deltas of zero or dx, dy on multiples of 1/16 (dw = dh = 0) every decoded coordinate is a multiple of 1/4 in
    [0, side] after the clamp: areas, intersections and unions are exact in fp32 (_nms_ref.lattice_boxes)."""
    r = np.random.RandomState(seed)
    x0, y0 = r.randint(0, (side - 64) * 4, n) / 4.0, r.randint(0, (side - 64) * 4, n) / 4.0
    w, h = r.randint(2, 41, n) * 4.0, r.randint(2, 41, n) * 4.0
    q = n // 4
    if q:
        x0[n - q:] = x0[:q] + r.randint(-8, 9, q) / 4.0
        y0[n - q:] = y0[:q] + r.randint(-8, 9, q) / 4.0
        w[n - q:], h[n - q:] = w[:q], h[:q]
    return np.stack([x0, y0, x0 + w, y0 + h], 1).astype(np.float32)


def _logits(kind, shape, r, pre):
    n = int(np.prod(shape))
    if kind == "rand":
        x = (r.randn(n) * 3).astype(np.float32)
    elif kind == "equal":
        x = np.full(n, 0.37, np.float32)
    elif kind == "tierun":                                 # a run of equal logits straddling the k-th place
        x = (r.randn(n) * 3).astype(np.float32)
        k = min(pre, n)
        v = np.sort(x)[::-1][k - 1]
        x[r.permutation(n)[:max(2, min(n, 9))]] = v
    elif kind == "lowbits":                                # differ only in the lowest 8 mantissa bits
        x = (np.uint32(0x3FC00000) | r.randint(0, 256, n).astype(np.uint32)).view(np.float32)
    elif kind == "signexp":                                # differ only in sign and exponent
        x = ((r.randint(0, 2, n).astype(np.uint32) << 31) | (r.randint(90, 160, n).astype(np.uint32) << 23)).view(np.float32)
    elif kind == "special":
        x = (r.randn(n) * 3).astype(np.float32)
        sp = np.array([0.0, -0.0, INF, -INF, NAN, 17.5, 18.0, 40.0, 88.0, 1e30, -1e30, -104.0, 0.0, -0.0, NAN, INF], np.float32)
        x[r.permutation(n)[:min(n, len(sp))]] = sp[:min(n, len(sp))]
        if n > 20:
            x[r.permutation(n)[:2]] = np.array([0xFFC00001, 0x7F800001], np.uint32).view(np.float32)          # NaNs of both signs
    elif kind == "lattice":                                # k / 64, |k| <= 512: neighbouring scores differ by >= (1 / 64)(1 - sigmoid(8))
        x = (r.randint(-512, 513, n) / 64.0).astype(np.float32)
    elif kind == "saturated":                              # distinct logits above 17, descending index = ascending logit: all scores are 1
        x = (18.0 + np.arange(n) / 16.0).astype(np.float32)
    else:
        raise KeyError(kind)
    return x.reshape(shape)


def _spec(levels, A=1, B=1, pre=7, logits="rand", deltas="rand", anchors="rand", min_size=0.0, clamp=True, seed=0, stds=(1.0, 1.0, 1.0, 1.0),
          means=(0.0, 0.0, 0.0, 0.0)):
    return dict(levels=tuple(levels), A=A, B=B, pre=pre, logits=logits, deltas=deltas, anchors=anchors, min_size=min_size, clamp=clamp, seed=seed,
                stds=stds, means=means)


# Select-only cases.  List lengths at which det_proposal.hip changes path: n = nms_pre (a list no longer than nms_pre skips the select and is
# only sorted), n = 2048 (one or two workgroups per list in the select passes) and k = 2048 (one or two rounds of the 1024 sorting
# threads).  1999 = nms_pre - 1 for nms_pre = 2000 is a prime above 512 and no h * w * A inside the limits: 1998 stands in; 2049 = 3 * 683
# likewise: 2050 stands in.
SELECT_CASES = {
    "pre1_n1": _spec([(1, 1)], pre=1), "pre1_n2": _spec([(1, 2)], pre=1),
    "pre7_n6": _spec([(1, 2)], A=3, pre=7), "pre7_n7": _spec([(7, 1)], pre=7), "pre7_n8": _spec([(2, 2)], A=2, pre=7),
    "pre64_n63": _spec([(3, 7)], A=3, pre=64), "pre64_n64": _spec([(8, 8)], pre=64), "pre64_n65": _spec([(5, 13)], pre=64),
    "pre2000_n1998": _spec([(27, 37)], A=2, pre=2000), "pre2000_n2000": _spec([(20, 20)], A=5, pre=2000),
    "pre2000_n2001": _spec([(23, 29)], A=3, pre=2000),
    "g5x7_a3": _spec([(5, 7)], A=3, pre=20), "g7x5_a3": _spec([(7, 5)], A=3, pre=20), "g3x16_a1": _spec([(3, 16)], A=1, pre=20),
    "ragged5": _spec([(64, 64), (31, 33), (16, 15), (8, 9), (3, 4)], A=3, pre=300, seed=3, stds=(0.5, 0.5, 0.25, 0.25), means=(0.01, -0.02, 0.0, 0.03)),
    "b3": _spec([(13, 17), (6, 9)], A=3, B=3, pre=100, seed=4),
    "equal": _spec([(30, 23)], A=3, B=2, pre=64, logits="equal"),
    "tierun": _spec([(30, 23)], A=3, B=2, pre=64, logits="tierun", seed=5),
    "tierun_short": _spec([(5, 4)], A=3, pre=64, logits="tierun", seed=6),
    "tierun2": _spec([(30, 23), (9, 8)], A=3, pre=64, logits="tierun", seed=18),
    "equal2": _spec([(9, 8), (9, 8)], A=3, pre=64, logits="equal", seed=19),
    "lowbits": _spec([(30, 23)], A=3, pre=100, logits="lowbits", seed=7),
    "signexp": _spec([(30, 23)], A=3, pre=100, logits="signexp", seed=8),
    "special": _spec([(30, 23), (2, 3)], A=3, B=2, pre=2000, logits="special", seed=9),
    "special_long": _spec([(30, 23)], A=3, pre=2065, logits="special", seed=10),
    "n2048_pre64": _spec([(32, 64)], pre=64, seed=11), "n2050_pre64": _spec([(25, 41)], A=2, pre=64, seed=12),
    "n4096_pre4096": _spec([(64, 64)], pre=4096, seed=13), "n4097_pre4096": _spec([(17, 241)], pre=4096, seed=14),
    "n2050_pre2049": _spec([(25, 41)], A=2, pre=2049, seed=15),
    "noclamp_nofilter": _spec([(9, 11)], A=3, B=2, pre=50, clamp=False, min_size=-1.0, seed=16),
    "minsize": _spec([(9, 11)], A=3, B=2, pre=50, min_size=16.0, seed=17),
}

# End-to-end cases: lattice logits, lattice anchors, deltas of zero or dyadic shifts with dw = dh = 0 (the decode is exact).
E2E_CASES = {
    "e2e_small": dict(_spec([(12, 10), (6, 5), (3, 3)], A=3, B=2, pre=120, logits="lattice", deltas="shift", anchors="lattice", seed=20),
                      max_per_img=60, iou=0.7),
    "e2e_cut": dict(_spec([(12, 10), (6, 5)], A=3, B=3, pre=2000, logits="lattice", deltas="shift", anchors="lattice", seed=21),
                    max_per_img=25, iou=0.5),
    "e2e_zero": dict(_spec([(30, 23), (4, 5)], A=3, B=1, pre=150, logits="lattice", deltas="zero", anchors="lattice", min_size=16.0, seed=22),
                     max_per_img=100, iou=0.7),
}

_built, _selected = {}, {}


def build_case(name):
    """-> dict(cls [L][B, A, h, w], reg [L][B, 4A, h, w], anchors [N, 4], max_shape [B, 2] or None, nms_pre, means, stds, wh_ratio_clip,
    min_bbox_size), numpy fp32, memoised and read-only."""
    if name in _built:
        return _built[name]
    sp = SELECT_CASES.get(name) or E2E_CASES[name]
    r = np.random.RandomState(1000 + sp["seed"])
    A, B = sp["A"], sp["B"]
    cls, reg, anc = [], [], []
    for (h, w) in sp["levels"]:
        cls.append(np.ascontiguousarray(_logits(sp["logits"], (B, A, h, w), r, sp["pre"])))
        if sp["deltas"] == "rand":
            d = (r.randn(B, 4 * A, h, w) * 0.5).astype(np.float32)
        elif sp["deltas"] == "zero":
            d = np.zeros((B, 4 * A, h, w), np.float32)
        else:                                              # dx, dy on multiples of 1/16 in [-1/2, 1/2], dw = dh = 0
            d = (r.randint(-8, 9, (B, A, 4, h, w)) / 16.0).astype(np.float32)
            d[:, :, 2:] = 0
            d = d.reshape(B, 4 * A, h, w)
        reg.append(np.ascontiguousarray(d))
        n = h * w * A
        if sp["anchors"] == "lattice":
            anc.append(lattice_anchors(n, r.randint(1 << 30)))
        else:
            xy = r.rand(n, 2) * 480
            anc.append(np.concatenate([xy, xy + 6 + r.rand(n, 2) * 120], 1).astype(np.float32))
    max_shape = np.array([[400.0 + 16 * b, 512.0 - 32 * b] for b in range(B)], np.float32) if sp["clamp"] else None
    case = dict(cls=cls, reg=reg, anchors=np.concatenate(anc, 0), max_shape=max_shape, nms_pre=sp["pre"], means=sp["means"], stds=sp["stds"],
                wh_ratio_clip=16 / 1000, min_bbox_size=sp["min_size"])
    for v in cls + reg + [case["anchors"], max_shape]:
        if v is not None:
            v.setflags(write=False)
    _built[name] = case
    return case


def expected(name):
    """select() of a case, computed once."""
    if name not in _selected:
        _selected[name] = select(build_case(name))
    return _selected[name]
