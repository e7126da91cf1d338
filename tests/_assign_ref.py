"""numpy restatement of include/clipself_assign.h: IoU assignment, sampling, box-delta targets (test infrastructure, not product code).

PARITY-UNPINNED: mmcv / mmdet are not available to this project, so nothing here was run against them.  The functions restate the
published mmdet 2.x sources as read: `bbox_overlaps` (mode 'iou', eps 1e-6), `MaxIoUAssigner.assign` -> `assign_wrt_overlaps`,
`AssignResult.add_gt_`, `RandomSampler.sample` (`_sample_pos`, `_sample_neg`, `random_choice`), `bbox2delta`,
`AnchorHead._get_targets_single` + `unmap`, `BBoxHead._get_target_single`, `AnchorGenerator.grid_priors`.  Where the header differs from
mmdet it says so (a NaN IoU counts as 0; the sampler takes the smallest (key, row) pairs instead of a randperm prefix).

Everything is np.float32 operation by operation, so every intermediate is a rounded fp32 number, exactly what the header prescribes.
Two forms of the assignment and of the sampler: `*_scalar` transcribes mmdet's control flow literally (Python loops, the sequential
`for i in range(num_gts)`), `*_vec` is vectorised; tests/test_det_targets_cpu.py tests one against the other.

dw, dh: the bound of `delta_bound`.  The host forms take libm's double log and round it once to fp32; the device calls logf, which ROCm's
device library documents at 1 ulp.  With u = 2^-24 (fp32 unit roundoff), v = fl(gw / pw) (the same fp32 number on both sides, an IEEE
division), L = log(v), S = L - mean, T = S / std in exact arithmetic on the fp32 values mean, std:
    |l - L| <= ulp(l) <= 2u |L| (1 + 2u) =: eL            the device logf; eL = 0 when v == 1 (logf(1) = 0 exactly)
    s = fl(l - mean):  |s - S| <= eL + u (|S| + eL) =: eS
    t = fl(s / std):   |t - T| <= eS / |std| + u (|T| + eS / |std|)
That is the per-element bound the GPU test holds |device - T64| to, T64 being T evaluated in float64 (whose own error, ~1e-16 relative, is
below 1e-8 of the bound).  It is derived, not measured; profiles/det_targets_parity.md records the worst measured fraction of it.
"""
import functools
import math

import numpy as np

F = np.float32
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ layout
def rng_of(tab, b, total, cap):
    """rows (s, n) of image b: starts / gt_starts clamped as the header says; tab None = the shared form"""
    if tab is None:
        return 0, min(total, cap)
    s, e = min(max(int(tab[b]), 0), total), min(max(int(tab[b + 1]), 0), total)
    return s, (min(e - s, cap) if e > s else 0)


# ------------------------------------------------------------------------------------------------ IoU
def iou_scalar(a, g):
    """bbox_overlaps for one pair, np.float32 scalars, one operation at a time"""
    with np.errstate(all="ignore"):
        area_a = F(F(a[2] - a[0]) * F(a[3] - a[1]))
        area_g = F(F(g[2] - g[0]) * F(g[3] - g[1]))
        w = np.maximum(F(np.minimum(a[2], g[2]) - np.maximum(a[0], g[0])), F(0))
        h = np.maximum(F(np.minimum(a[3], g[3]) - np.maximum(a[1], g[1])), F(0))
        inter = F(w * h)
        union = np.maximum(F(F(area_a + area_g) - inter), F(1e-6))
        v = F(inter / union)
    return F(0) if np.isnan(v) else v


def iou_matrix(gts, boxes):
    """[G, 4] x [N, 4] -> [G, N] fp32, NaN -> 0"""
    gts, boxes = np.asarray(gts, F).reshape(-1, 4), np.asarray(boxes, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area_g = (gts[:, 2] - gts[:, 0]) * (gts[:, 3] - gts[:, 1])
        area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        w = np.maximum(np.minimum(gts[:, None, 2], boxes[None, :, 2]) - np.maximum(gts[:, None, 0], boxes[None, :, 0]), F(0))
        h = np.maximum(np.minimum(gts[:, None, 3], boxes[None, :, 3]) - np.maximum(gts[:, None, 1], boxes[None, :, 1]), F(0))
        inter = w * h
        union = np.maximum((area_b[None, :] + area_g[:, None]) - inter, F(1e-6))
        v = inter / union
    assert v.dtype == F
    return np.where(np.isnan(v), F(0), v)


# ------------------------------------------------------------------------------------------------ assignment
def _thr(p):
    neg = p["neg"]
    lo, hi = neg if isinstance(neg, tuple) else (0.0, neg)
    return F(p["pos"]), F(lo), F(hi), F(p["min_pos"])


def assign_image_vec(boxes, ok, gts, p):
    """one image: boxes [n, 4], ok [n] bool, gts [g, 4] -> gt_inds [n] int32, max_overlaps [n] fp32"""
    n, g = len(boxes), len(gts)
    pos, lo, hi, min_pos = _thr(p)
    rows = np.arange(n)
    pref = (rows < g) if p["prefix"] else np.zeros(n, bool)
    act = ok & ~pref
    gi, mo = np.full(n, -1, np.int32), np.zeros(n, F)
    if g == 0:
        gi[ok] = 0
        return gi, mo
    if act.any():
        ov = iou_matrix(gts, boxes[act])
        mx = ov.max(axis=0)
        arg = ov.argmax(axis=0)                            # numpy's argmax returns the first maximum: the lowest ground truth
        a = np.full(len(mx), -1, np.int32)
        a[(mx >= lo) & (mx < hi)] = 0
        a[mx >= pos] = arg[mx >= pos] + 1
        if p["mlq"]:
            gt_mx = ov.max(axis=1)
            hit = (ov == gt_mx[:, None]) & (gt_mx >= min_pos)[:, None]
            if not p["all"]:
                first = hit.argmax(axis=1)
                only = np.zeros_like(hit)
                only[np.arange(g), first] = hit[np.arange(g), first]
                hit = only
            last = np.where(hit, np.arange(g)[:, None], -1).max(axis=0)          # later ground truths overwrite earlier ones
            a[last >= 0] = last[last >= 0] + 1
        gi[act], mo[act] = a, mx
    gi[pref & ok], mo[pref & ok] = rows[pref & ok] + 1, F(1)
    return gi, mo


def assign_image_scalar(boxes, ok, gts, p):
    """the same, transcribing assign_wrt_overlaps literally"""
    n, g = len(boxes), len(gts)
    pos, lo, hi, min_pos = _thr(p)
    gi, mo = np.full(n, -1, np.int32), np.zeros(n, F)
    act = [r for r in range(n) if ok[r] and not (p["prefix"] and r < g)]
    if g == 0:
        for r in range(n):
            if ok[r]:
                gi[r] = 0
        return gi, mo
    overlaps = [[iou_scalar(boxes[r], gts[i]) for r in act] for i in range(g)]
    assigned = [-1] * len(act)
    for c in range(len(act)):
        mx, arg = F(-1), 0
        for i in range(g):
            if overlaps[i][c] > mx:
                mx, arg = overlaps[i][c], i
        mo[act[c]] = mx
        if lo <= mx < hi:
            assigned[c] = 0
        if mx >= pos:
            assigned[c] = arg + 1
    if p["mlq"] and act:
        for i in range(g):
            gt_max = max(overlaps[i])
            if gt_max >= min_pos:
                if p["all"]:
                    for c in range(len(act)):
                        if overlaps[i][c] == gt_max:
                            assigned[c] = i + 1
                else:
                    assigned[overlaps[i].index(gt_max)] = i + 1
    for c, r in enumerate(act):
        gi[r] = assigned[c]
    for r in range(n):
        if p["prefix"] and r < g and ok[r]:
            gi[r], mo[r] = r + 1, F(1)
    return gi, mo


def assign(c, form="vec"):
    """a case -> gt_inds [B, Nmax] int32, max_overlaps [B, Nmax] fp32"""
    fn = assign_image_vec if form == "vec" else assign_image_scalar
    B, Nmax = c["B"], c["Nmax"]
    gt_inds, max_ov = np.full((B, Nmax), -1, np.int32), np.zeros((B, Nmax), F)
    K, Gtot = len(c["boxes"]), len(c["gts"])
    for b in range(B):
        s, n = rng_of(c["starts"], b, K, Nmax)
        gs, g = rng_of(c["gt_starts"], b, Gtot, c["Gmax"])
        ok = np.ones(n, bool) if c["valid"] is None else c["valid"][s:s + n] != 0
        gt_inds[b, :n], max_ov[b, :n] = fn(c["boxes"][s:s + n], ok, c["gts"][gs:gs + g], c["assigner"])
    return gt_inds, max_ov


# ------------------------------------------------------------------------------------------------ sampling
def _choose_vec(pool, keys, want):
    if want <= 0:
        return pool[:0]
    if len(pool) <= want:
        return pool
    order = np.lexsort((pool, keys[pool].astype(np.uint64)))[:want]
    return np.sort(pool[order])


def _choose_scalar(pool, keys, want):
    if want <= 0:
        return pool[:0]
    pairs = sorted((int(keys[r]), int(r)) for r in pool)
    return np.array(sorted(r for _, r in pairs[:want]), dtype=np.int64)


def sample(gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, ub, form="vec"):
    """-> flags [B, Nmax] uint8, sel [B, num] int32, counts [B, 2] int32"""
    choose = _choose_vec if form == "vec" else _choose_scalar
    B, Nmax = gt_inds.shape
    flags, sel, counts = np.zeros((B, Nmax), np.uint8), np.full((B, num), -1, np.int32), np.zeros((B, 2), np.int32)
    for b in range(B):
        _, n = rng_of(starts, b, K, Nmax)
        _, g = rng_of(gt_starts, b, Gtot, Gmax)
        gi, key = gt_inds[b, :n].astype(np.int64), np.asarray(keys[b, :n]).astype(np.uint32)
        pos = choose(np.nonzero((gi > 0) & (gi <= g))[0], key, min(max(expected_pos, 0), num))
        want_neg = num - len(pos)
        if ub >= 0:
            cap = F(F(ub) * F(max(1, len(pos))))
            if cap < F(want_neg):
                want_neg = int(cap)
        neg = choose(np.nonzero(gi == 0)[0], key, want_neg)
        flags[b, pos], flags[b, neg] = 1, 2
        sel[b, :len(pos)], sel[b, len(pos):len(pos) + len(neg)] = pos, neg
        counts[b] = (len(pos), len(neg))
    return flags, sel, counts


# ------------------------------------------------------------------------------------------------ targets
def host_log(v):
    """libm's double log of fp32 values, rounded once to fp32 (0 -> -inf, negative or NaN -> NaN)"""
    out = [float("nan") if (x != x or x < 0) else float("-inf") if x == 0 else float("inf") if x == float("inf") else math.log(x)
           for x in np.asarray(v, np.float64).reshape(-1).tolist()]
    return np.array(out, np.float64).astype(F).reshape(np.shape(v))


def bbox2delta(p, g, means, stds):
    """mmdet's bbox2delta, fp32 op by op -> (deltas fp32 [n, 4], T64 [n, 4], bound [n, 4]); T64 / bound are meaningful for columns 2, 3"""
    p, g = np.asarray(p, F).reshape(-1, 4), np.asarray(g, F).reshape(-1, 4)
    means, stds = np.asarray(means, F), np.asarray(stds, F)
    with np.errstate(all="ignore"):
        pxy, pwh = (p[:, :2] + p[:, 2:]) * F(0.5), p[:, 2:] - p[:, :2]
        gxy, gwh = (g[:, :2] + g[:, 2:]) * F(0.5), g[:, 2:] - g[:, :2]
        ratio = gwh / pwh
        d = np.concatenate([(gxy - pxy) / pwh, host_log(ratio)], axis=1)
        out = (d - means) / stds
        assert out.dtype == F
        L = np.log(ratio.astype(np.float64))
        m64, s64 = means[2:].astype(np.float64), stds[2:].astype(np.float64)
        S = L - m64
        T = S / s64
        eL = 2 * U * np.abs(L) * (1 + 2 * U)
        eS = eL + U * (np.abs(S) + eL)
        bound = eS / np.abs(s64) + U * (np.abs(T) + eS / np.abs(s64))
    z = np.zeros_like(T)
    return out, np.concatenate([z, T], axis=1), np.concatenate([z, bound], axis=1)


def targets(c, gt_inds, flags=None, sel=None):
    """csa_targets: dense (sel None) or compact -> dict of arrays; 't64' / 'bound' for the dw, dh columns of positives, 'pos' [B, S] bool, 'unit'
    [B, S, 4] bool: the dw / dh whose gwh == pwh"""
    B, Nmax = gt_inds.shape
    K, Gtot = len(c["boxes"]), len(c["gts"])
    S = Nmax if sel is None else sel.shape[1]
    out = dict(labels=np.full((B, S), c["bg_label"], np.int32), label_weights=np.zeros((B, S), F), bbox_targets=np.zeros((B, S, 4), F),
               bbox_weights=np.zeros((B, S, 4), F), t64=np.zeros((B, S, 4)), bound=np.zeros((B, S, 4)), pos=np.zeros((B, S), bool),
               unit=np.zeros((B, S, 4), bool))
    if sel is not None:
        out["rois"] = np.zeros((B, S, 5), F)
        out["rois"][:, :, 0] = -1
    for b in range(B):
        s, n = rng_of(c["starts"], b, K, Nmax)
        gs, g = rng_of(c["gt_starts"], b, Gtot, c["Gmax"])
        for t in range(S):
            row = t if sel is None else int(sel[b, t])
            sampled = (0 <= row < n) and (sel is not None or flags[b, row] != 0)
            if not sampled:
                continue
            gi = int(gt_inds[b, row])
            if gi < -1 or gi > g:
                gi = -1
            pos = gi > 0 and (sel is not None or flags[b, row] == 1)
            out["label_weights"][b, t] = 1
            if sel is not None:
                out["rois"][b, t, 0] = b
                out["rois"][b, t, 1:] = c["boxes"][s + row]
            if pos:
                out["labels"][b, t] = 0 if c["gt_labels"] is None else c["gt_labels"][gs + gi - 1]
                d, t64, bound = bbox2delta(c["boxes"][s + row], c["gts"][gs + gi - 1], c["means"], c["stds"])
                out["bbox_targets"][b, t], out["t64"][b, t], out["bound"][b, t] = d[0], t64[0], bound[0]
                out["bbox_weights"][b, t] = 1
                out["pos"][b, t] = True
                pb, gb = c["boxes"][s + row], c["gts"][gs + gi - 1]
                out["unit"][b, t, 2:] = (gb[2:] - gb[:2]) == (pb[2:] - pb[:2])      # gwh == pwh: the ratio is 1 and its log exactly 0
    return out


# ------------------------------------------------------------------------------------------------ anchors
def anchors_np(featmap_sizes, strides=(4, 8, 16, 32, 64), scale=8.0, ratios=(0.5, 1.0, 2.0)):
    """AnchorGenerator(strides, ratios, scales=[scale]).grid_priors, all levels concatenated: location-major, base anchors innermost"""
    out = []
    for (fh, fw), st in zip(featmap_sizes, strides):
        hr = np.sqrt(np.asarray(ratios, F))
        wr = F(1) / hr
        ws, hs = F(st) * wr * F(scale), F(st) * hr * F(scale)
        base = np.stack([F(0) - F(0.5) * ws, F(0) - F(0.5) * hs, F(0) + F(0.5) * ws, F(0) + F(0.5) * hs], axis=-1).astype(F)
        xs, ys = (np.arange(fw) * st).astype(F), (np.arange(fh) * st).astype(F)
        xx, yy = np.tile(xs, fh), np.repeat(ys, fw)
        shifts = np.stack([xx, yy, xx, yy], axis=-1)
        out.append((base[None] + shifts[:, None]).reshape(-1, 4))
    return np.concatenate(out).astype(F)


# ------------------------------------------------------------------------------------------------ cases
RPN = dict(pos=0.7, neg=0.3, min_pos=0.3, mlq=True, all=True, prefix=False)
RPN_FIRST = dict(RPN, all=False)
RCNN = dict(pos=0.5, neg=0.5, min_pos=0.5, mlq=False, all=True, prefix=False)
RCNN_PREFIX = dict(RCNN, prefix=True)
BAND = dict(pos=0.6, neg=(0.1, 0.4), min_pos=0.0, mlq=True, all=True, prefix=False)      # the tuple form; min_pos_iou = 0

LATTICE_GTS = [[0, 0, 10, 10], [0, 0, 10, 10],            # 0, 1 identical: argmax -> 0, the low-quality match -> 1 (later)
               [100, 100, 120, 120],                      # 2: a box at IoU exactly 0.5
               [200, 200, 220, 220],                      # 3: two boxes share its maximum 0.5
               [300, 300, 310, 310],                      # 4: a box at 7/10
               [400, 400, 420, 420], [410, 400, 430, 420],  # 5, 6: one box is the maximum of both (0.6 each)
               [500, 500, 520, 520], [500, 505, 520, 525],  # 7, 8: a 0.9 positive of 7 that is 8's only (low-quality) match
               [700, 700, 700, 700]]                      # 9: zero area
LATTICE_BOXES = [[0, 0, 10, 8],                           # 0.8 with gts 0 and 1
                 [100, 100, 120, 110],                    # 0.5 with 2
                 [200, 200, 210, 220], [210, 200, 220, 220],  # 0.5 and 0.5 with 3
                 [300, 300, 310, 307],                    # 0.7f with 4
                 [405, 400, 425, 420],                    # 0.6 with 5 and 6
                 [500, 500, 520, 518],                    # 0.9 with 7, 0.52 with 8
                 [600, 600, 600, 610],                    # zero area
                 [900, 900, 910, 910],                    # far away
                 [0, 0, 20, 10],                          # 0.5 with 0 / 1: below 0.8
                 [700, 700, 700, 700]]                    # zero area on the zero-area gt


def _case(boxes, gts, gt_starts, assigner, *, starts=None, valid=None, gt_labels=None, B=1, Nmax=None, Gmax=None, num=16, frac=0.5, ub=-1.0,
          means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), bg_label=1, seed=0, keys=None):
    boxes, gts = np.asarray(boxes, F).reshape(-1, 4), np.asarray(gts, F).reshape(-1, 4)
    if Nmax is None:
        Nmax = len(boxes) if starts is None else max([starts[b + 1] - starts[b] for b in range(B)] + [0])
    if Gmax is None:
        Gmax = max([gt_starts[b + 1] - gt_starts[b] for b in range(B)] + [0])
    if keys is None:
        keys = np.random.default_rng(1000 + seed).integers(0, 1 << 32, size=(B, Nmax), dtype=np.uint64).astype(np.uint32)
    return dict(boxes=boxes, starts=starts, gts=gts, gt_starts=list(gt_starts), gt_labels=None if gt_labels is None else np.asarray(gt_labels, np.int32),
                valid=None if valid is None else np.asarray(valid, np.uint8), B=B, Nmax=Nmax, Gmax=Gmax, assigner=assigner, num=num,
                expected_pos=int(num * frac), ub=float(ub), keys=keys, means=means, stds=stds, bg_label=bg_label)


def _random_boxes(rng, n, gts, side=256.0):
    """half jittered copies of ground truths (high IoUs), half anywhere; real corners"""
    xy = rng.uniform(0, side * 0.8, size=(n, 2))
    wh = rng.uniform(4, side * 0.4, size=(n, 2))
    out = np.concatenate([xy, xy + wh], axis=1)
    if len(gts):
        pick = rng.integers(0, len(gts), size=n)
        jit = gts[pick] + rng.normal(0, 3.0, size=(n, 4))
        near = rng.random(n) < 0.5
        good = near & (jit[:, 2] > jit[:, 0] + 1) & (jit[:, 3] > jit[:, 1] + 1)
        out[good] = jit[good]
    return out.astype(F)


def _random_gts(rng, g, side=256.0):
    xy = rng.uniform(0, side * 0.7, size=(g, 2))
    wh = rng.uniform(8, side * 0.3, size=(g, 2))
    return np.concatenate([xy, xy + wh], axis=1).astype(F)


def _random_case(seed, ns, gs, assigner, shared=False, mask=False, **kw):
    rng = np.random.default_rng(seed)
    B = len(gs)
    gts = [_random_gts(rng, g) for g in gs]
    gt_starts = np.concatenate([[0], np.cumsum(gs)]).tolist()
    if shared:
        allg = np.concatenate(gts) if sum(gs) else np.zeros((0, 4), F)
        boxes, starts = _random_boxes(rng, ns, allg), None
    else:
        parts = []
        for b in range(B):
            bx = _random_boxes(rng, ns[b], gts[b])
            if assigner["prefix"]:
                bx = np.concatenate([gts[b], bx])
            parts.append(bx)
        boxes = np.concatenate(parts)
        starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    gcat = np.concatenate(gts) if sum(gs) else np.zeros((0, 4), F)
    valid = (rng.random(len(boxes)) < 0.8).astype(np.uint8) if mask else None
    labels = rng.integers(0, 65, size=len(gcat))
    return _case(boxes, gcat, gt_starts, assigner, starts=starts, valid=valid, gt_labels=labels, B=B, seed=seed, **kw)


def _lattice(assigner, **kw):
    return _case(LATTICE_BOXES, LATTICE_GTS, [0, len(LATTICE_GTS)], assigner, gt_labels=np.arange(10) + 20, **kw)


def _anchor_case(seed, gs):
    rng = np.random.default_rng(seed)
    anchors = anchors_np([(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)])
    gts = [_random_gts(rng, g, side=64.0) for g in gs]
    valid = np.ones(len(anchors), np.uint8)
    valid[rng.integers(0, len(anchors), size=40)] = 0
    return _case(anchors, np.concatenate(gts), np.concatenate([[0], np.cumsum(gs)]).tolist(), RPN, valid=valid, B=len(gs), num=256, seed=seed)


def _hostile_tables():
    c = _random_case(31, [50, 40, 30], [4, 3, 5], RPN, num=12)
    # K = 120, Gtot = 12.  image 0: rows [0, 30) (the -5 is clamped); 1: non-monotone, empty; 2: [20, 120) cut to Nmax; 3: past K, empty
    c["B"], c["starts"] = 4, [-5, 30, 20, 2000, 2100]
    # image 0: gts [0, 2); 1: non-monotone, none; 2: [1, 12) cut to Gmax; 3: non-monotone, none
    c["gt_starts"] = [-3, 2, 1, 99, 5]
    c["Nmax"], c["Gmax"] = 64, 8
    c["keys"] = np.random.default_rng(5).integers(0, 1 << 32, size=(4, 64), dtype=np.uint64).astype(np.uint32)
    return c


def _hostile_nonfinite():
    c = _random_case(32, [70], [6], RPN, num=12)
    c["boxes"][3] = [np.nan, 0, 10, 10]
    c["boxes"][4] = [0, 0, np.inf, 10]
    c["boxes"][5] = [-np.inf, -np.inf, np.inf, np.inf]
    c["boxes"][6] = [np.nan] * 4
    c["gts"][1] = [0, 0, np.inf, np.inf]
    c["gts"][2] = [np.nan, 5, 50, 50]
    return c


CASES = {
    "lattice_rpn_all": lambda: _lattice(RPN, num=8),
    "lattice_rpn_first": lambda: _lattice(RPN_FIRST, num=8),
    "lattice_rcnn": lambda: _lattice(RCNN, num=8, frac=0.25, stds=(.1, .1, .2, .2), bg_label=65),
    "lattice_band": lambda: _lattice(BAND, num=8),
    "n1_g1": lambda: _random_case(1, 1, [1], RPN, shared=True, num=4),
    "n63_g3": lambda: _random_case(2, 63, [3], RPN, shared=True, num=16),
    "n65_g65_mask": lambda: _random_case(3, 65, [65], RPN_FIRST, shared=True, mask=True, num=32),
    "n1000_g257": lambda: _random_case(4, 1000, [257], RPN, shared=True, num=256),
    "n1000_g0": lambda: _random_case(5, 1000, [0], RPN, shared=True, num=64),
    "shared_b3": lambda: _random_case(6, 1000, [65, 0, 1], RPN, shared=True, mask=True, num=256),
    "shared_b3_first": lambda: _random_case(7, 4099, [3, 65, 1], RPN_FIRST, shared=True, num=256),
    "starts_b3": lambda: _random_case(8, [4099, 1, 1000], [65, 0, 3], RCNN, num=128, frac=0.25, stds=(.1, .1, .2, .2), bg_label=65),
    "prefix_b3": lambda: _random_case(9, [1000, 63, 1], [65, 1, 0], RCNN_PREFIX, num=128, frac=0.25, stds=(.1, .1, .2, .2), bg_label=65),
    "prefix_mask_lowq": lambda: _random_case(10, [65, 63], [3, 5], dict(RPN, prefix=True), mask=True, num=32, ub=1.0),
    "band_b1": lambda: _random_case(11, 1000, [65], BAND, shared=True, num=64, means=(.1, -.1, .2, -.2), stds=(.5, .5, .25, .25)),
    "anchors64": lambda: _anchor_case(12, [1, 65, 17]),
    "hostile_tables": _hostile_tables,
    "hostile_nonfinite": _hostile_nonfinite,
}
SCALAR_CASES = ("lattice_rpn_all", "lattice_rpn_first", "lattice_rcnn", "lattice_band", "n1_g1", "n63_g3", "n65_g65_mask", "prefix_mask_lowq",
                "hostile_tables", "hostile_nonfinite")          # small enough for the Python double loop


@functools.lru_cache(maxsize=None)
def build_case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the whole pipeline of a case, computed once and shared: assignment, sampling, dense and compact targets"""
    c = build_case(name)
    gt_inds, max_ov = assign(c)
    flags, sel, counts = sample(gt_inds, c["keys"], c["starts"], len(c["boxes"]), c["gt_starts"], len(c["gts"]), c["Gmax"], c["num"],
                                c["expected_pos"], c["ub"])
    return dict(gt_inds=gt_inds, max_overlaps=max_ov, flags=flags, sel=sel, counts=counts, dense=targets(c, gt_inds, flags=flags),
                compact=targets(c, gt_inds, sel=sel))


# ---- the sampler alone: hand-made pools ------------------------------------------------------------
def _sample_case(gt_inds, keys, G, num, expected_pos, ub=-1.0):
    gt_inds = np.asarray(gt_inds, np.int32)
    B, Nmax = gt_inds.shape
    return dict(gt_inds=gt_inds, keys=np.asarray(keys, np.uint32).reshape(B, Nmax), gt_starts=np.concatenate([[0], np.cumsum(G)]).tolist(),
                Gtot=int(sum(G)), Gmax=int(max(G)), num=num, expected_pos=expected_pos, ub=ub)


def _pool(n, npos, nneg, seed, G=4):
    rng = np.random.default_rng(seed)
    gi = np.full(n, -1, np.int32)
    idx = rng.permutation(n)
    gi[idx[:npos]] = rng.integers(1, G + 1, size=npos)
    gi[idx[npos:npos + nneg]] = 0
    return gi


def _sample_cases():
    rng = np.random.default_rng(77)
    n = 3000
    rk = lambda B=1: rng.integers(0, 1 << 32, size=(B, n), dtype=np.uint64).astype(np.uint32)
    dup = (rng.integers(0, 6, size=(2, n)) * 0x30000000 % (1 << 32)).astype(np.uint32)      # six distinct keys, some with the top bit
    hostile = _pool(n, 300, 2000, 6)
    hostile[::7] = 5                                       # G + 1
    hostile[1::11] = -2
    hostile[3::17] = -(1 << 31)
    hostile[2::13] = 1 << 30
    return {
        "pool_smaller": _sample_case([_pool(n, 10, 2000, 1)], rk(), [4], 64, 32),
        "pool_equal": _sample_case([_pool(n, 32, 32, 2)], rk(), [4], 64, 32),
        "pool_larger": _sample_case([_pool(n, 500, 2400, 3), _pool(n, 33, 31, 4)], rk(2), [4, 4], 64, 32),
        "keys_equal": _sample_case([_pool(n, 500, 2400, 3)], np.full((1, n), 7, np.uint32), [4], 64, 32),
        "keys_duplicate": _sample_case([_pool(n, 500, 2400, 5), _pool(n, 1500, 1500, 6)], dup, [4, 4], 256, 128),
        "keys_top_bit": _sample_case([_pool(n, 500, 2400, 7)], rk() | np.uint32(0x80000000) * (rng.random((1, n)) < 0.5), [4], 64, 32),
        "neg_short": _sample_case([_pool(n, 500, 5, 8)], rk(), [4], 64, 16),
        "neg_pos_ub": _sample_case([_pool(n, 7, 2000, 9), _pool(n, 0, 2000, 10)], rk(2), [4, 4], 64, 32, ub=1.0),
        "hostile_gt_inds": _sample_case([hostile], rk(), [4], 512, 128),
        "num_max": _sample_case([_pool(n, 2900, 100, 11)], rk(), [4], 4096, 2048),
        "single_row": _sample_case([[1]], [[5]], [1], 4, 2),
    }


@functools.lru_cache(maxsize=None)
def sample_cases():
    return _sample_cases()


def same_float_bits(a, b):
    """bit-equal, or NaN on both sides (a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))
