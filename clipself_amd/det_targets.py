"""Detector training targets: anchors, IoU assignment, random sampling and box-delta targets, usable without mmcv / mmdet.

What every F-ViT config runs twice per step through mmdet 2.x: `train_cfg.rpn` (MaxIoUAssigner over all anchors, RandomSampler(256, 0.5),
DeltaXYWHBBoxCoder.encode with stds 1) and `train_cfg.rcnn` (MaxIoUAssigner over the proposals, RandomSampler(512, 0.25,
add_gt_as_proposals=True), stds (.1, .1, .2, .2)).  The contract -- IoU arithmetic, thresholds, the order of the low-quality matches, the
selection rule of the sampler, the target layouts -- is stated once, in include/clipself_assign.h.  mmcv / mmdet are not available to this
project: names, keywords and semantics follow the published mmdet 2.x sources as read (parity-unpinned, like det_post and roi_extractor).

Two routes.  KERNEL (CUDA tensors on a backend with ASSIGN, HipOps): csa_assign / csa_sample / csa_targets, everything on the stream,
fixed shapes; `rpn_targets` / `rcnn_targets` read nothing back, the per-image `assign` / `sample` of the mmdet-named classes read `counts`
once because mmdet's results are variable length.  TORCH (CPU tensors or a backend without ASSIGN): `assign_torch` / `sample_torch` /
`targets_torch`, the same contract in plain fp32 torch, per image, with the Python loop over ground truths -- the SLOW route: it exists so
that the module works everywhere and as the other implementation the kernels are compared with (tools/det_targets_bench.py times the
kernels next to mmdet's own route, torch on the device).  The two
routes return equal integers and bit-equal floats, except the dw, dh targets: the device's logf is not the host's (the torch route takes
libm's double log and rounds it once to fp32).

The sampler's randomness is a tensor of 32-bit keys (from a torch.Generator, or passed as keys=): the rows with the smallest (key, row)
pairs are taken.  With independent uniform keys that is a uniform random subset, which is all mmdet's `random_choice` promises; it is not
the sequence `torch.randperm` would draw.
"""
from __future__ import annotations

import math

import torch

from .det_backend import as_i32, kernel_ops
from .det_post import delta2bbox  # noqa: F401  (the inverse of bbox2delta; re-exported, not copied)
from .hip import ASSIGN_MAX_GT as KERNEL_MAX_GT, ASSIGN_MAX_NUM as KERNEL_MAX_NUM, ASSIGN_MAX_ROWS as KERNEL_MAX_ROWS  # include/clipself_assign.h: Gmax, num, Nmax


def _kernel_ops(t, ops=None):
    return kernel_ops(t, "ASSIGN", ops)


# ================================================================================================ anchors
def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class AnchorGenerator:
    """mmdet 2.x `AnchorGenerator` (the 2-D anchor-based one): same keywords, same base anchors, same order of `grid_priors` --
    location-major with the base anchors innermost, matching rpn_cls_score.permute(0, 2, 3, 1).  Plain torch, computed once per
    (sizes, dtype, device) and cached: not a hot path."""

    def __init__(self, strides, ratios, scales=None, base_sizes=None, scale_major=True, octave_base_scale=None, scales_per_octave=None,
                 centers=None, center_offset=0.):
        if center_offset != 0 and centers is not None:
            raise ValueError(f"center cannot be set when center_offset != 0, {centers} is given")
        if not 0 <= center_offset <= 1:
            raise ValueError(f"center_offset should be in range [0, 1], {center_offset} is given")
        if centers is not None and len(centers) != len(strides):
            raise ValueError(f"The number of strides should be the same as centers, got {strides} and {centers}")
        self.strides = [_pair(s) for s in strides]
        self.base_sizes = [min(s) for s in self.strides] if base_sizes is None else list(base_sizes)
        if len(self.base_sizes) != len(self.strides):
            raise ValueError(f"The number of strides should be the same as base sizes, got {self.strides} and {self.base_sizes}")
        if (octave_base_scale is not None and scales_per_octave is not None) == (scales is not None):
            raise ValueError("scales and octave_base_scale with scales_per_octave cannot be set at the same time")
        if scales is not None:
            self.scales = torch.tensor([float(s) for s in scales])
        else:
            self.scales = torch.tensor([2.0 ** (i / scales_per_octave) for i in range(scales_per_octave)]) * octave_base_scale
        self.octave_base_scale, self.scales_per_octave = octave_base_scale, scales_per_octave
        self.ratios = torch.tensor([float(r) for r in ratios])
        self.scale_major, self.centers, self.center_offset = scale_major, centers, center_offset
        self.base_anchors = self.gen_base_anchors()
        self._cache = {}

    @property
    def num_base_priors(self):
        return [b.shape[0] for b in self.base_anchors]

    num_base_anchors = num_base_priors

    @property
    def num_levels(self):
        return len(self.strides)

    def gen_base_anchors(self):
        return [self.gen_single_level_base_anchors(bs, self.scales, self.ratios, None if self.centers is None else self.centers[i])
                for i, bs in enumerate(self.base_sizes)]

    def gen_single_level_base_anchors(self, base_size, scales, ratios, center=None):
        w = h = base_size
        x_center, y_center = (self.center_offset * w, self.center_offset * h) if center is None else center
        h_ratios = torch.sqrt(ratios)
        w_ratios = 1 / h_ratios
        if self.scale_major:
            ws = (w * w_ratios[:, None] * scales[None, :]).view(-1)
            hs = (h * h_ratios[:, None] * scales[None, :]).view(-1)
        else:
            ws = (w * scales[:, None] * w_ratios[None, :]).view(-1)
            hs = (h * scales[:, None] * h_ratios[None, :]).view(-1)
        return torch.stack([x_center - 0.5 * ws, y_center - 0.5 * hs, x_center + 0.5 * ws, y_center + 0.5 * hs], dim=-1)

    def single_level_grid_priors(self, featmap_size, level_idx, dtype=torch.float32, device="cpu"):
        base = self.base_anchors[level_idx].to(device=device, dtype=dtype)
        feat_h, feat_w = featmap_size
        stride_w, stride_h = self.strides[level_idx]
        shift_x = torch.arange(0, feat_w, device=device).to(dtype) * stride_w
        shift_y = torch.arange(0, feat_h, device=device).to(dtype) * stride_h
        xx, yy = shift_x.repeat(feat_h), shift_y.view(-1, 1).repeat(1, feat_w).view(-1)
        shifts = torch.stack([xx, yy, xx, yy], dim=-1)
        return (base[None, :, :] + shifts[:, None, :]).view(-1, 4)

    def grid_priors(self, featmap_sizes, dtype=torch.float32, device="cpu"):
        """-> one [h * w * num_base, 4] tensor per level."""
        if len(featmap_sizes) != self.num_levels:
            raise ValueError(f"{len(featmap_sizes)} feature maps for {self.num_levels} levels")
        key = (tuple(tuple(int(v) for v in s) for s in featmap_sizes), dtype, str(device))
        if key not in self._cache:
            self._cache[key] = [self.single_level_grid_priors(s, i, dtype, device) for i, s in enumerate(key[0])]
        return self._cache[key]

    grid_anchors = grid_priors

    def valid_flags(self, featmap_sizes, pad_shape, device="cpu"):
        """-> one bool [h * w * num_base] per level: the anchors whose location lies inside the padded image."""
        if len(featmap_sizes) != self.num_levels:
            raise ValueError(f"{len(featmap_sizes)} feature maps for {self.num_levels} levels")
        out = []
        for i, (feat_h, feat_w) in enumerate(featmap_sizes):
            stride_w, stride_h = self.strides[i]
            h, w = pad_shape[:2]
            valid_h, valid_w = min(int(math.ceil(h / stride_h)), feat_h), min(int(math.ceil(w / stride_w)), feat_w)
            vx = torch.zeros(feat_w, dtype=torch.bool, device=device)
            vy = torch.zeros(feat_h, dtype=torch.bool, device=device)
            vx[:valid_w], vy[:valid_h] = True, True
            valid = vx.repeat(feat_h) & vy.view(-1, 1).repeat(1, feat_w).view(-1)
            nb = self.num_base_priors[i]
            out.append(valid[:, None].expand(valid.size(0), nb).contiguous().view(-1))
        return out


# ================================================================================================ the torch route
def _range(tab, b, total, cap):
    """Rows (s, n) of image b: the header's clamping of starts / gt_starts; tab None = the shared form."""
    if tab is None:
        return 0, min(total, cap)
    s, e = min(max(int(tab[b]), 0), total), min(max(int(tab[b + 1]), 0), total)
    return s, (min(e - s, cap) if e > s else 0)


def _tab(t):
    return None if t is None else [int(v) for v in (t.tolist() if isinstance(t, torch.Tensor) else t)]


def bbox_overlaps(bboxes1, bboxes2, mode="iou", is_aligned=False, eps=1e-6):
    """mmdet 2.x `bbox_overlaps`, mode 'iou': [M, 4] x [N, 4] -> [M, N] (aligned: [M, 4] x [M, 4] -> [M]), in the header's fp32 arithmetic:
    every product and sum is a torch op of its own.  Unlike mmdet a NaN IoU counts as 0."""
    if mode != "iou":
        raise ValueError(f"mode {mode!r}: only 'iou' is implemented")
    a, b = bboxes1.detach().float(), bboxes2.detach().float()
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    if is_aligned:
        if a.shape[0] != b.shape[0]:
            raise ValueError("aligned boxes need equal counts")
        lt, rb = torch.maximum(a[:, :2], b[:, :2]), torch.minimum(a[:, 2:4], b[:, 2:4])
        both = area1 + area2
    else:
        lt, rb = torch.maximum(a[:, None, :2], b[None, :, :2]), torch.minimum(a[:, None, 2:4], b[None, :, 2:4])
        both = area1[:, None] + area2[None, :]
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.maximum(both - overlap, torch.tensor(eps, dtype=torch.float32, device=a.device))
    ious = overlap / union
    return torch.where(torch.isnan(ious), torch.zeros_like(ious), ious)


def _log_f32(t):
    """The host routes' log: libm's double log of each fp32 value, rounded once to fp32 (0 -> -inf, negative or NaN -> NaN)."""
    vals = []
    for v in t.reshape(-1).tolist():
        vals.append(float("nan") if (v != v or v < 0) else float("-inf") if v == 0 else float("inf") if v == float("inf") else math.log(v))
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32).reshape(t.shape).to(t.device)


def bbox2delta(proposals, gt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """mmdet 2.x `bbox2delta` in fp32, op by op: proposals [n, 4], gt [n, 4] -> deltas [n, 4].  CPU tensors: the header's arithmetic with
    the host log; CUDA tensors: torch's own log (a convenience -- the training targets come from `rpn_targets` / `rcnn_targets`)."""
    p, g = proposals.detach().float(), gt.detach().float()
    pxy, pwh = (p[:, :2] + p[:, 2:4]) * 0.5, p[:, 2:4] - p[:, :2]
    gxy, gwh = (g[:, :2] + g[:, 2:4]) * 0.5, g[:, 2:4] - g[:, :2]
    ratio = gwh / pwh
    d = torch.cat([(gxy - pxy) / pwh, ratio.log() if ratio.is_cuda else _log_f32(ratio)], dim=1)
    f = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float32, device=p.device)
    return (d - f(means)) / f(stds)


def assign_torch(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True,
                 gt_max_assign_all=True, gt_prefix=False, valid=None):
    """csa_assign in plain torch (module docstring: the slow route) -> gt_inds [B, Nmax] int32, max_overlaps [B, Nmax] fp32."""
    dev = boxes.device
    boxes, gt_boxes = boxes.detach().float().cpu(), gt_boxes.detach().float().cpu()
    valid = None if valid is None else valid.detach().cpu() != 0
    starts, gt_starts = _tab(starts), _tab(gt_starts)
    K, Gtot = boxes.shape[0], gt_boxes.shape[0]
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    lo, hi = (neg_iou_thr if isinstance(neg_iou_thr, (tuple, list)) else (0.0, neg_iou_thr))
    lo, hi, pos_thr, min_pos = f32(lo), f32(hi), f32(pos_iou_thr), f32(min_pos_iou)
    gt_inds = torch.full((B, Nmax), -1, dtype=torch.int32)
    max_ov = torch.zeros(B, Nmax, dtype=torch.float32)
    for b in range(B):
        s, n = _range(starts, b, K, Nmax)
        gs, g = _range(gt_starts, b, Gtot, Gmax)
        if n == 0:
            continue
        rows = torch.arange(n)
        ok = torch.ones(n, dtype=torch.bool) if valid is None else valid[s:s + n]
        pref = (rows < g) if gt_prefix else torch.zeros(n, dtype=torch.bool)
        act = ok & ~pref
        gi, mo = torch.full((n,), -1, dtype=torch.int64), torch.zeros(n)
        if g == 0:
            gi[ok] = 0
        else:
            m = int(act.sum())
            if m > 0:
                ov = bbox_overlaps(gt_boxes[gs:gs + g], boxes[s:s + n][act])                 # [g, m]
                mx = ov.max(dim=0).values
                arg = torch.where(ov == mx[None, :], torch.arange(g)[:, None], g).min(dim=0).values       # ties: the lowest ground truth
                a = torch.full((m,), -1, dtype=torch.int64)
                a[(mx >= lo) & (mx < hi)] = 0
                p = mx >= pos_thr
                a[p] = arg[p] + 1
                if match_low_quality:
                    gt_mx = ov.max(dim=1).values
                    for i in range(g):                                                         # in this order: later ones overwrite
                        if gt_mx[i] >= min_pos:
                            hit = ov[i] == gt_mx[i]
                            if gt_max_assign_all:
                                a[hit] = i + 1
                            else:
                                a[int(torch.nonzero(hit)[0, 0])] = i + 1
                gi[act], mo[act] = a, mx
            gi[pref & ok], mo[pref & ok] = rows[pref & ok] + 1, 1.0
        gt_inds[b, :n], max_ov[b, :n] = gi.to(torch.int32), mo
    return gt_inds.to(dev), max_ov.to(dev)


def _ukeys(keys):
    """32-bit keys (an int32 or uint32 tensor) -> int64 in [0, 2^32): the unsigned order."""
    return keys.detach().cpu().view(torch.int32).to(torch.int64) & 0xFFFFFFFF if keys.dtype != torch.int64 else keys.detach().cpu() & 0xFFFFFFFF


def sample_torch(gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, neg_pos_ub=-1.0):
    """csa_sample in plain torch -> flags [B, Nmax] uint8, sel [B, num] int32, counts [B, 2] int32."""
    dev = gt_inds.device
    gt_inds, keys = gt_inds.detach().cpu().to(torch.int64), _ukeys(keys)
    B, Nmax = gt_inds.shape
    starts, gt_starts = _tab(starts), _tab(gt_starts)
    flags = torch.zeros(B, Nmax, dtype=torch.uint8)
    sel = torch.full((B, num), -1, dtype=torch.int32)
    counts = torch.zeros(B, 2, dtype=torch.int32)

    def choose(pool, key, want):
        if want <= 0:
            return pool[:0]
        if pool.numel() <= want:
            return pool
        order = torch.argsort(key[pool], stable=True)[:want]                # pool is in ascending row: a stable sort orders by (key, row)
        return pool[order].sort().values

    for b in range(B):
        _, n = _range(starts, b, K, Nmax)
        _, g = _range(gt_starts, b, Gtot, Gmax)
        gi, key = gt_inds[b, :n], keys[b, :n]
        pos = choose(torch.nonzero((gi > 0) & (gi <= g))[:, 0], key, min(max(int(expected_pos), 0), num))
        want_neg = num - pos.numel()
        if neg_pos_ub >= 0:
            ub = float(torch.tensor(float(neg_pos_ub), dtype=torch.float32) * torch.tensor(float(max(1, pos.numel())), dtype=torch.float32))
            if ub < want_neg:
                want_neg = int(ub)
        neg = choose(torch.nonzero(gi == 0)[:, 0], key, want_neg)
        flags[b, pos], flags[b, neg] = 1, 2
        sel[b, :pos.numel()] = pos.to(torch.int32)
        sel[b, pos.numel():pos.numel() + neg.numel()] = neg.to(torch.int32)
        counts[b, 0], counts[b, 1] = pos.numel(), neg.numel()
    return flags.to(dev), sel.to(dev), counts.to(dev)


def targets_torch(boxes, starts, gt_boxes, gt_labels, gt_starts, Gmax, gt_inds, flags=None, sel=None, means=(0., 0., 0., 0.),
                  stds=(1., 1., 1., 1.), bg_label=1, pos_weight=-1.0):
    """csa_targets in plain torch: the dense form (sel None, from flags) or the compact form (sel [B, num])."""
    if pos_weight > 0:
        raise ValueError(f"pos_weight = {pos_weight} is not supported (only pos_weight <= 0)")
    dev = boxes.device
    boxes, gt_boxes = boxes.detach().float().cpu(), gt_boxes.detach().float().cpu()
    gt_inds = gt_inds.detach().cpu().to(torch.int64)
    gt_labels = None if gt_labels is None else gt_labels.detach().cpu().to(torch.int32)
    B, Nmax = gt_inds.shape
    starts, gt_starts = _tab(starts), _tab(gt_starts)
    K, Gtot = boxes.shape[0], gt_boxes.shape[0]
    S = Nmax if sel is None else sel.shape[1]
    labels = torch.full((B, S), int(bg_label), dtype=torch.int32)
    lw, bt, bw = torch.zeros(B, S), torch.zeros(B, S, 4), torch.zeros(B, S, 4)
    rois = None
    if sel is not None:
        sel = sel.detach().cpu().to(torch.int64)
        rois = torch.zeros(B, S, 5)
        rois[:, :, 0] = -1.0
    else:
        flags = flags.detach().cpu()
    for b in range(B):
        s, n = _range(starts, b, K, Nmax)
        gs, g = _range(gt_starts, b, Gtot, Gmax)
        if sel is None:
            slots = torch.nonzero(flags[b, :n] != 0)[:, 0]
            rows = slots
        else:
            ok = (sel[b] >= 0) & (sel[b] < n)
            slots = torch.nonzero(ok)[:, 0]
            rows = sel[b][slots]
        if slots.numel() == 0:
            continue
        gi = gt_inds[b][rows]
        gi = torch.where((gi < -1) | (gi > g), torch.full_like(gi, -1), gi)
        pos = gi > 0
        if sel is None:
            pos &= flags[b][rows] == 1
        lw[b, slots] = 1.0
        if sel is not None:
            rois[b, slots, 0] = float(b)
            rois[b, slots, 1:] = boxes[s + rows]
        ps, pr, pg = slots[pos], rows[pos], gi[pos] - 1
        if ps.numel():
            labels[b, ps] = gt_labels[gs + pg] if gt_labels is not None else 0
            bt[b, ps] = bbox2delta(boxes[s + pr], gt_boxes[gs + pg], means, stds)
            bw[b, ps] = 1.0
    out = (labels.to(dev), lw.to(dev), bt.to(dev), bw.to(dev))
    return out if sel is None else (rois.to(dev),) + out


# ================================================================================================ tensor-level entry points
def _f32_rows(t):
    t = t.detach()
    if t.dtype != torch.float32 or (t.shape[0] and t.stride(1) != 1):
        t = t.float().contiguous()
    return t


def _check_limits(Nmax, Gmax, num=1):
    if not (0 <= Nmax <= KERNEL_MAX_ROWS and 0 <= Gmax <= KERNEL_MAX_GT and 1 <= num <= KERNEL_MAX_NUM):
        raise ValueError(f"the kernel route takes at most {KERNEL_MAX_ROWS} boxes and {KERNEL_MAX_GT} ground truths per image and "
                         f"num <= {KERNEL_MAX_NUM} (Nmax = {Nmax}, Gmax = {Gmax}, num = {num})")


def assign(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True,
           gt_max_assign_all=True, gt_prefix=False, valid=None, ops=None):
    """Route by tensor: csa_assign on a kernel backend, assign_torch otherwise."""
    k_ops = _kernel_ops(boxes, ops)
    if k_ops is None:
        return assign_torch(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, pos_iou_thr, neg_iou_thr, min_pos_iou, match_low_quality,
                            gt_max_assign_all, gt_prefix, valid)
    _check_limits(Nmax, Gmax)
    dev = boxes.device
    valid = None if valid is None else valid.detach().to(device=dev, dtype=torch.uint8).contiguous()
    return k_ops.assign(_f32_rows(boxes), as_i32(starts, dev), _f32_rows(gt_boxes.to(dev)), as_i32(gt_starts, dev), B, Nmax, Gmax, pos_iou_thr,
                        neg_iou_thr, min_pos_iou, match_low_quality, gt_max_assign_all, gt_prefix, valid)


def sample(gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, neg_pos_ub=-1.0, ops=None):
    """Route by tensor: csa_sample on a kernel backend, sample_torch otherwise."""
    k_ops = _kernel_ops(gt_inds, ops)
    if k_ops is None:
        return sample_torch(gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, neg_pos_ub)
    _check_limits(gt_inds.shape[1], Gmax, num)
    dev = gt_inds.device
    if keys.dtype == torch.int64:
        keys = keys.to(torch.int32)                                         # wraps: the low 32 bits
    return k_ops.sample(gt_inds.contiguous(), keys.to(dev).contiguous(), as_i32(starts, dev), K, as_i32(gt_starts, dev), Gtot, Gmax, num,
                        expected_pos, neg_pos_ub)


def bbox_targets(boxes, starts, gt_boxes, gt_labels, gt_starts, Gmax, gt_inds, flags=None, sel=None, means=(0., 0., 0., 0.),
                 stds=(1., 1., 1., 1.), bg_label=1, pos_weight=-1.0, ops=None):
    """Route by tensor: csa_targets on a kernel backend, targets_torch otherwise."""
    k_ops = _kernel_ops(boxes, ops)
    if k_ops is None:
        return targets_torch(boxes, starts, gt_boxes, gt_labels, gt_starts, Gmax, gt_inds, flags, sel, means, stds, bg_label, pos_weight)
    _check_limits(gt_inds.shape[1], Gmax, 1 if sel is None else sel.shape[1])
    dev = boxes.device
    return k_ops.bbox_targets(_f32_rows(boxes), as_i32(starts, dev), _f32_rows(gt_boxes.to(dev)), as_i32(gt_labels, dev), as_i32(gt_starts, dev), Gmax,
                              gt_inds.contiguous(), None if flags is None else flags.contiguous(), None if sel is None else sel.contiguous(),
                              means, stds, bg_label, pos_weight)


def random_keys(shape, device, generator=None):
    """Independent uniform 32-bit keys as an int32 tensor (its bits are the keys), drawn on `device` from `generator`."""
    return torch.randint(-(1 << 31), 1 << 31, tuple(shape), dtype=torch.int64, device=device, generator=generator).to(torch.int32)


# ================================================================================================ mmdet's classes
class AssignResult:
    """mmdet's `AssignResult`: num_gts, gt_inds [n] int64 (-1 ignore, 0 negative, i + 1 ground truth i), max_overlaps [n], labels or None."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels

    @property
    def num_preds(self):
        return len(self.gt_inds)

    def add_gt_(self, gt_labels):
        dev = self.gt_inds.device
        self.gt_inds = torch.cat([torch.arange(1, len(gt_labels) + 1, dtype=torch.long, device=dev), self.gt_inds])
        self.max_overlaps = torch.cat([self.max_overlaps.new_ones(len(gt_labels)), self.max_overlaps])
        if self.labels is not None:
            self.labels = torch.cat([gt_labels.to(self.labels.dtype), self.labels])


class SamplingResult:
    """mmdet's `SamplingResult`: pos_inds, neg_inds, pos_bboxes, neg_bboxes, pos_is_gt, num_gts, pos_assigned_gt_inds, pos_gt_bboxes,
    pos_gt_labels."""

    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)
        else:
            self.pos_gt_bboxes = gt_bboxes.view(-1, 4)[self.pos_assigned_gt_inds.long(), :]
        self.pos_gt_labels = assign_result.labels[pos_inds] if assign_result.labels is not None else None

    @property
    def bboxes(self):
        return torch.cat([self.pos_bboxes, self.neg_bboxes])


class MaxIoUAssigner:
    """mmdet 2.x `MaxIoUAssigner` with its constructor keywords (`type` is accepted so that a config dict builds it unchanged).  What the
    contract leaves out raises ValueError here: ignore_iof_thr > 0, gpu_assign_thr > 0, an iou_calculator other than BboxOverlaps2D."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1, ignore_wrt_candidates=True,
                 match_low_quality=True, gpu_assign_thr=-1, iou_calculator=None, type=None):
        if type not in (None, "MaxIoUAssigner"):
            raise ValueError(f"type {type!r} is not MaxIoUAssigner")
        if ignore_iof_thr > 0:
            raise ValueError("ignore_iof_thr > 0 (gt_bboxes_ignore) is not implemented: no F-ViT config uses it")
        if gpu_assign_thr > 0:
            raise ValueError("gpu_assign_thr is not implemented: the assignment never leaves the device")
        calc = iou_calculator or dict(type="BboxOverlaps2D")
        if dict(calc) != dict(type="BboxOverlaps2D"):
            raise ValueError(f"iou_calculator {calc!r}: only dict(type='BboxOverlaps2D') is implemented")
        if isinstance(neg_iou_thr, (tuple, list)) and len(neg_iou_thr) != 2:
            raise ValueError("neg_iou_thr is a float or a (lo, hi) pair")
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.match_low_quality = bool(gt_max_assign_all), bool(match_low_quality)
        self.ignore_iof_thr, self.ignore_wrt_candidates, self.gpu_assign_thr = ignore_iof_thr, ignore_wrt_candidates, gpu_assign_thr

    def assign_batched(self, boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, gt_prefix=False, valid=None, ops=None):
        return assign(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou,
                      self.match_low_quality, self.gt_max_assign_all, gt_prefix, valid, ops)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """One image: bboxes [n, 4], gt_bboxes [k, 4] -> AssignResult."""
        if gt_bboxes_ignore is not None and len(gt_bboxes_ignore) > 0:
            raise ValueError("gt_bboxes_ignore is not implemented")
        n, g = bboxes.shape[0], gt_bboxes.shape[0]
        gt_inds, max_ov = self.assign_batched(bboxes[:, :4], None, gt_bboxes.reshape(-1, 4), [0, g], 1, n, g)
        gt_inds = gt_inds[0].to(torch.int64)
        labels = None
        if gt_labels is not None:
            labels = gt_inds.new_full((n,), -1)
            pos = gt_inds > 0
            labels[pos] = gt_labels.to(torch.int64)[gt_inds[pos] - 1]
        return AssignResult(g, gt_inds, max_ov[0], labels)


class RandomSampler:
    """mmdet 2.x `RandomSampler` with its constructor keywords; the randomness comes as keys (module docstring)."""

    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, type=None, pos_weight=-1, **kwargs):
        if type not in (None, "RandomSampler"):
            raise ValueError(f"type {type!r} is not RandomSampler")
        if kwargs:
            raise ValueError(f"unsupported keywords {sorted(kwargs)}")
        if pos_weight > 0:
            raise ValueError("pos_weight > 0 is not implemented: every F-ViT config passes -1")
        if not (1 <= int(num) and 0 <= pos_fraction <= 1):
            raise ValueError(f"num = {num} must be >= 1 and pos_fraction = {pos_fraction} in [0, 1]")
        self.num, self.pos_fraction, self.neg_pos_ub, self.add_gt_as_proposals = int(num), pos_fraction, neg_pos_ub, bool(add_gt_as_proposals)

    @property
    def expected_pos(self):
        return int(self.num * self.pos_fraction)

    def sample_batched(self, gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, ops=None):
        return sample(gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, self.num, self.expected_pos, float(self.neg_pos_ub), ops)

    def sample(self, assign_result, bboxes, gt_bboxes, gt_labels=None, generator=None, keys=None):
        """One image -> SamplingResult.  With add_gt_as_proposals the ground truths are put in front of bboxes (AssignResult.add_gt_), which
        needs gt_labels, as in mmdet.  `counts` is read once."""
        bboxes = bboxes[:, :4]
        gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.uint8)
        if self.add_gt_as_proposals and len(gt_bboxes) > 0:
            if gt_labels is None:
                raise ValueError("gt_labels must be given when add_gt_as_proposals is True")
            bboxes = torch.cat([gt_bboxes.reshape(-1, 4).to(bboxes.dtype), bboxes], dim=0)
            assign_result.add_gt_(gt_labels)
            gt_flags = torch.cat([bboxes.new_ones(gt_bboxes.shape[0], dtype=torch.uint8), gt_flags])
        n, g = bboxes.shape[0], gt_bboxes.shape[0]
        gi = assign_result.gt_inds.to(torch.int32).reshape(1, n).contiguous()
        if keys is None:
            keys = random_keys((1, n), bboxes.device, generator)
        _, sel, counts = self.sample_batched(gi, keys.reshape(1, n), None, n, [0, g], g, g)
        npos, nneg = (int(v) for v in counts[0].tolist())
        pos_inds, neg_inds = sel[0, :npos].to(torch.int64), sel[0, npos:npos + nneg].to(torch.int64)
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes.reshape(-1, 4), assign_result, gt_flags)


# ================================================================================================ the batched forms a training loop calls
def _cat_gts(gt_bboxes_list, gt_labels_list, device):
    lens = [int(g.shape[0]) for g in gt_bboxes_list]                        # host values: the loader made these lists
    gt_starts = [0]
    for n in lens:
        gt_starts.append(gt_starts[-1] + n)
    if sum(lens):
        gts = torch.cat([g.reshape(-1, 4).to(device=device, dtype=torch.float32) for g in gt_bboxes_list], dim=0)
    else:
        gts = torch.zeros(0, 4, dtype=torch.float32, device=device)
    labels = None
    if gt_labels_list is not None:
        labels = (torch.cat([l.reshape(-1).to(device=device, dtype=torch.int32) for l in gt_labels_list]) if sum(lens)
                  else torch.zeros(0, dtype=torch.int32, device=device))
    return gts, labels, gt_starts, max(lens) if lens else 0


def rpn_targets(anchors, valid, gt_bboxes_list, assigner, sampler, coder_means=(0., 0., 0., 0.), coder_stds=(1., 1., 1., 1.), generator=None,
                keys=None, ops=None):
    """AnchorHead.get_targets for the RPN, all images in three launches' worth of calls, fixed shapes, no read-back on the kernel route.
    anchors [N, 4] (all levels concatenated, shared by the images), valid [N] bool / uint8 or None, gt_bboxes_list: B tensors [G_b, 4].
    -> labels [B, N] int32 (0 foreground, 1 background), label_weights [B, N], bbox_targets [B, N, 4], bbox_weights [B, N, 4] and
    num_total_samples (a device scalar, at least 1)."""
    if sampler.add_gt_as_proposals:
        raise ValueError("rpn_targets: the anchors are shared by the images, so the sampler must have add_gt_as_proposals=False")
    dev, B, N = anchors.device, len(gt_bboxes_list), anchors.shape[0]
    gts, _, gt_starts, Gmax = _cat_gts(gt_bboxes_list, None, dev)
    Gtot = gts.shape[0]
    anchors = _f32_rows(anchors)
    valid = None if valid is None else valid.to(torch.uint8)
    gt_starts_t = as_i32(gt_starts, dev) if anchors.is_cuda else gt_starts
    gt_inds, _ = assigner.assign_batched(anchors, None, gts, gt_starts_t, B, N, Gmax, False, valid, ops)
    if keys is None:
        keys = random_keys((B, N), dev, generator)
    flags, _, counts = sampler.sample_batched(gt_inds, keys, None, N, gt_starts_t, Gtot, Gmax, ops)
    labels, lw, bt, bw = bbox_targets(anchors, None, gts, None, gt_starts_t, Gmax, gt_inds, flags, None, coder_means, coder_stds, 1, -1.0, ops)
    return labels, lw, bt, bw, counts.sum().clamp(min=1)


def _pos_gt_inds(gt_inds, sel, starts, gt_starts, K, Gtot, Gmax):
    """[B * num] int32: the row of each slot's assigned ground truth in the concatenated ground-truth list, -1 for negatives and padding
    slots.  One gather on the tensors' device, with the clamping of the header's starts / gt_starts; nothing is read back."""
    dev, i64 = gt_inds.device, torch.int64
    B, Nmax = gt_inds.shape
    if Nmax == 0:
        return torch.full((sel.numel(),), -1, dtype=torch.int32, device=dev)
    st = torch.as_tensor(starts, device=dev).to(i64).clamp(0, K)
    gst = torch.as_tensor(gt_starts, device=dev).to(i64).clamp(0, Gtot)
    n = (st[1:] - st[:-1]).clamp(0, Nmax)
    g = (gst[1:] - gst[:-1]).clamp(0, Gmax)
    rows = sel.to(i64)
    ok = (rows >= 0) & (rows < n[:, None])
    gi = gt_inds.to(i64).gather(1, rows.clamp(0, Nmax - 1))
    pos = ok & (gi > 0) & (gi <= g[:, None])
    return torch.where(pos, gst[:-1, None] + gi - 1, torch.full_like(gi, -1)).to(torch.int32).reshape(-1)


def rcnn_targets(proposals, gt_bboxes_list, gt_labels_list, assigner, sampler, coder_means=(0., 0., 0., 0.), coder_stds=(.1, .1, .2, .2),
                 num_classes=65, generator=None, keys=None, ops=None, return_gt_inds=False, proposal_counts=None):
    """StandardRoIHead's assign + sample and BBoxHead.get_targets (reg_class_agnostic=True) for all images, fixed shapes, no read-back on
    the kernel route.  proposals [B, P, 4] or a list of [P_b, 4(+)] tensors.
    -> rois [B * num, 5], labels [B * num] int32, label_weights [B * num], bbox_targets [B * num, 4], bbox_weights [B * num, 4]; slots a
    sampler could not fill are rows with image -1 and zero weights, which SingleRoIExtractor pools to zeros.
    return_gt_inds=True adds a sixth tensor, pos_gt_inds [B * num] int32: the row of the slot's assigned ground truth in the concatenated
    ground-truth list (what `det_masks.mask_target` indexes the masks with), -1 for negatives and padding slots.
    proposal_counts [B] (a device tensor, as `det_proposals.rpn_proposals` returns it with its fixed-shape proposals): the rows of image b
    past its count are marked valid = 0 for the assigner -- never matched, never sampled, weights 0 -- so the result equals the list form
    on the trimmed proposals with the same keys, and nothing is read back."""
    props = [p[:, :4] for p in (proposals if isinstance(proposals, (list, tuple)) else proposals.unbind(0))]
    B, dev = len(props), props[0].device
    if len(gt_bboxes_list) != B or len(gt_labels_list) != B:
        raise ValueError(f"{B} images of proposals, {len(gt_bboxes_list)} of gt_bboxes, {len(gt_labels_list)} of gt_labels")
    gts, labels, gt_starts, Gmax = _cat_gts(gt_bboxes_list, gt_labels_list, dev)
    Gtot = gts.shape[0]
    prefix = sampler.add_gt_as_proposals
    if proposal_counts is not None and proposal_counts.numel() != B:
        raise ValueError(f"proposal_counts holds {proposal_counts.numel()} counts for {B} images")
    parts, starts, live = [], [0], []
    for b in range(B):
        if prefix:
            parts.append(gts[gt_starts[b]:gt_starts[b + 1]])
        parts.append(props[b].to(torch.float32))
        starts.append(starts[-1] + props[b].shape[0] + (gt_starts[b + 1] - gt_starts[b] if prefix else 0))
        if proposal_counts is not None:                                     # built on the device: the ground-truth prefix rows are valid
            if prefix:
                live.append(torch.ones(gt_starts[b + 1] - gt_starts[b], dtype=torch.bool, device=dev))
            live.append(torch.arange(props[b].shape[0], device=dev) < proposal_counts.reshape(-1)[b].to(dev))
    boxes = torch.cat(parts, dim=0).contiguous()
    valid = torch.cat(live).to(torch.uint8) if proposal_counts is not None else None
    K, Nmax = boxes.shape[0], max(starts[b + 1] - starts[b] for b in range(B))
    starts_t, gt_starts_t = (as_i32(starts, dev), as_i32(gt_starts, dev)) if boxes.is_cuda else (starts, gt_starts)
    gt_inds, _ = assigner.assign_batched(boxes, starts_t, gts, gt_starts_t, B, Nmax, Gmax, prefix, valid, ops)
    if keys is None:
        keys = random_keys((B, Nmax), dev, generator)
    _, sel, _ = sampler.sample_batched(gt_inds, keys, starts_t, K, gt_starts_t, Gtot, Gmax, ops)
    rois, lab, lw, bt, bw = bbox_targets(boxes, starts_t, gts, labels, gt_starts_t, Gmax, gt_inds, None, sel, coder_means, coder_stds,
                                         int(num_classes), -1.0, ops)
    n = B * sampler.num
    out = (rois.reshape(n, 5), lab.reshape(n), lw.reshape(n), bt.reshape(n, 4), bw.reshape(n, 4))
    if return_gt_inds:
        out += (_pos_gt_inds(gt_inds, sel, starts_t, gt_starts_t, K, Gtot, Gmax),)
    return out
