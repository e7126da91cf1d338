"""Detector post-processing: box decoding, score threshold, class-aware NMS and the per-image cut, usable without mmcv / mmdet.

The tail of the reference's F-ViT heads (F-ViT/models/fvit_head.py:123-164, FViTBBoxHead.get_bboxes): `bbox_coder.decode`, rescale,
`multiclass_nms(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img)`; and mmcv's `batched_nms`, which the RPN calls with the FPN level
as `idxs`.  The contract -- candidates, IoU arithmetic, order, ties, padding -- is stated once, in include/clipself_det.h.

Two routes.  KERNEL (CUDA tensors on a backend with DET_POST, HipOps): csd_nms / csd_delta2bbox, everything on the stream, fixed-shape
outputs; `detections` reads nothing back, `batched_nms` / `multiclass_nms` read `counts` once because mmcv's returns are variable length.
TORCH (CPU tensors, a backend without DET_POST, per-class boxes [n, 4 * C]): `nms_torch` / `delta2bbox_torch`, the same contract in plain
fp32 torch on the CPU -- a Python loop per list and per kept box.  It is the SLOW route: it exists so that the module works everywhere
and as the only other implementation to measure the kernels against (tools/det_post_bench.py).

Differences from mmcv / mmdet, all inside what they leave open: ties between equal scores go to the lower box row (their sort is
unstable); NMS runs per list on the un-offset boxes (equal to their offset formulation in exact arithmetic, tests/_nms_ref.py); the
kernel route needs a bound on the output: `max_num` at most 4096 and at most 16384 boxes per image.
"""
from __future__ import annotations

import math

import torch

from .det_backend import as_i32, kernel_ops
from .hip import DET_MAX_BOXES as KERNEL_MAX_BOXES, DET_MAX_NUM as KERNEL_MAX_NUM      # include/clipself_det.h: Kmax and max_num


def _kernel_ops(t, ops=None):
    return kernel_ops(t, "DET_POST", ops)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _check_nms_cfg(nms_cfg):
    if _get(nms_cfg, "type", "nms") != "nms":
        raise ValueError(f"nms_cfg type {_get(nms_cfg, 'type')!r}: only 'nms' (greedy hard NMS) is implemented")
    if _get(nms_cfg, "offset", 0) != 0:
        raise ValueError("nms_cfg offset must be 0 (mmcv's default; the +1 pixel convention is not implemented)")
    iou = _get(nms_cfg, "iou_threshold", _get(nms_cfg, "iou_thr"))
    if iou is None:
        raise ValueError("nms_cfg needs iou_threshold")
    return float(iou)                                     # split_thr is accepted and ignored: per-list NMS has no offset to split for


# ================================================================================================ the torch route
def _ord(scores):
    """fp32 scores -> int64 in [0, 2^32) with the same order (-0 below +0), the kernel's sort key."""
    bits = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)


def _suppress_row(a, rest, iou_thr):
    """iou(a, rest) > iou_thr in the header's fp32 arithmetic: every product and sum is a torch op of its own, so none is fused."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (rest[:, 2] - rest[:, 0]) * (rest[:, 3] - rest[:, 1])
    iw = (torch.minimum(a[2], rest[:, 2]) - torch.maximum(a[0], rest[:, 0])).clamp(min=0)
    ih = (torch.minimum(a[3], rest[:, 3]) - torch.maximum(a[1], rest[:, 1])).clamp(min=0)
    inter = iw * ih
    return inter / ((area_a + area_b) - inter) > iou_thr


def _greedy(boxes, iou_thr, limit):
    """boxes [m, 4] in greedy order -> positions kept (at most `limit`)."""
    m = boxes.shape[0]
    sup = torch.zeros(m, dtype=torch.bool)
    keep = []
    for i in range(m):
        if sup[i]:
            continue
        keep.append(i)
        if len(keep) >= limit:
            break
        sup |= _suppress_row(boxes[i], boxes, iou_thr)
        sup[i] = True
    return keep


def nms_torch(boxes, scores, starts, Kmax, score_thr, iou_thr, max_num, group=None, G=0):
    """csd_nms in plain torch (module docstring: the slow route).  boxes [K, 4], or [K, C, 4] for per-class boxes (list (image, c) then
    uses boxes[:, c]); scores [K, C]; starts [B + 1] (tensor or list); group [K] with G groups -> the group form (C == 1).
    -> dets [B, max_num, 5] fp32, labels, inds [B, max_num] int32, counts [B] int32 on the device of `boxes`."""
    dev = boxes.device
    boxes, scores = boxes.detach().float().cpu(), scores.detach().float().cpu()
    starts = [int(v) for v in (starts.tolist() if isinstance(starts, torch.Tensor) else starts)]
    K, C = scores.shape
    B = len(starts) - 1
    if group is not None:
        if C != 1:
            raise ValueError(f"the group form needs C == 1, got C = {C}")
        group = group.detach().cpu().to(torch.int64)
    if not (B >= 1 and max_num >= 1 and Kmax >= 0):
        raise ValueError(f"nms needs B >= 1, max_num >= 1, Kmax >= 0 (B = {B}, max_num = {max_num}, Kmax = {Kmax})")
    L = int(G) if group is not None else C
    dets = torch.zeros(B, max_num, 5)
    labels = torch.full((B, max_num), -1, dtype=torch.int32)
    inds = torch.full((B, max_num), -1, dtype=torch.int32)
    counts = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        s, e = min(max(starts[b], 0), K), min(max(starts[b + 1], 0), K)
        n = min(e - s, Kmax) if e > s else 0
        if n == 0:
            continue
        bx, sc = boxes[s:s + n], scores[s:s + n]
        kept_ord, kept_flat, kept_k, kept_lab = [], [], [], []
        for l in range(L):
            col = sc[:, 0] if group is not None else sc[:, l]
            cand = col > score_thr                                        # false for NaN
            if group is not None:
                cand &= group[s:s + n] == l
            idx = torch.nonzero(cand)[:, 0]
            if idx.numel() == 0:
                continue
            o = _ord(col[idx])
            idx = idx[torch.argsort(-o, stable=True)]                     # score descending, ties by ascending row
            lb = bx[idx] if bx.dim() == 2 else bx[idx, l]
            keep = idx[_greedy(lb, iou_thr, max_num)]
            kept_ord.append(_ord(col[keep]))
            kept_flat.append(keep if group is not None else keep * C + l)
            kept_k.append(keep)
            kept_lab.append(torch.full_like(keep, l))
        if not kept_k:
            continue
        o, flat, k, lab = torch.cat(kept_ord), torch.cat(kept_flat), torch.cat(kept_k), torch.cat(kept_lab)
        by_flat = torch.argsort(flat, stable=True)
        order = by_flat[torch.argsort(-o[by_flat], stable=True)][:max_num]  # score descending, ties by ascending flat index
        m = order.numel()
        k, lab = k[order], lab[order]
        dets[b, :m, :4] = bx[k] if bx.dim() == 2 else bx[k, lab]
        dets[b, :m, 4] = sc[k, 0] if group is not None else sc[k, lab]
        labels[b, :m], inds[b, :m], counts[b] = lab.to(torch.int32), (k + s).to(torch.int32), m
    return dets.to(dev), labels.to(dev), inds.to(dev), counts.to(dev)


def delta2bbox_torch(rois, deltas, means, stds, wh_ratio_clip, starts=None, max_shape=None, scale=None):
    """csd_delta2bbox in plain fp32 torch: mmdet 2.x delta2bbox (add_ctr_clamp=False, clip_border=True), op by op, then the division by
    the image's scale factor.  max_shape [B, 2] = (h, w) and scale [B, 4] are per image (tensors or nested lists), with starts [B + 1]."""
    rois, deltas = rois.detach().float(), deltas.detach().float()
    K = rois.shape[0]
    f = lambda v: torch.as_tensor(v, dtype=torch.float32, device=rois.device)
    d = deltas * f(stds) + f(means)
    pxy = (rois[:, :2] + rois[:, 2:4]) * 0.5
    pwh = rois[:, 2:4] - rois[:, :2]
    max_ratio = float(torch.tensor(abs(math.log(float(torch.tensor(wh_ratio_clip, dtype=torch.float32)))), dtype=torch.float32))
    dwh = d[:, 2:].clamp(min=-max_ratio, max=max_ratio)
    gxy = pxy + pwh * d[:, :2]
    half = (pwh * dwh.exp()) * 0.5
    out = torch.cat([gxy - half, gxy + half], dim=1)
    if max_shape is not None or scale is not None:
        st = torch.as_tensor(starts, device=rois.device).to(torch.int64)
        B = st.numel() - 1
        img = (torch.searchsorted(st[1:B].contiguous(), torch.arange(K, device=rois.device), right=True) if B > 1
               else torch.zeros(K, dtype=torch.int64, device=rois.device))
        if max_shape is not None:
            hw = f(max_shape).reshape(B, 2)[img]
            hi = torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], dim=1)
            out = torch.minimum(out.clamp(min=0), hi)
        if scale is not None:
            out = out / f(scale).reshape(B, 4)[img]
    return out


# ================================================================================================ tensor-level entry points
def nms(boxes, scores, starts, Kmax, score_thr, iou_thr, max_num, group=None, G=0, ops=None):
    """Route by tensor: csd_nms on a kernel backend, nms_torch otherwise (and for per-class boxes [K, C, 4])."""
    k_ops = _kernel_ops(boxes, ops) if boxes.dim() == 2 else None
    if k_ops is None:
        return nms_torch(boxes, scores, starts, Kmax, score_thr, iou_thr, max_num, group, G)
    boxes, scores = boxes.detach(), scores.detach()
    if boxes.dtype != torch.float32 or (boxes.shape[0] and boxes.stride(1) != 1):
        boxes = boxes.float().contiguous()
    if scores.dtype != torch.float32 or (scores.shape[0] and scores.stride(1) != 1):
        scores = scores.float().contiguous()
    if group is not None:
        group = group.detach().to(torch.int32).contiguous()
    return k_ops.nms(boxes, scores, as_i32(starts, boxes.device), Kmax, score_thr, iou_thr, max_num, group, G)


def _per_image(v, B, width, device):
    """img_shapes / scale_factors as a device tensor [B, width]: a tensor passes through, a host list is one small copy."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.float32).reshape(B, -1)[:, :width].contiguous()
    rows = [([float(x) for x in r] if hasattr(r, "__len__") else [float(r)] * width)[:width] for r in v]       # (h, w, c) -> (h, w); a scalar scale -> 4
    return torch.tensor(rows, dtype=torch.float32, device=device).reshape(B, width)


def _decode(rois4, deltas, means, stds, wh_ratio_clip, starts, max_shape, scale, ops=None):
    k_ops = _kernel_ops(rois4, ops) if deltas.shape[-1] == 4 else None
    if k_ops is None:
        return delta2bbox_torch(rois4, deltas, means, stds, wh_ratio_clip, starts, max_shape, scale)
    rois4, deltas = rois4.detach(), deltas.detach()
    if rois4.dtype != torch.float32 or (rois4.shape[0] and rois4.stride(1) != 1):
        rois4 = rois4.float().contiguous()
    if deltas.dtype != torch.float32 or (deltas.shape[0] and deltas.stride(1) != 1):
        deltas = deltas.float().contiguous()
    out = torch.empty(rois4.shape[0], 4, dtype=torch.float32, device=rois4.device)
    st = None if starts is None else as_i32(starts, rois4.device)
    return k_ops.delta2bbox(rois4, deltas, out, means, stds, wh_ratio_clip, st, max_shape, scale)


# ================================================================================================ mmdet / mmcv call signatures
def delta2bbox(rois, deltas, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), max_shape=None, wh_ratio_clip=16 / 1000):
    """mmdet 2.x `delta2bbox` for one image: rois [n, 4], deltas [n, 4] (class-agnostic; [n, 4 * C] takes the torch route class by
    class), max_shape = (h, w[, c]) or None -> boxes [n, 4]."""
    n = rois.shape[0]
    if deltas.shape[-1] != 4:
        C = deltas.shape[-1] // 4
        parts = [delta2bbox(rois, deltas[:, 4 * c:4 * c + 4], means, stds, max_shape, wh_ratio_clip) for c in range(C)]
        return torch.cat(parts, dim=1)
    ms = None if max_shape is None else _per_image([list(max_shape)[:2]], 1, 2, rois.device)
    return _decode(rois, deltas, means, stds, wh_ratio_clip, None if ms is None else [0, n], ms, None)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv's `batched_nms`: boxes [n, 4], scores [n], idxs [n] (non-negative integers: class or FPN level) -> (dets [m, 5], keep [m]),
    score descending.  nms_cfg: dict(type='nms', iou_threshold=..., max_num=..., split_thr=... (ignored)).  On the kernel route the
    output needs a bound: max_num, or min(n, 4096) when it is missing -- and a ValueError that asks for it when n > 4096 (the RPN passes
    its max_per_img).  'num_groups' in nms_cfg (an upper bound on idxs + 1) saves the read of idxs.max(); `counts` is read once."""
    nms_cfg = dict(nms_cfg)
    iou_thr = _check_nms_cfg(nms_cfg)
    n = boxes.shape[0]
    max_num = nms_cfg.get("max_num", -1)
    kernel = _kernel_ops(boxes) is not None
    if max_num is None or max_num <= 0:
        if kernel and n > KERNEL_MAX_NUM:
            raise ValueError(f"batched_nms of {n} boxes on the kernel route needs nms_cfg['max_num'] (at most {KERNEL_MAX_NUM}): "
                             f"its outputs have a fixed shape")
        max_num = max(n, 1)
    if kernel and (n > KERNEL_MAX_BOXES or max_num > KERNEL_MAX_NUM):
        raise ValueError(f"the kernel route takes at most {KERNEL_MAX_BOXES} boxes and max_num <= {KERNEL_MAX_NUM} (n = {n}, max_num = {max_num})")
    if n == 0:
        return boxes.new_zeros(0, 5), torch.zeros(0, dtype=torch.int64, device=boxes.device)
    group, G = None, 0
    if not class_agnostic:
        group = idxs
        G = nms_cfg.get("num_groups") or int(idxs.max()) + 1
    dets, _, inds, counts = nms(boxes, scores.reshape(n, 1), [0, n], n, float("-inf"), iou_thr, max_num, group, G)
    m = int(counts[0])
    return dets[0, :m], inds[0, :m].to(torch.int64)


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, return_inds=False):
    """mmdet 2.x `multiclass_nms`: multi_bboxes [n, 4] (or [n, 4 * C]: the torch route), multi_scores [n, C + 1] whose last column
    (background) is dropped -> (dets [m, 5], labels [m]) and, with return_inds, the indices k * C + c into the [n * C] candidate
    grid.  On the kernel route max_num < 0 means min(n * C, 4096) and raises when n * C is larger (module docstring)."""
    if score_factors is not None:
        raise ValueError("score_factors is not implemented (no F-ViT config uses it)")
    iou_thr = _check_nms_cfg(nms_cfg)
    n, C = multi_scores.shape[0], multi_scores.shape[1] - 1
    per_class = multi_bboxes.shape[1] > 4
    boxes = multi_bboxes.reshape(n, C, 4) if per_class else multi_bboxes
    kernel = not per_class and _kernel_ops(boxes) is not None
    inner = _get(nms_cfg, "max_num", -1) or -1
    limits = [v for v in (max_num, inner) if v is not None and v > 0]
    cut = min(limits) if limits else max(n * C, 1)
    if kernel and (cut > KERNEL_MAX_NUM or n > KERNEL_MAX_BOXES):
        raise ValueError(f"multiclass_nms on the kernel route needs max_num <= {KERNEL_MAX_NUM} and at most {KERNEL_MAX_BOXES} boxes "
                         f"(n = {n}, C = {C}, max_num = {max_num}): its outputs have a fixed shape")
    if n == 0 or C == 0:
        out = (multi_bboxes.new_zeros(0, 5), torch.zeros(0, dtype=torch.int64, device=multi_bboxes.device))
        return out + (torch.zeros(0, dtype=torch.int64, device=multi_bboxes.device),) if return_inds else out
    dets, labels, inds, counts = nms(boxes, multi_scores[:, :C], [0, n], n, float(score_thr), iou_thr, cut)
    m = int(counts[0])
    dets, labels, inds = dets[0, :m], labels[0, :m].to(torch.int64), inds[0, :m].to(torch.int64)
    return (dets, labels, inds * C + labels) if return_inds else (dets, labels)


def detections(rois, scores, bbox_pred, img_shapes, scale_factors, score_thr, iou_threshold, max_per_img, means=(0., 0., 0., 0.),
               stds=(0.1, 0.1, 0.2, 0.2), wh_ratio_clip=16 / 1000, starts=None, Kmax=None, ops=None):
    """get_bboxes for all images of a batch, fixed shapes, no read-back on the kernel route: what a serving loop calls.

    rois [K, 5] = (image index, x0, y0, x1, y1), grouped by image in image order (bbox2roi); scores [K, C + 1] (the background column,
    last, is ignored); bbox_pred [K, 4] or None (the rois themselves are the boxes, unclamped -- the reference's clamp_ at
    fvit_head.py:150-151 works on a copy); img_shapes: B x (h, w[, c]) or None; scale_factors: B x 4 (or B scalars) or None = no
    rescale -- host lists or device tensors.  starts [B + 1]: the per-image offsets when the caller has the proposal counts (list or
    int32 tensor); otherwise one searchsorted of rois[:, 0] on the device.  Kmax: a host bound on boxes per image (default K; it sizes
    the workspace, so pass the proposal limit).
    -> dets [B, max_per_img, 5], labels [B, max_per_img], inds [B, max_per_img], counts [B] (include/clipself_det.h)."""
    K, C = scores.shape[0], scores.shape[1] - 1
    if img_shapes is None and scale_factors is None and starts is None:
        raise ValueError("detections needs the number of images: img_shapes, scale_factors or starts")
    B = len(img_shapes) if img_shapes is not None else len(scale_factors) if scale_factors is not None else len(starts) - 1
    dev = rois.device
    if starts is None:
        img_col = rois[:, 0].detach().float().contiguous()
        starts = torch.searchsorted(img_col, torch.arange(B + 1, dtype=torch.float32, device=dev)).to(torch.int32)
    else:
        starts = as_i32(starts, dev)
    ms, sf = _per_image(img_shapes, B, 2, dev), _per_image(scale_factors, B, 4, dev)
    rois4 = rois[:, 1:5]
    if bbox_pred is not None:
        boxes = _decode(rois4, bbox_pred, means, stds, wh_ratio_clip, starts, ms, sf, ops)
    elif sf is not None:
        boxes = rois4.detach().float() / sf[rois[:, 0].detach().long().clamp(0, B - 1)]
    else:
        boxes = rois4
    return nms(boxes, scores[:, :C], starts, K if Kmax is None else int(Kmax), float(score_thr), float(iou_threshold), int(max_per_img),
               ops=ops)
