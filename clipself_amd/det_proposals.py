"""RPN proposals: the RPN head's dense maps -> proposals per image, usable without mmcv / mmdet.

What `train_cfg.rpn_proposal` and `test_cfg.rpn` configure in every F-ViT config of the reference: mmdet 2.28.1's `RPNHead.get_bboxes` /
`simple_test_rpn`, i.e. `_get_bboxes_single` (sigmoid, the `nms_pre` best anchors of each level, `DeltaXYWHBBoxCoder.decode` against the
image shape) followed by `_bbox_post_process` (the `min_bbox_size` filter, `batched_nms` by level, the cut to `max_per_img`).  The contract
of the first half -- lists, selection order, ties, output rows, arithmetic -- is stated once, in include/clipself_rpn.h; the second half is
the group form of include/clipself_det.h.

Two routes for the first half.  KERNEL (CUDA tensors on a backend with RPN, HipOps): csp_select, one call for all images and levels.
TORCH (`select_torch`: CPU tensors, a backend without RPN, fused=False): the same contract in plain fp32 torch, level by level with the
images batched -- a sigmoid, a stable sort of the integer keys, gathers and a decode per level, mmdet's formulation without its loop over
the images.  Both hand fixed-shape tensors to `det_post.nms`, so on the kernel route `rpn_proposals` reads nothing back and
`det_targets.rcnn_targets(proposal_counts=)` continues on the device.

Differences from mmdet, all inside what it leaves open: the selection is on the logit with ties to the lower anchor index (mmdet sorts the
rounded sigmoid with an unstable sort), NMS runs per level on the un-offset boxes (det_post), and the outputs have fixed shapes with
`counts`.  Not implemented (ValueError): a softmax RPN, nms_pre <= 0, with_nms=False, mmdet's deprecated nms_thr / max_num keys.
"""
from __future__ import annotations

import math

import torch

from . import det_post
from .det_backend import f32c, kernel_ops
# include/clipself_rpn.h: PRE bounds nms_pre, ROWS bounds Ktot (the Kmax of clipself_det.h)
from .hip import (RPN_MAX_ANCHORS as KERNEL_MAX_ANCHORS, RPN_MAX_LEVELS as KERNEL_MAX_LEVELS, RPN_MAX_PRE as KERNEL_MAX_PRE,
                  RPN_MAX_ROWS as KERNEL_MAX_ROWS, RPN_MAX_SIDE as KERNEL_MAX_SIDE)

# fused=None takes csp_select where the backend has it (tools/det_proposals_bench.py, profiles/det_proposals_bench.md: against
# select_torch on the same device, at both shapes measured)
FUSED_PROPOSALS_DEFAULT = True


def _kernel_ops(t, ops=None, fused=None):
    return kernel_ops(t, "RPN", ops, fused, FUSED_PROPOSALS_DEFAULT)


# ================================================================================================ shapes and cfg
def _layout(cls_scores, bbox_preds, anchors, nms_pre):
    """-> (L, B, A, [(h, w, n, k)], N, Ktot) after the checks of the header's limits."""
    L = len(cls_scores)
    if not (1 <= L <= KERNEL_MAX_LEVELS and len(bbox_preds) == L):
        raise ValueError(f"{L} cls maps and {len(bbox_preds)} reg maps (1 <= L <= {KERNEL_MAX_LEVELS})")
    nms_pre = int(nms_pre)
    if not 1 <= nms_pre <= KERNEL_MAX_PRE:
        raise ValueError(f"nms_pre = {nms_pre} must be in [1, {KERNEL_MAX_PRE}]")
    if cls_scores[0].dim() != 4:
        raise ValueError(f"level 0: cls must be [B, A, h, w], got {tuple(cls_scores[0].shape)}")
    B, A = int(cls_scores[0].shape[0]), int(cls_scores[0].shape[1])
    if not (1 <= B <= 65535 and 1 <= A <= KERNEL_MAX_ANCHORS):
        raise ValueError(f"B = {B} must be in [1, 65535] and A = {A} in [1, {KERNEL_MAX_ANCHORS}]")
    dims, N, Ktot = [], 0, 0
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        if c.dim() != 4 or c.shape[0] != B or c.shape[1] != A:
            raise ValueError(f"level {l}: cls must be [{B}, {A}, h, w], got {tuple(c.shape)}")
        h, w = int(c.shape[2]), int(c.shape[3])
        if tuple(r.shape) != (B, 4 * A, h, w):
            raise ValueError(f"level {l}: reg must be {(B, 4 * A, h, w)}, got {tuple(r.shape)}")
        if not (1 <= h <= KERNEL_MAX_SIDE and 1 <= w <= KERNEL_MAX_SIDE):
            raise ValueError(f"level {l}: h = {h}, w = {w} must be in [1, {KERNEL_MAX_SIDE}]")
        n = h * w * A
        dims.append((h, w, n, min(nms_pre, n)))
        N += n
        Ktot += min(nms_pre, n)
    if Ktot > KERNEL_MAX_ROWS:
        raise ValueError(f"Ktot = {Ktot} selected rows per image, at most {KERNEL_MAX_ROWS}")
    if anchors.dim() != 2 or anchors.shape[0] != N or anchors.shape[1] < 4:
        raise ValueError(f"anchors must be [N = {N}, >= 4] (all levels one after another), got {tuple(anchors.shape)}")
    return L, B, A, dims, N, Ktot


def check_cfg(cfg):
    """cfg = dict(nms_pre, max_per_img, nms=dict(type='nms', iou_threshold), min_bbox_size), as the reference's configs write it.
    -> (nms_pre, max_per_img, iou_threshold, min_bbox_size); ValueError for anything else."""
    if not isinstance(cfg, dict):
        try:
            cfg = dict(cfg)
        except (TypeError, ValueError):
            raise ValueError(f"cfg must be a dict, got {type(cfg).__name__}") from None
    unknown = sorted(set(cfg) - {"nms_pre", "max_per_img", "nms", "min_bbox_size"})
    if unknown:
        raise ValueError(f"cfg keys {unknown} are not implemented (known: nms_pre, max_per_img, nms, min_bbox_size)")
    for key in ("nms_pre", "max_per_img", "nms"):
        if key not in cfg:
            raise ValueError(f"cfg needs {key!r}")
    nms = cfg["nms"]
    if not isinstance(nms, dict):
        raise ValueError(f"cfg['nms'] must be a dict, got {type(nms).__name__}")
    if nms.get("type", "nms") != "nms":
        raise ValueError(f"cfg['nms'] type {nms.get('type')!r}: only 'nms' (greedy hard NMS) is implemented")
    unknown = sorted(set(nms) - {"type", "iou_threshold"})
    if unknown:
        raise ValueError(f"cfg['nms'] keys {unknown} are not implemented (known: type, iou_threshold)")
    if "iou_threshold" not in nms:
        raise ValueError("cfg['nms'] needs iou_threshold")
    nms_pre, max_per_img = cfg["nms_pre"], cfg["max_per_img"]
    if int(nms_pre) != nms_pre or not 1 <= int(nms_pre) <= KERNEL_MAX_PRE:
        raise ValueError(f"nms_pre = {nms_pre} must be an integer in [1, {KERNEL_MAX_PRE}] (nms_pre <= 0, mmdet's 'keep all', is not implemented)")
    if int(max_per_img) != max_per_img or not 1 <= int(max_per_img) <= det_post.KERNEL_MAX_NUM:
        raise ValueError(f"max_per_img = {max_per_img} must be an integer in [1, {det_post.KERNEL_MAX_NUM}]")
    iou = float(nms["iou_threshold"])
    if not 0.0 <= iou <= 1.0:
        raise ValueError(f"iou_threshold = {iou} must be in [0, 1]")
    min_size = float(cfg.get("min_bbox_size", 0))
    if not math.isfinite(min_size):
        raise ValueError(f"min_bbox_size = {min_size} must be finite")
    return int(nms_pre), int(max_per_img), iou, min_size


def _max_shape(img_shapes, B, device):
    if img_shapes is not None and len(img_shapes) != B:
        raise ValueError(f"img_shapes must give (h, w) for each of the {B} images, got {len(img_shapes)}")
    return det_post._per_image(img_shapes, B, 2, device)


# ================================================================================================ the torch route
def _keys(x):
    """fp32 logits -> int64 keys in [0, 2^32): ~ord(x), smallest = best; NaN -> 0xFFFFFFFF."""
    k = 0xFFFFFFFF - det_post._ord(x)
    return torch.where(torch.isnan(x), torch.full_like(k, 0xFFFFFFFF), k)


def select_torch(cls_scores, bbox_preds, anchors, max_shape, nms_pre, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000,
                 min_bbox_size=0.0):
    """csp_select in plain fp32 torch on the tensors' device: every product and sum is a torch op of its own.  max_shape [B, 2] tensor or
    None.  -> boxes [B, Ktot, 4], scores [B, Ktot], levels [B, Ktot] int32, anchor_inds [B, Ktot] int32."""
    L, B, A, dims, N, Ktot = _layout(cls_scores, bbox_preds, anchors, nms_pre)
    dev = cls_scores[0].device
    f = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)
    anchors = anchors.detach()[:, :4].to(device=dev, dtype=torch.float32)
    mean, std = f(means), f(stds)
    max_ratio = float(torch.tensor(abs(math.log(float(torch.tensor(wh_ratio_clip, dtype=torch.float32)))), dtype=torch.float32))
    min_size = float(torch.tensor(min_bbox_size, dtype=torch.float32))
    boxes, scores, levels, inds = [], [], [], []
    anc0 = 0
    for l, (h, w, n, k) in enumerate(dims):
        x = cls_scores[l].detach().float().permute(0, 2, 3, 1).reshape(B, n)
        order = torch.sort(_keys(x), dim=1, stable=True).indices[:, :k]                      # best first, ties by ascending anchor index
        x = x.gather(1, order)
        e = torch.exp(-x.abs())
        sc = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        sc = torch.where(torch.isnan(x), x, sc)
        reg = bbox_preds[l].detach().float().reshape(B, A, 4, h, w).permute(0, 3, 4, 1, 2).reshape(B, n, 4)
        d = reg.gather(1, order[:, :, None].expand(B, k, 4)) * std + mean
        a = anchors[anc0:anc0 + n][order]                                                   # [B, k, 4]
        pxy = (a[..., :2] + a[..., 2:]) * 0.5
        pwh = a[..., 2:] - a[..., :2]
        dwh = d[..., 2:].clamp(min=-max_ratio, max=max_ratio)
        gxy = pxy + pwh * d[..., :2]
        half = (pwh * dwh.exp()) * 0.5
        bx = torch.cat([gxy - half, gxy + half], dim=-1)
        if max_shape is not None:
            hw = max_shape.to(device=dev, dtype=torch.float32).reshape(B, 1, 2)
            hi = torch.cat([hw[..., 1:], hw[..., :1], hw[..., 1:], hw[..., :1]], dim=-1)
            bx = torch.minimum(bx.clamp(min=0), hi)
        lev = torch.full((B, k), l, dtype=torch.int32, device=dev)
        if min_size >= 0:
            ok = ((bx[..., 2] - bx[..., 0]) > min_size) & ((bx[..., 3] - bx[..., 1]) > min_size)
            lev = torch.where(ok, lev, torch.full_like(lev, -1))
        boxes.append(bx)
        scores.append(sc)
        levels.append(lev)
        inds.append((order + anc0).to(torch.int32))
        anc0 += n
    return torch.cat(boxes, 1), torch.cat(scores, 1), torch.cat(levels, 1), torch.cat(inds, 1)


# ================================================================================================ entry points
def _select(cls_scores, bbox_preds, anchors, img_shapes, nms_pre, means, stds, wh_ratio_clip, min_bbox_size, ops, fused):
    """-> (boxes, scores, levels, anchor_inds as `select` returns them, starts [B + 1] int32 or None on the torch route)."""
    L, B, A, dims, N, Ktot = _layout(cls_scores, bbox_preds, anchors, nms_pre)
    dev = cls_scores[0].device
    ms = _max_shape(img_shapes, B, dev)
    k_ops = _kernel_ops(cls_scores[0], ops, fused)
    if k_ops is None:
        return select_torch(cls_scores, bbox_preds, anchors, ms, nms_pre, means, stds, wh_ratio_clip, min_bbox_size) + (None,)
    anc = anchors.detach().to(device=dev)
    if anc.dtype != torch.float32 or anc.stride(1) != 1:
        anc = anc.float().contiguous()
    boxes, scores, group, inds, starts = k_ops.rpn_select([f32c(c.detach()) for c in cls_scores], [f32c(r.detach()) for r in bbox_preds], anc,
                                                          nms_pre, means, stds, wh_ratio_clip, ms, min_bbox_size)
    return boxes.view(B, Ktot, 4), scores.view(B, Ktot), group.view(B, Ktot), inds.view(B, Ktot), starts


def select(cls_scores, bbox_preds, anchors, img_shapes, nms_pre, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000,
           min_bbox_size=0, ops=None, fused=None):
    """The nms_pre best anchors of every (image, level), decoded against the image shape and filtered by min_bbox_size
    (include/clipself_rpn.h).  cls_scores[l] [B, A, h, w], bbox_preds[l] [B, 4A, h, w] (any float dtype: converted, as rpn_loss does);
    anchors [N, 4], all levels one after another; img_shapes: B tuples (h, w[, c]), a [B, 2] tensor, or None for no clamp.
    -> boxes [B, Ktot, 4], scores [B, Ktot], levels [B, Ktot] int32 (-1: dropped by the filter), anchor_inds [B, Ktot] int32."""
    return _select(cls_scores, bbox_preds, anchors, img_shapes, nms_pre, means, stds, wh_ratio_clip, float(min_bbox_size), ops, fused)[:4]


def rpn_proposals(cls_scores, bbox_preds, anchors, img_shapes, cfg, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000,
                  ops=None, fused=None, return_inds=False):
    """RPNHead.get_bboxes for all images: `select`, then NMS per level and the cut to cfg.max_per_img (det_post.nms in the group form with
    score_thr = -1, G = L, Kmax = Ktot).  -> proposals [B, max_per_img, 5] (x0, y0, x1, y1, score; rows past the count are zero) and counts
    [B] int32; return_inds=True adds levels and anchor_inds [B, max_per_img] int32 (-1 past the count).  Fixed shapes; on the kernel route
    nothing is read back.

    mmdet runs one batched_nms over the image and returns dets[:max_per_img], the best max_per_img of everything kept.  Here every
    level's list stops after max_per_img keeps and the per-image top-k follows.  The two are equal: a kept box that is among the image's
    best max_per_img kept boxes has fewer than max_per_img better kept boxes in the image, hence in its own level, so it is among its own
    list's first max_per_img keeps; and greedy NMS decides a box from the better boxes of its list only, so stopping a list early changes
    nothing before the stop."""
    nms_pre, max_per_img, iou_thr, min_size = check_cfg(cfg)
    boxes, scores, levels, inds, starts = _select(cls_scores, bbox_preds, anchors, img_shapes, nms_pre, means, stds, wh_ratio_clip, min_size,
                                                  ops, fused)
    B, Ktot = scores.shape
    L = len(cls_scores)
    if starts is None:
        starts = torch.arange(B + 1, dtype=torch.int32, device=scores.device) * Ktot
    dets, labels, rows, counts = det_post.nms(boxes.reshape(B * Ktot, 4), scores.reshape(B * Ktot, 1), starts, Ktot, -1.0, iou_thr, max_per_img,
                                              levels.reshape(B * Ktot), L, ops)
    if not return_inds:
        return dets, counts
    picked = inds.reshape(-1)[rows.clamp(min=0).to(torch.int64)]
    return dets, counts, labels, torch.where(rows >= 0, picked, torch.full_like(picked, -1))


def get_bboxes(cls_scores, bbox_preds, anchors_or_generator, img_metas, cfg, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.),
               wh_ratio_clip=16 / 1000, ops=None, fused=None):
    """mmdet's return: a list of [n_b, 5] tensors (x0, y0, x1, y1, score), one per image, with one read of `counts`.
    anchors_or_generator: the concatenated anchors [N, 4], or a det_targets.AnchorGenerator; img_metas: dicts with 'img_shape'."""
    dev = cls_scores[0].device
    anchors = anchors_or_generator
    if hasattr(anchors, "grid_priors"):
        sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
        anchors = torch.cat(anchors.grid_priors(sizes, device=dev), dim=0)
    shapes = [tuple(m["img_shape"])[:2] for m in img_metas]
    if len(shapes) != cls_scores[0].shape[0]:
        raise ValueError(f"{len(shapes)} img_metas for {cls_scores[0].shape[0]} images")
    dets, counts = rpn_proposals(cls_scores, bbox_preds, anchors, shapes, cfg, means, stds, wh_ratio_clip, ops, fused)
    return [dets[b, :n] for b, n in enumerate(counts.tolist())]
