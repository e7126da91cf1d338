"""Detector mask branch: mask targets, the mask loss with its gradient and the paste of predicted masks, usable without mmcv / mmdet.

What the four OV-LVIS configs of the reference add to the box branch through mmdet 2.28.1: `mask_target` / `BitmapMasks.crop_and_resize`
(train_cfg.rcnn.mask_size = 28), `FCNMaskHead.loss` with CrossEntropyLoss(use_mask=True) (`mask_cross_entropy`, class_agnostic=True) and
`FCNMaskHead.get_seg_masks` / `_do_paste_mask` (test_cfg.rcnn.mask_thr_binary = 0.5).  The contract -- the clip of the box, the RoIAlign
geometry and its separable sum, the BCE and sigmoid expressions, n * M * M as the denominator, torch's grid_sample coordinate and tap
order, the all-zero rules -- is stated once, in include/clipself_mask.h.  mmcv / mmdet are not available to this project: names, keywords
and semantics follow the published mmdet 2.28.1 sources as read (parity-unpinned, like det_post, roi_extractor, det_targets and
det_losses); the two pieces plain torch can express are pinned on torch itself (tests/_mask_ref.py: F.grid_sample for the paste,
F.binary_cross_entropy_with_logits with autograd for the loss).

Two routes.  KERNEL (CUDA tensors on a backend with MASK, HipOps): csm_mask_target / csm_mask_loss / csm_paste_masks, fixed shapes,
nothing read back.  TORCH (CPU tensors, a backend without MASK, or fused=False): `mask_target_torch` / `mask_loss_torch` /
`paste_masks_torch`, the same contract in plain fp32 torch, in chunks of rows so that no [R, H, W] float tensor of the whole batch exists.

A training loop goes `det_targets.rcnn_targets(..., return_gt_inds=True)` -> `mask_target(rois, pos_gt_inds, gt_masks)` -> the mask head
(plain nn.Conv2d + neck.Deconv2x2, left to the loop) -> `mask_loss(mask_pred, mask_targets, labels, row_weights)`, where row_weights is 1
on the positive slots (`(pos_gt_inds >= 0).float()`); a serving loop goes `det_post.detections` -> `paste_masks`.  Neither reads back.

Out of scope: PolygonMasks (the configs load with mmdet's default poly2mask=True), the head's convolutions, RLE encoding, class-specific
paste for more than 4096 classes, mmdet's skip_empty=True CPU path, and mask_thr_binary < 0 (the 0 - 255 soft bytes).
"""
from __future__ import annotations

import torch

from .det_backend import f32c, kernel_ops
from .hip import (MASK_MAX_CLASSES as KERNEL_MAX_CLASSES, MASK_MAX_IMAGE as KERNEL_MAX_IMAGE, MASK_MAX_MASK as KERNEL_MAX_MASK,  # include/clipself_mask.h
                  MASK_MAX_ROWS as KERNEL_MAX_ROWS, MASK_MAX_SIDE as KERNEL_MAX_SIDE)

# fused=None takes the kernels where the backend has them (tools/det_masks_bench.py, profiles/det_masks_bench.md: against the torch route of
# this module on the same device, at every shape measured)
FUSED_MASK_DEFAULT = True

_CHUNK = 32                                                                   # rows per step of the torch route


def _kernel_ops(t, ops=None, fused=None):
    return kernel_ops(t, "MASK", ops, fused, FUSED_MASK_DEFAULT)


# ================================================================================================ mmdet's loss module
class MaskCrossEntropyLoss:
    """mmdet 2.28.1 `CrossEntropyLoss(use_mask=True)` with its constructor keywords (`type` is accepted so that a config dict builds it
    unchanged).  What the kernel does not cover raises ValueError: use_mask=False or use_sigmoid=True (those are `det_losses`'),
    reduction != 'mean', class_weight, avg_non_ignore, an ignore_index other than None / -100."""

    def __init__(self, use_sigmoid=False, use_mask=True, reduction="mean", class_weight=None, ignore_index=None, loss_weight=1.0,
                 avg_non_ignore=False, type=None):
        if type not in (None, "CrossEntropyLoss"):
            raise ValueError(f"type {type!r} is not CrossEntropyLoss")
        if not use_mask or use_sigmoid:
            raise ValueError("the mask loss is CrossEntropyLoss(use_mask=True, use_sigmoid=False); the other forms are det_losses'")
        if reduction != "mean":
            raise ValueError(f"reduction {reduction!r}: only 'mean' is implemented")
        if class_weight is not None:
            raise ValueError("class_weight is not implemented for the mask loss: no F-ViT config uses it")
        if avg_non_ignore:
            raise ValueError("avg_non_ignore=True is not implemented: no F-ViT config uses it")
        if ignore_index not in (None, -100):
            raise ValueError(f"ignore_index {ignore_index!r}: mmdet's mask_cross_entropy accepts none")
        self.use_sigmoid, self.use_mask, self.reduction, self.class_weight = False, True, reduction, None
        self.ignore_index, self.loss_weight, self.avg_non_ignore = ignore_index, float(loss_weight), False


def build_loss(cfg):
    """The mask loss from a config dict such as dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0), or the module itself."""
    if isinstance(cfg, MaskCrossEntropyLoss):
        return cfg
    if not isinstance(cfg, dict):
        raise ValueError(f"loss_mask must be a config dict or a MaskCrossEntropyLoss, got {type(cfg).__name__}")
    if cfg.get("type") != "CrossEntropyLoss":
        raise ValueError(f"loss type {cfg.get('type')!r}: the mask loss is CrossEntropyLoss(use_mask=True)")
    known = ("type", "use_sigmoid", "use_mask", "reduction", "class_weight", "ignore_index", "loss_weight", "avg_non_ignore")
    extra = sorted(k for k in cfg if k not in known)
    if extra:
        raise ValueError(f"unsupported keywords {extra} (avg_factor is not implemented: the factor is n * M * M, taken on the device)")
    return MaskCrossEntropyLoss(**cfg)


# ================================================================================================ the torch route
def _axis_weights(lo_c, hi_c, size, M):
    """The header's per-axis weights for a chunk of boxes: clipped box edges lo_c, hi_c [r] fp32 -> (A [r, M, size] fp32 with
    A[r, p, x] = the tap weights of bin p that land on pixel x, grid [r] int64)."""
    f32, dev = torch.float32, lo_c.device
    start = lo_c - 0.5
    binsz = ((hi_c - 0.5) - start) / float(M)
    grid = torch.ceil(binsz).clamp(min=0).to(torch.int64)
    gmax = max(int(grid.max()) if grid.numel() else 0, 1)
    p = torch.arange(M, dtype=f32, device=dev)[None, :, None]
    i = torch.arange(gmax, dtype=f32, device=dev)[None, None, :]
    gf = grid.clamp(min=1).to(f32)[:, None, None]
    c = (start[:, None, None] + p * binsz[:, None, None]) + ((i + 0.5) * binsz[:, None, None]) / gf
    valid = (c >= -1) & (c <= size) & (i < grid[:, None, None].to(f32))
    c = torch.where(valid & (c > 0), c, torch.zeros_like(c))
    lo = c.to(torch.int64)
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    c = torch.where(edge, lo.to(f32), c)
    w_hi = c - lo.to(f32)
    w_lo = 1.0 - w_hi
    zero = torch.zeros_like(c)
    A = torch.zeros(lo_c.shape[0], M, size, dtype=f32, device=dev)
    A.scatter_add_(2, lo, torch.where(valid, w_lo, zero))
    A.scatter_add_(2, hi, torch.where(valid, w_hi, zero))
    return A, grid


def mask_target_torch(rois, gt_rows, masks, M, soft=False):
    """csm_mask_target in plain fp32 torch -> targets [R, M, M] (uint8, or fp32 with soft=True): the separable form, Ay . m . Ax^T / count,
    in chunks of rows."""
    R = rois.shape[0]
    Gtot, H, W = masks.shape
    dev, f32 = rois.device, torch.float32
    out = torch.zeros(R, M, M, dtype=f32, device=dev)
    rows = gt_rows.to(torch.int64)
    box = rois[:, 1:5].detach().to(f32)
    ok = (rows >= 0) & (rows < Gtot) & torch.isfinite(box).all(dim=1)
    box = torch.where(ok[:, None], box, torch.zeros_like(box))
    rows = torch.where(ok, rows, torch.zeros_like(rows))
    for s in range(0, R if Gtot else 0, _CHUNK):
        b, g = box[s:s + _CHUNK], rows[s:s + _CHUNK]
        Ax, gw = _axis_weights(b[:, 0].clamp(0, W), b[:, 2].clamp(0, W), W, M)
        Ay, gh = _axis_weights(b[:, 1].clamp(0, H), b[:, 3].clamp(0, H), H, M)
        m = (masks[g] != 0).to(f32)                                              # [r, H, W]
        count = (gh * gw).clamp(min=1).to(f32)
        t = torch.bmm(torch.bmm(Ay, m), Ax.transpose(1, 2)) / count[:, None, None]
        out[s:s + _CHUNK] = torch.where((ok[s:s + _CHUNK] & (gh > 0) & (gw > 0))[:, None, None], t, torch.zeros_like(t))
    return out if soft else (out >= 0.5).to(torch.uint8)


def mask_loss_torch(pred, labels, targets, row_weights):
    """csm_mask_loss in plain fp32 torch -> (out2 = (loss, n), dpred [R, C, M, M]): the header's expressions and closed-form gradient;
    rows that are not counted never see their prediction."""
    R, C, M, _ = pred.shape
    dev, f32 = pred.device, torch.float32
    zero = torch.zeros((), dtype=f32, device=dev)
    lab = torch.zeros(R, dtype=torch.int64, device=dev) if labels is None else labels.to(torch.int64)
    counted = (row_weights > 0) & (lab >= 0) & (lab < C)
    n = counted.sum().clamp(min=1).to(f32)
    den = n * float(M * M)
    dpred = torch.zeros_like(pred)
    if R == 0:
        return torch.stack([zero, n]), dpred
    ls = torch.where(counted, lab, torch.zeros_like(lab))
    idx = torch.arange(R, device=dev)
    on = counted[:, None, None]
    x = torch.where(on, pred[idx, ls], zero)
    t = targets.to(f32) if targets.dtype == f32 else (targets != 0).to(f32)
    w = torch.where(counted, row_weights, zero)[:, None, None]
    e = torch.exp(-x.abs())
    bce = (x.clamp(min=0) - x * t) + torch.log1p(e)
    sig = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    loss = torch.where(on, w * bce, zero).sum() / den
    dpred[idx, ls] = torch.where(on, (w * (sig - t)) / den, zero)
    return torch.stack([loss, n]), dpred


def _paste_coord(n, lo, extent, M, dev):
    X = torch.arange(n, dtype=torch.float32, device=dev)[None, :]
    gx = ((X + 0.5) - lo[:, None]) / extent[:, None] * 2 - 1
    return ((gx + 1) * float(M) - 1) / 2


def paste_masks_torch(logits, labels, boxes, img_h, img_w, thr=0.5, return_soft=False):
    """csm_paste_masks in plain fp32 torch -> out [N, img_h, img_w] uint8 (and v, fp32, with return_soft=True), in chunks of detections."""
    N, C, M, _ = logits.shape
    dev, f32 = logits.device, torch.float32
    if not thr >= 0:
        raise ValueError(f"thr = {thr} must be >= 0 (mmdet's soft 0 - 255 bytes are not implemented)")
    out = torch.zeros(N, img_h, img_w, dtype=torch.uint8, device=dev)
    soft = torch.zeros(N, img_h, img_w, dtype=f32, device=dev) if return_soft else None
    lab = torch.zeros(N, dtype=torch.int64, device=dev) if labels is None else labels.to(torch.int64)
    box = boxes.detach().to(f32)
    dx, dy = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    ok = (lab >= 0) & (lab < C) & torch.isfinite(box).all(dim=1) & torch.isfinite(dx) & torch.isfinite(dy) & (dx > 0) & (dy > 0)
    one = torch.ones_like(dx)
    dx, dy = torch.where(ok, dx, one), torch.where(ok, dy, one)
    box = torch.where(ok[:, None], box, torch.zeros_like(box))
    ls = torch.where(ok, lab, torch.zeros_like(lab))
    for s in range(0, N, _CHUNK):
        sl = slice(s, s + _CHUNK)
        x = logits[torch.arange(s, min(s + _CHUNK, N), device=dev), ls[sl]]       # [r, M, M]
        e = torch.exp(-x.abs())
        p = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
        pp = torch.zeros(x.shape[0], M + 2, M + 2, dtype=f32, device=dev)       # zero padding: tap k sits at k + 1
        pp[:, 1:M + 1, 1:M + 1] = p
        ix, iy = _paste_coord(img_w, box[sl, 0], dx[sl], M, dev), _paste_coord(img_h, box[sl, 1], dy[sl], M, dev)
        lx, ly = (ix >= -1) & (ix < M), (iy >= -1) & (iy < M)
        ix, iy = torch.where(lx, ix, torch.zeros_like(ix)), torch.where(ly, iy, torch.zeros_like(iy))
        fx, fy = torch.floor(ix), torch.floor(iy)
        wx1, wx0 = (ix - fx)[:, None, :], ((fx + 1) - ix)[:, None, :]
        wy1, wy0 = (iy - fy)[:, :, None], ((fy + 1) - iy)[:, :, None]
        xi, yi = fx.to(torch.int64)[:, None, :] + 1, fy.to(torch.int64)[:, :, None] + 1
        r = torch.arange(x.shape[0], device=dev)[:, None, None]
        v = (wx0 * wy0) * pp[r, yi, xi] + (wx1 * wy0) * pp[r, yi, xi + 1]
        v = v + (wx0 * wy1) * pp[r, yi + 1, xi]
        v = v + (wx1 * wy1) * pp[r, yi + 1, xi + 1]
        v = torch.where(ok[sl, None, None] & ly[:, :, None] & lx[:, None, :], v, torch.zeros_like(v))
        out[sl] = (v >= thr).to(torch.uint8)
        if return_soft:
            soft[sl] = v
    return (out, soft) if return_soft else out


# ================================================================================================ autograd
class _MaskLossFn(torch.autograd.Function):
    """forward: one call for out2 = (loss, n) and the unit-upstream gradient, which it saves; backward: that gradient times the incoming
    gradient of the loss.  n carries no gradient."""

    @staticmethod
    def forward(ctx, ops, labels, targets, row_weights, pred):
        if ops is not None:
            out2, dpred = ops.mask_loss(pred, labels, targets, row_weights)
        else:
            out2, dpred = mask_loss_torch(pred, labels, targets, row_weights)
        ctx.save_for_backward(dpred)
        return out2

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return None, None, None, None, dpred * g[0]


# ================================================================================================ the forms a training / serving loop calls
def _cat_masks(gt_masks, device):
    if isinstance(gt_masks, torch.Tensor):
        m = gt_masks
    else:
        shapes = {tuple(g.shape[-2:]) for g in gt_masks}
        if len(shapes) > 1:
            raise ValueError(f"mask_target: the images' masks must share one H x W (Pad(size=image_size) guarantees it), got {sorted(shapes)}")
        if not shapes:
            raise ValueError("mask_target: gt_masks is an empty list")
        m = torch.cat([g.reshape(-1, *g.shape[-2:]) for g in gt_masks], dim=0)
    if m.dim() != 3:
        raise ValueError(f"mask_target: gt_masks must be [Gtot, H, W], got {tuple(m.shape)}")
    if m.dtype == torch.bool:
        m = m.view(torch.uint8) if m.is_contiguous() else m.to(torch.uint8)
    if m.dtype != torch.uint8:
        raise ValueError(f"mask_target: gt_masks must be uint8 (or bool), got {m.dtype}")
    return m.to(device)


def mask_target(rois, pos_gt_inds, gt_masks, mask_size=28, soft=False, ops=None, fused=None):
    """mmdet's `mask_target` for all images at once.  rois [R, 5] and pos_gt_inds [R] int32 as `det_targets.rcnn_targets(...,
    return_gt_inds=True)` returns them (-1: not a positive slot -> an all-zero target); gt_masks: a [Gtot, H, W] uint8 tensor in the order
    of the concatenated ground-truth list, or the list of per-image [G_b, H, W] tensors (one H, W for the batch, else ValueError).
    -> mask_targets [R, mask_size, mask_size] uint8, or fp32 with soft=True (mmdet's soft_mask_target)."""
    mask_size = int(mask_size) if not isinstance(mask_size, (tuple, list)) else int(mask_size[0])
    if rois.dim() != 2 or rois.shape[1] != 5 or tuple(pos_gt_inds.shape) != (rois.shape[0],):
        raise ValueError(f"mask_target: rois {tuple(rois.shape)} must be [R, 5] and pos_gt_inds {tuple(pos_gt_inds.shape)} [R]")
    if not 1 <= mask_size <= KERNEL_MAX_MASK:
        raise ValueError(f"mask_target: mask_size = {mask_size} must be in [1, {KERNEL_MAX_MASK}]")
    dev = rois.device
    masks = _cat_masks(gt_masks, dev)
    rois = f32c(rois.detach())
    rows = pos_gt_inds.detach().to(device=dev, dtype=torch.int32).contiguous()
    k_ops = _kernel_ops(rois, ops, fused)
    if k_ops is None:
        return mask_target_torch(rois, rows, masks, mask_size, soft)
    if not (masks.shape[1] <= KERNEL_MAX_SIDE and masks.shape[2] <= KERNEL_MAX_SIDE):
        raise ValueError(f"mask_target: the kernel route takes masks of at most {KERNEL_MAX_SIDE} x {KERNEL_MAX_SIDE}, got {tuple(masks.shape[1:])}")
    if masks.numel() and masks.stride(2) != 1:
        masks = masks.contiguous()
    return k_ops.mask_target(rois, rows, masks, mask_size, soft)


def mask_loss(mask_pred, mask_targets, labels, row_weights, class_agnostic=True, loss_mask=None, ops=None, fused=None):
    """FCNMaskHead.loss.  mask_pred [R, C, M, M] (C = 1 with class_agnostic=True; any float dtype), mask_targets [R, M, M] uint8 or fp32
    (`mask_target`), labels [R] (the slots' classes; not used with class_agnostic=True, where mmdet passes zeros), row_weights [R]: 1 on the
    slots that take part (the positives), 0 elsewhere.  loss_mask: MaskCrossEntropyLoss or its config dict.  The averaging factor
    max(count of counted rows, 1) * M * M is taken on the device.  -> dict(loss_mask=...)."""
    loss = build_loss(loss_mask) if loss_mask is not None else MaskCrossEntropyLoss()
    if mask_pred.dim() != 4 or mask_pred.shape[2] != mask_pred.shape[3]:
        raise ValueError(f"mask_loss: mask_pred must be [R, C, M, M], got {tuple(mask_pred.shape)}")
    R, C, M, _ = mask_pred.shape
    if not (0 <= R <= KERNEL_MAX_ROWS and 1 <= C <= KERNEL_MAX_CLASSES and 1 <= M <= KERNEL_MAX_MASK and R * C * M * M < 1 << 31):
        raise ValueError(f"mask_loss: limits R <= {KERNEL_MAX_ROWS}, C <= {KERNEL_MAX_CLASSES}, M <= {KERNEL_MAX_MASK}, R * C * M * M < 2^31 "
                         f"(got {tuple(mask_pred.shape)})")
    if tuple(mask_targets.shape) != (R, M, M) or tuple(row_weights.shape) != (R,):
        raise ValueError(f"mask_loss: mask_targets must be [R, M, M] and row_weights [R] with R = {R}, M = {M}")
    if not class_agnostic and (labels is None or tuple(labels.shape) != (R,)):
        raise ValueError("mask_loss: class_agnostic=False needs labels [R]")
    dev = mask_pred.device
    tg = mask_targets.detach().to(dev)
    if tg.dtype == torch.bool:
        tg = tg.to(torch.uint8)
    elif tg.dtype != torch.uint8:
        tg = tg.float()
    lab = None if class_agnostic else labels.detach().to(device=dev, dtype=torch.int32).contiguous()
    k_ops = _kernel_ops(mask_pred, ops, fused)
    out2 = _MaskLossFn.apply(k_ops, lab, tg.contiguous(), f32c(row_weights.detach().to(dev)), f32c(mask_pred))
    w = loss.loss_weight
    return dict(loss_mask=out2[0] * w if w != 1.0 else out2[0])


def paste_masks(mask_pred, det_bboxes, det_labels, img_shape, scale_factor=None, thr=0.5, class_agnostic=True, ops=None, fused=None):
    """`_do_paste_mask(skip_empty=False)` and the threshold for all detections of one image.  mask_pred [N, C, M, M] LOGITS (the sigmoid
    is the kernel's), det_bboxes [N, 4(+)] in network-input pixels, det_labels [N], img_shape = (img_h, img_w) of the output;
    scale_factor: None, a number or four numbers the boxes are divided by first (mmdet's rescale=True).  -> [N, img_h, img_w] uint8."""
    if mask_pred.dim() != 4 or mask_pred.shape[2] != mask_pred.shape[3]:
        raise ValueError(f"paste_masks: mask_pred must be [N, C, M, M], got {tuple(mask_pred.shape)}")
    N, C, M, _ = mask_pred.shape
    img_h, img_w = int(img_shape[0]), int(img_shape[1])
    if not thr >= 0:
        raise ValueError(f"paste_masks: thr = {thr} must be >= 0 (mmdet's soft 0 - 255 bytes are not implemented)")
    if not (1 <= img_h <= KERNEL_MAX_IMAGE and 1 <= img_w <= KERNEL_MAX_IMAGE and 1 <= C <= KERNEL_MAX_CLASSES and 1 <= M <= KERNEL_MAX_MASK):
        raise ValueError(f"paste_masks: limits img_h, img_w <= {KERNEL_MAX_IMAGE}, C <= {KERNEL_MAX_CLASSES}, M <= {KERNEL_MAX_MASK}")
    dev = mask_pred.device
    boxes = det_bboxes.detach()[:, :4].to(device=dev, dtype=torch.float32)
    if scale_factor is not None:
        boxes = boxes / torch.as_tensor(scale_factor, dtype=torch.float32, device=dev)
    boxes = boxes.contiguous()
    lab = None if class_agnostic else det_labels.detach().to(device=dev, dtype=torch.int32).contiguous()
    logits = f32c(mask_pred.detach())
    k_ops = _kernel_ops(logits, ops, fused)
    if k_ops is None:
        return paste_masks_torch(logits, lab, boxes, img_h, img_w, thr)
    return k_ops.paste_masks(logits, lab, boxes, img_h, img_w, thr)


def get_seg_masks(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale, num_classes=1203, class_agnostic=True,
                  ops=None, fused=None):
    """mmdet's `FCNMaskHead.get_seg_masks` argument list on top of `paste_masks`: -> num_classes lists of [img_h, img_w] bool numpy arrays,
    detection i in the list of its class.  mask_pred are logits.  Reads back once, at the end."""
    thr = rcnn_test_cfg["mask_thr_binary"] if isinstance(rcnn_test_cfg, dict) else rcnn_test_cfg.mask_thr_binary
    sf = [float(v) for v in (scale_factor.tolist() if hasattr(scale_factor, "tolist") else
                             scale_factor if isinstance(scale_factor, (tuple, list)) else [scale_factor] * 4)]
    if rescale:
        img_h, img_w = int(ori_shape[0]), int(ori_shape[1])
    else:
        img_h, img_w = int(round(ori_shape[0] * sf[1])), int(round(ori_shape[1] * sf[0]))
    masks = paste_masks(mask_pred, det_bboxes, det_labels, (img_h, img_w), sf if rescale else None, thr, class_agnostic, ops, fused)
    masks, labels = masks.cpu().numpy().astype(bool), [int(v) for v in det_labels.cpu().tolist()]
    cls_segms = [[] for _ in range(int(num_classes))]
    for i, l in enumerate(labels):
        cls_segms[l].append(masks[i])
    return cls_segms
