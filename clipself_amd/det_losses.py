"""Detector losses: the RPN's and the box head's losses with their gradients, usable without mmcv / mmdet.

What every F-ViT config runs once per step through mmdet 2.28.1: `RPNHead.loss` (CrossEntropyLoss(use_sigmoid=True) + L1Loss over the
dense targets of `det_targets.rpn_targets`) and `BBoxHead.loss` with reg_class_agnostic=True (the reference's
CustomCrossEntropyLoss(use_sigmoid=False) + L1Loss + accuracy over the rows of `det_targets.rcnn_targets`).  The contract -- the
expressions, the eps of weight_reduce_loss, the class mask, the zero-weight rule, the order of the additions -- is stated once, in
include/clipself_loss.h.  mmcv / mmdet are not available to this project: names, keywords and semantics follow the published mmdet 2.28.1
sources as read (parity-unpinned, like det_post, roi_extractor and det_targets).

Two routes behind one pair of autograd Functions.  KERNEL (CUDA tensors on a backend with LOSS, HipOps): csl_rpn_loss /
csl_bbox_head_loss, one call per head for the losses and the unit-upstream gradients, fixed shapes, nothing read back.  TORCH (CPU tensors,
a backend without LOSS, or fused=False): `rpn_loss_torch` / `bbox_head_loss_torch`, the same contract and the same closed-form gradients in
plain fp32 torch, `torch.where` for the zero-weight rule and no write into the caller's logits.  Both return the losses and the gradients
at unit upstream; backward multiplies the saved gradients by the incoming ones (per level for the RPN); `acc` carries no gradient.

Out of scope: `OpenVocabBoxScores.class_logits` (normalise, matmul, temperature) stays torch and differentiable and feeds
`bbox_head_loss`; the mask head's `mask_cross_entropy` and mask targets; sigmoid / focal box-head losses, SmoothL1, class-specific
regression.
"""
from __future__ import annotations

import json

import torch

from .det_backend import f32c, kernel_ops
from .hip import (LOSS_MAX_ANCHORS as KERNEL_MAX_ANCHORS, LOSS_MAX_CLASSES as KERNEL_MAX_CLASSES, LOSS_MAX_LEVELS as KERNEL_MAX_LEVELS,  # include/clipself_loss.h
                  LOSS_MAX_ROWS as KERNEL_MAX_ROWS, LOSS_MAX_SIDE as KERNEL_MAX_SIDE)
FLT_EPSILON = 2.0 ** -23                                                  # mmdet's eps of weight_reduce_loss, torch.finfo(torch.float32).eps
MASK_BELOW = 1e-5                                                         # CustomCrossEntropyLoss: class_weight < 1e-5 masks the class

# fused=None takes the kernels where the backend has them (tools/det_losses_bench.py, profiles/det_losses_bench.md: forward + backward
# against mmdet's formulation in torch on the device, at every shape measured)
FUSED_LOSS_DEFAULT = True


def _kernel_ops(t, ops=None, fused=None):
    return kernel_ops(t, "LOSS", ops, fused, FUSED_LOSS_DEFAULT)


# ================================================================================================ mmdet's loss modules
def load_class_freq(path="datasets/lvis_v1_train_cat_norare_info.json", freq_weight=1.0, min_count=0):
    """The reference's `load_class_freq`: image counts per category, ordered by category id, to the power freq_weight."""
    with open(path, "r") as f:
        cat_info = json.load(f)
    counts = torch.tensor([max(c["image_count"], min_count) for c in sorted(cat_info, key=lambda x: x["id"])])
    return counts.float() ** freq_weight


class _Loss:
    def _weight_tensor(self, device):
        """class_weight as an fp32 tensor on `device` (cached), or None."""
        if self.class_weight is None:
            return None
        cache = self.__dict__.setdefault("_cw_cache", {})
        key = str(device)
        if key not in cache:
            cache[key] = torch.tensor([float(v) for v in self.class_weight], dtype=torch.float32, device=device)
        return cache[key]


class CrossEntropyLoss(_Loss):
    """mmdet 2.28.1 `CrossEntropyLoss` with its constructor keywords (`type` is accepted so that a config dict builds it unchanged).
    use_sigmoid=True is the RPN's objectness loss (`rpn_loss`), use_sigmoid=False the box head's softmax loss (`bbox_head_loss`).  What
    the kernels do not cover raises ValueError: use_mask=True, reduction != 'mean', avg_non_ignore, an ignore_index other than -100."""
    _type = "CrossEntropyLoss"

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, ignore_index=None, loss_weight=1.0,
                 avg_non_ignore=False, type=None):
        if type not in (None, self._type):
            raise ValueError(f"type {type!r} is not {self._type}")
        if use_mask:
            raise ValueError("use_mask=True (the mask head's mask_cross_entropy) is not implemented")
        if reduction != "mean":
            raise ValueError(f"reduction {reduction!r}: only 'mean' is implemented")
        if avg_non_ignore:
            raise ValueError("avg_non_ignore=True is not implemented: no F-ViT config uses it")
        if ignore_index not in (None, -100):
            raise ValueError(f"ignore_index {ignore_index!r}: only None / -100 is implemented")
        if isinstance(class_weight, str) and self._type != "CustomCrossEntropyLoss":
            raise ValueError("class_weight as a path is CustomCrossEntropyLoss's form")
        self.use_sigmoid, self.use_mask, self.reduction = bool(use_sigmoid), False, reduction
        self.class_weight = None if class_weight is None else class_weight if isinstance(class_weight, str) else [float(v) for v in class_weight]
        self.ignore_index, self.loss_weight, self.avg_non_ignore = ignore_index, float(loss_weight), False
        if self.use_sigmoid and self.class_weight is not None:
            raise ValueError("class_weight with use_sigmoid=True is not implemented (the RPN's loss has none)")


class CustomCrossEntropyLoss(CrossEntropyLoss):
    """The reference's `CustomCrossEntropyLoss` (F-ViT/models/custom_losses.py): classes whose class_weight is below 1e-5 are left out of
    the softmax.  class_weight is a list of C1 weights, or a path read as `load_class_freq` does: 1 for a category with images, 0 for one
    without, and bg_weight for the background at the end."""
    _type = "CustomCrossEntropyLoss"

    def __init__(self, bg_weight=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.bg_weight = float(bg_weight)
        if isinstance(self.class_weight, str):
            self.class_weight = (load_class_freq(self.class_weight, min_count=0) > 0.0).float().tolist() + [self.bg_weight]


class L1Loss(_Loss):
    """mmdet 2.28.1 `L1Loss` with its constructor keywords; reduction != 'mean' raises ValueError."""
    class_weight = None

    def __init__(self, reduction="mean", loss_weight=1.0, type=None):
        if type not in (None, "L1Loss"):
            raise ValueError(f"type {type!r} is not L1Loss")
        if reduction != "mean":
            raise ValueError(f"reduction {reduction!r}: only 'mean' is implemented")
        self.reduction, self.loss_weight = reduction, float(loss_weight)


_LOSSES = {"CrossEntropyLoss": CrossEntropyLoss, "CustomCrossEntropyLoss": CustomCrossEntropyLoss, "L1Loss": L1Loss}


def build_loss(cfg):
    """A loss module from a config dict (`type` names the class), or the module itself."""
    if not isinstance(cfg, dict):
        return cfg
    if cfg.get("type") not in _LOSSES:
        raise ValueError(f"loss type {cfg.get('type')!r} is not one of {sorted(_LOSSES)}")
    return _LOSSES[cfg["type"]](**cfg)


# ================================================================================================ the torch route
def _sign(d):
    one = torch.ones_like(d)
    return torch.where(d > 0, one, torch.where(d < 0, -one, d))              # d == 0 gives 0, a NaN stays a NaN


def rpn_loss_torch(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor):
    """csl_rpn_loss in plain fp32 torch -> (losses [L, 2], dcls list, dreg list): the header's expressions and closed-form gradients.  The
    targets are viewed in the predictions' layout (no copy of a dense map); zero-weight elements never see their prediction."""
    L, B, A = len(cls_scores), cls_scores[0].shape[0], cls_scores[0].shape[1]
    den = avg_factor.reshape(()).to(torch.float32) + FLT_EPSILON
    zero = torch.zeros((), dtype=torch.float32, device=labels.device)
    losses, dcls, dreg, off = [], [], [], 0
    for x, r in zip(cls_scores, bbox_preds):
        h, w = x.shape[2], x.shape[3]
        n = h * w * A
        lab = labels[:, off:off + n].reshape(B, h, w, A).permute(0, 3, 1, 2)
        lw = label_weights[:, off:off + n].reshape(B, h, w, A).permute(0, 3, 1, 2)
        bt = bbox_targets[:, off:off + n].reshape(B, h, w, 4 * A).permute(0, 3, 1, 2)
        bw = bbox_weights[:, off:off + n].reshape(B, h, w, 4 * A).permute(0, 3, 1, 2)
        off += n
        on = (lw != 0) & ((lab == 0) | (lab == 1))
        xs = torch.where(on, x, zero)
        t = (lab == 0).to(torch.float32)
        e = torch.exp(-xs.abs())
        bce = (xs.clamp(min=0) - xs * t) + torch.log1p(e)
        sig = torch.where(xs >= 0, 1 / (1 + e), e / (1 + e))
        lc = torch.where(on, lw * bce, zero).sum() / den
        dcls.append(torch.where(on, (lw * (sig - t)) / den, zero))
        bon = bw != 0
        d = torch.where(bon, r, zero) - torch.where(bon, bt, zero)
        lb = torch.where(bon, bw * d.abs(), zero).sum() / den
        dreg.append(torch.where(bon, (bw * _sign(d)) / den, zero))
        losses.append(torch.stack([lc, lb]))
    return torch.stack(losses), dcls, dreg


def bbox_head_loss_torch(cls_score, labels, label_weights, bbox_pred, bbox_targets, bbox_weights, bg_label, class_weight=None, avg_factor=None):
    """csl_bbox_head_loss in plain fp32 torch -> (out4 = (loss_cls, acc, loss_bbox, avg), dcls [R, C1], dbbox [R, 4])."""
    R, C1 = cls_score.shape
    dev, f32 = cls_score.device, torch.float32
    zero = torch.zeros((), dtype=f32, device=dev)
    if avg_factor is None:
        avg = (label_weights > 0).sum().clamp(min=1).to(f32)
    else:
        avg = avg_factor.reshape(()).to(f32)
    den = avg + FLT_EPSILON
    cw = torch.ones(C1, dtype=f32, device=dev) if class_weight is None else class_weight
    live = ~(cw < MASK_BELOW)                                                  # [C1]
    y = labels.to(torch.int64)
    y_in = (y >= 0) & (y < C1)
    ys = torch.where(y_in, y, torch.zeros_like(y))
    ninf = torch.full((), float("-inf"), dtype=f32, device=dev)
    xm = torch.where(live[None, :], cls_score, ninf)                          # a masked copy: the caller's logits are only read
    # argmax over the unmasked classes, ties to the lowest index, a NaN never wins
    cand = torch.where(torch.isnan(xm), ninf, xm)
    best = cand.max(dim=1, keepdim=True).values
    idx = torch.arange(C1, device=dev)[None, :].expand(R, C1)
    is_best = (cand == best) & live[None, :] & ~torch.isnan(xm)
    arg = torch.where(is_best, idx, torch.full_like(idx, 2 ** 31 - 1)).min(dim=1).values
    hits = ((arg == y) & y_in).sum()
    acc = (100.0 * hits.to(f32) / float(R)) if R else zero
    valid = (label_weights != 0) & y_in & live[ys]
    xv = torch.where(valid[:, None], xm, torch.where(live[None, :], zero, ninf))   # rows that take no part never see their logits
    m = torch.where(valid[:, None], best, zero)
    e = torch.where(live[None, :], torch.exp(xv - m), zero)
    s = e.sum(dim=1)
    xy = xv.gather(1, ys[:, None])[:, 0]
    cwy = cw[ys]
    loss_r = -cwy * ((xy - m[:, 0]) - torch.log(s))
    loss_cls = torch.where(valid, label_weights * loss_r, zero).sum() / den
    coef = torch.where(valid, (label_weights * cwy) / den, zero)
    onehot = (idx == ys[:, None]).to(f32)
    dcls = torch.where(valid[:, None] & live[None, :], coef[:, None] * (e / s[:, None] - onehot), zero)
    pos = (y >= 0) & (y < int(bg_label))
    bon = pos[:, None] & (bbox_weights != 0)
    d = torch.where(bon, bbox_pred, zero) - torch.where(bon, bbox_targets, zero)
    terms = torch.where(bon, bbox_weights * d.abs(), zero)
    rows = ((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]
    rden = torch.tensor(float(R), dtype=f32, device=dev) + FLT_EPSILON
    loss_bbox = rows.sum() / rden
    dbbox = torch.where(bon, (bbox_weights * _sign(d)) / rden, zero)
    return torch.stack([loss_cls, acc.reshape(()), loss_bbox, avg]), dcls, dbbox


# ================================================================================================ autograd
class _RpnLossFn(torch.autograd.Function):
    """forward: one call for the [L, 2] losses and the unit-upstream gradients, which it saves; backward: level l's gradients times the
    incoming gradients of its two losses."""

    @staticmethod
    def forward(ctx, ops, L, labels, label_weights, bbox_targets, bbox_weights, avg_factor, *preds):
        cls_scores, bbox_preds = preds[:L], preds[L:]
        if ops is not None:
            losses, dcls, dreg = ops.rpn_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor)
        else:
            losses, dcls, dreg = rpn_loss_torch(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor)
        ctx.L = L
        ctx.save_for_backward(*dcls, *dreg)
        return losses

    @staticmethod
    def backward(ctx, g):
        L, saved = ctx.L, ctx.saved_tensors
        out = [saved[l] * g[l, 0] for l in range(L)] + [saved[L + l] * g[l, 1] for l in range(L)]
        return (None,) * 7 + tuple(out)


class _HeadLossFn(torch.autograd.Function):
    """forward: one call for out4 = (loss_cls, acc, loss_bbox, avg) and the unit-upstream gradients; backward: dcls times the incoming
    gradient of loss_cls, dbbox times that of loss_bbox.  acc and avg carry no gradient."""

    @staticmethod
    def forward(ctx, ops, bg_label, labels, label_weights, bbox_targets, bbox_weights, class_weight, avg_factor, cls_score, bbox_pred):
        if ops is not None:
            out4, dcls, dbbox = ops.bbox_head_loss(cls_score, labels, label_weights, bbox_pred, bbox_targets, bbox_weights, bg_label, class_weight,
                                                   avg_factor)
        else:
            out4, dcls, dbbox = bbox_head_loss_torch(cls_score, labels, label_weights, bbox_pred, bbox_targets, bbox_weights, bg_label,
                                                     class_weight, avg_factor)
        ctx.save_for_backward(dcls, dbbox)
        return out4

    @staticmethod
    def backward(ctx, g):
        dcls, dbbox = ctx.saved_tensors
        return (None,) * 8 + (dcls * g[0], dbbox * g[2])


# ================================================================================================ the batched forms a training loop calls
def _targets(dev, labels, label_weights, bbox_targets, bbox_weights):
    return (labels.detach().to(device=dev, dtype=torch.int32).contiguous(), f32c(label_weights.detach().to(dev)),
            f32c(bbox_targets.detach().to(dev)), f32c(bbox_weights.detach().to(dev)))


def rpn_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, num_total_samples, loss_cls=None, loss_bbox=None,
             ops=None, fused=None):
    """RPNHead.loss for all levels and images.  cls_scores[l] [B, A, h, w], bbox_preds[l] [B, 4A, h, w] (the RPN head's outputs, any
    float dtype); labels, label_weights [B, N], bbox_targets, bbox_weights [B, N, 4] and num_total_samples as `det_targets.rpn_targets`
    returns them (the count is converted on the device).  loss_cls: CrossEntropyLoss(use_sigmoid=True) or its config dict, loss_bbox:
    L1Loss or its dict.  -> dict(loss_rpn_cls=[L scalars], loss_rpn_bbox=[L scalars]), as mmdet returns them."""
    loss_cls = build_loss(loss_cls) if loss_cls is not None else CrossEntropyLoss(use_sigmoid=True)
    loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else L1Loss()
    if not (isinstance(loss_cls, CrossEntropyLoss) and loss_cls.use_sigmoid and loss_cls.class_weight is None):
        raise ValueError("rpn_loss: loss_cls must be CrossEntropyLoss(use_sigmoid=True) without class_weight")
    if not isinstance(loss_bbox, L1Loss):
        raise ValueError("rpn_loss: loss_bbox must be L1Loss")
    L = len(cls_scores)
    if not (1 <= L <= KERNEL_MAX_LEVELS and len(bbox_preds) == L):
        raise ValueError(f"rpn_loss: {L} cls maps and {len(bbox_preds)} reg maps (1 <= L <= {KERNEL_MAX_LEVELS})")
    dev = cls_scores[0].device
    B, A = cls_scores[0].shape[0], cls_scores[0].shape[1]
    N = 0
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        if c.dim() != 4 or c.shape[:2] != (B, A) or tuple(r.shape) != (B, 4 * A, c.shape[2], c.shape[3]):
            raise ValueError(f"rpn_loss: level {l}: cls {tuple(c.shape)} and reg {tuple(r.shape)} must be [B, A, h, w] and [B, 4A, h, w]")
        if not (1 <= c.shape[2] <= KERNEL_MAX_SIDE and 1 <= c.shape[3] <= KERNEL_MAX_SIDE):
            raise ValueError(f"rpn_loss: level {l}: h, w = {tuple(c.shape[2:])} must be in [1, {KERNEL_MAX_SIDE}]")
        N += c.shape[2] * c.shape[3] * A
    if not 1 <= A <= KERNEL_MAX_ANCHORS:
        raise ValueError(f"rpn_loss: A = {A} must be in [1, {KERNEL_MAX_ANCHORS}]")
    if tuple(labels.shape) != (B, N) or tuple(label_weights.shape) != (B, N) or tuple(bbox_targets.shape) != (B, N, 4) or tuple(bbox_weights.shape) != (B, N, 4):
        raise ValueError(f"rpn_loss: the targets must be [B, N] / [B, N, 4] with B = {B}, N = {N} (the levels' h * w * A), got "
                         f"{tuple(labels.shape)}, {tuple(label_weights.shape)}, {tuple(bbox_targets.shape)}, {tuple(bbox_weights.shape)}")
    k_ops = _kernel_ops(cls_scores[0], ops, fused)
    lab, lw, bt, bw = _targets(dev, labels, label_weights, bbox_targets, bbox_weights)
    avg = torch.as_tensor(num_total_samples, device=dev).detach().to(torch.float32).reshape(1)
    preds = [f32c(c) for c in cls_scores] + [f32c(r) for r in bbox_preds]
    losses = _RpnLossFn.apply(k_ops, L, lab, lw, bt, bw, avg, *preds)
    wc, wb = loss_cls.loss_weight, loss_bbox.loss_weight
    return dict(loss_rpn_cls=[losses[l, 0] * wc if wc != 1.0 else losses[l, 0] for l in range(L)],
                loss_rpn_bbox=[losses[l, 1] * wb if wb != 1.0 else losses[l, 1] for l in range(L)])


def bbox_head_loss(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, loss_cls=None, loss_bbox=None, num_classes=65,
                   ops=None, fused=None):
    """BBoxHead.loss with reg_class_agnostic=True.  cls_score [R, C1] (C1 = num_classes + 1; `OpenVocabBoxScores.class_logits`), bbox_pred
    [R, 4]; labels, label_weights [R], bbox_targets, bbox_weights [R, 4] as `det_targets.rcnn_targets` returns them.  loss_cls:
    CustomCrossEntropyLoss / CrossEntropyLoss with use_sigmoid=False or its config dict, loss_bbox: L1Loss or its dict.  The averaging
    factor max(count(label_weights > 0), 1) is taken on the device.  -> dict(loss_cls, acc, loss_bbox)."""
    loss_cls = build_loss(loss_cls) if loss_cls is not None else CrossEntropyLoss()
    loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else L1Loss()
    if not isinstance(loss_cls, CrossEntropyLoss) or loss_cls.use_sigmoid:
        raise ValueError("bbox_head_loss: loss_cls must be a CrossEntropyLoss / CustomCrossEntropyLoss with use_sigmoid=False "
                         "(sigmoid and focal box-head losses are not implemented)")
    if not isinstance(loss_bbox, L1Loss):
        raise ValueError("bbox_head_loss: loss_bbox must be L1Loss")
    if cls_score.dim() != 2 or bbox_pred.dim() != 2 or bbox_pred.shape != (cls_score.shape[0], 4):
        raise ValueError(f"bbox_head_loss: cls_score {tuple(cls_score.shape)} must be [R, C1] and bbox_pred {tuple(bbox_pred.shape)} [R, 4] "
                         "(class-specific regression is not implemented)")
    R, C1 = cls_score.shape
    if not (0 <= R <= KERNEL_MAX_ROWS and 1 <= C1 <= KERNEL_MAX_CLASSES):
        raise ValueError(f"bbox_head_loss: R = {R} must be in [0, {KERNEL_MAX_ROWS}] and C1 = {C1} in [1, {KERNEL_MAX_CLASSES}]")
    if tuple(labels.shape) != (R,) or tuple(label_weights.shape) != (R,) or tuple(bbox_targets.shape) != (R, 4) or tuple(bbox_weights.shape) != (R, 4):
        raise ValueError(f"bbox_head_loss: the targets must be [R] / [R, 4] with R = {R}")
    dev = cls_score.device
    cw = loss_cls._weight_tensor(dev)
    if cw is not None and cw.numel() != C1:
        raise ValueError(f"bbox_head_loss: class_weight has {cw.numel()} entries for {C1} classes")
    k_ops = _kernel_ops(cls_score, ops, fused)
    lab, lw, bt, bw = _targets(dev, labels, label_weights, bbox_targets, bbox_weights)
    out4 = _HeadLossFn.apply(k_ops, int(num_classes), lab, lw, bt, bw, cw, None, f32c(cls_score), f32c(bbox_pred))
    wc, wb = loss_cls.loss_weight, loss_bbox.loss_weight
    return dict(loss_cls=out4[0] * wc if wc != 1.0 else out4[0], acc=out4[1].detach(), loss_bbox=out4[2] * wb if wb != 1.0 else out4[2])
