"""Detector RoI extractor: multi-level RoIAlign between the FPN and the heads, usable without mmcv / mmdet / torchvision.

`self.bbox_roi_extractor(x[:num_inputs], rois)` of the reference's F-ViT/models/fvit_head.py:267-277 (FViTRoIHead._bbox_forward): mmdet
2.x `SingleRoIExtractor` -- a box goes to the FPN level its size asks for (`map_roi_levels`) -- over mmcv 1.x
`RoIAlign(output_size, sampling_ratio, aligned=True, pool_mode='avg')`.  The contract -- level, sample coordinates, bilinear rule,
bounded boxes, the backward's order -- is stated once, in include/clipself_roi.h.  PARITY UNPINNED: mmcv and mmdet are restated from their
published sources, not run.

Two routes.  KERNEL (CUDA tensors on a backend with ROI_EXTRACT, HipOps): csr_roi_extract_fwd / csr_roi_extract_bwd under one
torch.autograd.Function -- all levels in one launch, the level chosen on the device (mmdet reads a `nonzero()` per level back), the
backward a gather without floating-point atomics.  The kernels work on channel-last maps: NCHW maps are brought there with
`contiguous(memory_format=torch.channels_last)` (no copy when they already are), the result is a [K, C, P, P] tensor with channel-last
strides, and so are the gradients.  TORCH (CPU tensors, a backend without ROI_EXTRACT): `roi_extract_torch`, the same contract in plain
differentiable fp32 torch, a Python loop over the boxes.  It is the SLOW route: it exists so that the module works everywhere and as
the second implementation the kernels are measured against (tools/roi_extract_bench.py).
"""
from __future__ import annotations

import torch
from torch import nn

from .det_backend import kernel_ops
from .hip import ROI_MAX_LEVELS as KERNEL_MAX_LEVELS, ROI_MAX_P as KERNEL_MAX_OUTPUT, ROI_MAX_SR as KERNEL_MAX_SAMPLING  # include/clipself_roi.h


def _kernel_ops(t, ops=None):
    return kernel_ops(t, "ROI_EXTRACT", ops)


def bbox2roi(bbox_list):
    """mmdet's `bbox2roi`: a list of per-image boxes [n_i, >= 4] -> rois [K, 5] = (image index, x0, y0, x1, y1), grouped by image."""
    parts = []
    for i, b in enumerate(bbox_list):
        if b.shape[0] > 0:
            parts.append(torch.cat([b.new_full((b.shape[0], 1), i), b[:, :4]], dim=1))
        else:
            parts.append(b.new_zeros((0, 5)))
    return torch.cat(parts, dim=0)


def map_roi_levels_torch(rois, num_levels, finest_scale=56):
    """The header's level rule in fp32 torch, op by op: floor(log2(sqrt(area) / finest_scale + 1e-6)) clamped to [0, num_levels - 1];
    a NaN (negative or non-finite area) is level 0.  -> int64 [K]."""
    r = rois.detach().float()
    scale = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    t = torch.floor(torch.log2(scale / float(finest_scale) + 1e-6))
    t = torch.where(t >= 1, t.clamp(max=float(num_levels - 1)), torch.zeros_like(t))
    return t.to(torch.int64)


# ================================================================================================ the torch route
def _axis_torch(start, binsz, grid, P, size):
    """All P * grid samples of one axis, ascending (p, i): -> (valid, lo, hi, w_lo, w_hi), fp32, one rounded operation per torch op."""
    p = torch.arange(P, dtype=torch.float32).repeat_interleave(grid)
    i = torch.arange(grid, dtype=torch.float32).repeat(P)
    c = (start + p * binsz) + ((i + 0.5) * binsz) / float(grid)
    valid = (c >= -1.0) & (c <= float(size))
    c = torch.where(c <= 0, torch.zeros_like(c), c)
    c = torch.where(valid, c, torch.zeros_like(c))
    lo = c.to(torch.int64)
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    c = torch.where(edge, lo.to(torch.float32), c)
    w_hi = c - lo.to(torch.float32)
    w_lo = 1.0 - w_hi
    return valid, lo, hi, w_lo, w_hi


def roi_extract_torch(feats, rois, output_size, sampling_ratio, featmap_strides, finest_scale=56):
    """include/clipself_roi.h in plain fp32 torch (module docstring: the slow route), differentiable with respect to feats.
    feats: L maps [B, C, h_l, w_l]; rois [K, 5] -> [K, C, P, P]."""
    P, L = int(output_size), len(feats)
    dev = feats[0].device
    maps = [f.float().cpu().permute(0, 2, 3, 1) for f in feats]                      # [B, h, w, C] views: a tap is maps[l][b, y, x]
    B, C = maps[0].shape[0], maps[0].shape[3]
    r = rois.detach().float().cpu()
    K = r.shape[0]
    lvls = map_roi_levels_torch(r, L, finest_scale).tolist()
    scales = [torch.tensor(1.0 / float(s), dtype=torch.float64).to(torch.float32) for s in featmap_strides]
    zero = sum(m[:0].sum() for m in maps)                                             # an exact 0 that keeps every level in the graph
    rows = []
    for k in range(K):
        l = lvls[k]
        m, s = maps[l], scales[l]
        h, w = m.shape[1], m.shape[2]
        bf, x0, y0, x1, y1 = r[k]
        sx, sy = x0 * s - 0.5, y0 * s - 0.5
        rw, rh = (x1 * s - 0.5) - sx, (y1 * s - 0.5) - sy
        bw, bh = rw / float(P), rh / float(P)
        ok = bool(bf >= 0) and bool(bf < B) and bool(rw.abs() <= 2.0 * w) and bool(rh.abs() <= 2.0 * h)
        gw = gh = 0
        if ok:
            gw = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(bw))
            gh = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(bh))
        if gw <= 0 or gh <= 0:
            rows.append(torch.zeros(P, P, C) + zero)
            continue
        count = float(max(gh * gw, 1))
        vy, ylo, yhi, hy, ly = _axis_torch(sy, bh, gh, P, h)
        vx, xlo, xhi, hx, lx = _axis_torch(sx, bw, gw, P, w)
        img = m[int(bf)]
        tap = lambda yi, xi: img[yi][:, xi]                                           # [P * gh, P * gw, C]
        val = ((hy[:, None] * hx[None, :])[..., None] * tap(ylo, xlo) + (hy[:, None] * lx[None, :])[..., None] * tap(ylo, xhi)
               + (ly[:, None] * hx[None, :])[..., None] * tap(yhi, xlo) + (ly[:, None] * lx[None, :])[..., None] * tap(yhi, xhi))
        val = torch.where((vy[:, None] & vx[None, :])[..., None], val, torch.zeros_like(val))
        rows.append(val.reshape(P, gh, P, gw, C).sum(dim=(1, 3)) / count + zero)
    out = torch.stack(rows) if rows else torch.zeros(0, P, P, C)
    return out.permute(0, 3, 1, 2).to(dev)


# ================================================================================================ the kernel route
def _rows(t):
    """A channel-last [N, C, H, W] tensor as its 2-D view [N * H * W, C]."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


class _RoIExtract(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ops, rois, P, sampling_ratio, scales, finest_scale, *feats):
        maps = [f.detach().float().contiguous(memory_format=torch.channels_last) for f in feats]
        B, C = maps[0].shape[0], maps[0].shape[1]
        grids = [(m.shape[2], m.shape[3]) for m in maps]
        rois = rois.detach().float().contiguous()
        K = rois.shape[0]
        out = torch.empty(K * P * P, C, dtype=torch.float32, device=rois.device)
        if K:
            ops.roi_extract_fwd([_rows(m) for m in maps], grids, scales, rois, out, B, P, sampling_ratio, finest_scale)
        ctx.ops, ctx.args = ops, (B, C, K, P, sampling_ratio, scales, finest_scale, grids, [f.dtype for f in feats])
        ctx.save_for_backward(rois)
        return out.view(K, P, P, C).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad):
        B, C, K, P, sampling_ratio, scales, finest_scale, grids, dtypes = ctx.args
        rois, = ctx.saved_tensors
        dmaps = [torch.zeros(B * h * w, C, dtype=torch.float32, device=grad.device) for h, w in grids]
        if K:
            g = grad.float().contiguous(memory_format=torch.channels_last)
            ctx.ops.roi_extract_bwd(_rows(g), rois, dmaps, grids, scales, B, P, sampling_ratio, finest_scale)
        grads = [d.view(B, h, w, C).permute(0, 3, 1, 2).to(dt) for d, (h, w), dt in zip(dmaps, grids, dtypes)]
        return (None,) * 6 + tuple(grads)


def roi_extract(feats, rois, output_size, sampling_ratio, featmap_strides, finest_scale=56, ops=None):
    """Route by tensor: the kernels on a backend with ROI_EXTRACT, roi_extract_torch otherwise.  -> [K, C, P, P] fp32."""
    k_ops = _kernel_ops(feats[0], ops)
    if k_ops is None:
        return roi_extract_torch(feats, rois, output_size, sampling_ratio, featmap_strides, finest_scale)
    scales = [1.0 / float(s) for s in featmap_strides]
    return _RoIExtract.apply(k_ops, rois, int(output_size), int(sampling_ratio), scales, float(finest_scale), *feats)


# ================================================================================================ mmdet's module
class SingleRoIExtractor(nn.Module):
    """mmdet 2.x `SingleRoIExtractor` with its constructor keywords, so that the reference's config dict builds it unchanged:
    dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
    featmap_strides=[4, 8, 16, 32]).  forward(feats, rois) -> [K, out_channels, P, P]."""

    def __init__(self, roi_layer=None, out_channels=256, featmap_strides=(4, 8, 16, 32), finest_scale=56, init_cfg=None, ops=None):
        super().__init__()
        cfg = dict(type="RoIAlign", output_size=7, sampling_ratio=0) if roi_layer is None else dict(roi_layer)
        kind = cfg.pop("type", "RoIAlign")
        if kind != "RoIAlign":
            raise ValueError(f"roi_layer type {kind!r}: only 'RoIAlign' is implemented")
        if cfg.pop("aligned", True) is not True:
            raise ValueError("roi_layer aligned=False (the half-pixel-shifted legacy form) is not implemented")
        mode = cfg.pop("pool_mode", "avg")
        if mode != "avg":
            raise ValueError(f"roi_layer pool_mode={mode!r}: only 'avg' is implemented")
        cfg.pop("use_torchvision", None)                              # accepted and ignored: both libraries compute the same algorithm
        size = cfg.pop("output_size", 7)
        if isinstance(size, (tuple, list)):
            if len(size) != 2 or size[0] != size[1]:
                raise ValueError(f"roi_layer output_size={size!r}: only square outputs are implemented")
            size = size[0]
        ratio = cfg.pop("sampling_ratio", 0)
        if cfg:
            raise ValueError(f"roi_layer options {sorted(cfg)} are not implemented")
        if not 1 <= int(size) <= KERNEL_MAX_OUTPUT:
            raise ValueError(f"roi_layer output_size={size} must be in [1, {KERNEL_MAX_OUTPUT}]")
        if not 0 <= int(ratio) <= KERNEL_MAX_SAMPLING:
            raise ValueError(f"roi_layer sampling_ratio={ratio} must be in [0, {KERNEL_MAX_SAMPLING}]")
        featmap_strides = list(featmap_strides)
        if not 1 <= len(featmap_strides) <= KERNEL_MAX_LEVELS:
            raise ValueError(f"featmap_strides has {len(featmap_strides)} levels: 1 to {KERNEL_MAX_LEVELS} levels are implemented")
        self.output_size, self.sampling_ratio = int(size), int(ratio)
        self.out_channels, self.featmap_strides, self.finest_scale = int(out_channels), featmap_strides, finest_scale
        self.ops = ops

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def map_roi_levels(self, rois, num_levels):
        return map_roi_levels_torch(rois, num_levels, self.finest_scale).to(rois.device)

    def forward(self, feats, rois, roi_scale_factor=None):
        if roi_scale_factor is not None:
            raise ValueError("roi_scale_factor is not implemented (no F-ViT config uses it)")
        feats = list(feats)[:self.num_inputs]
        if len(feats) != self.num_inputs:
            raise ValueError(f"{len(feats)} maps for {self.num_inputs} featmap_strides")
        for f in feats:
            if f.dim() != 4 or f.shape[1] != self.out_channels or f.shape[0] != feats[0].shape[0]:
                raise ValueError(f"a map of shape {tuple(f.shape)}: every level must be [B, out_channels = {self.out_channels}, h, w]")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError(f"rois must be [K, 5] = (image index, x0, y0, x1, y1), got {tuple(rois.shape)}")
        return roi_extract(feats, rois, self.output_size, self.sampling_ratio, self.featmap_strides, self.finest_scale, self.ops)
