"""The detector's feature pyramid: 1 x 1 laterals, the top-down path and 3 x 3 output convolutions on channel-last maps.

mmdet 2.28's FPN (mmdet/models/necks/fpn.py) as every F-ViT config builds it,
`neck=dict(type='FPN', in_channels=[w]*4, out_channels=256, num_outs=5, norm_cfg=dict(type='SyncBN', requires_grad=True))`, called as
`self.neck(self.backbone(img)[:-1])` (F-ViT/models/fvit.py:14-16, 43-45):

  laterals[i] = lateral_convs[i](inputs[i])                              ConvModule(in_i, out, 1, norm_cfg, act_cfg=None)
  laterals[i - 1] += F.interpolate(laterals[i], mode='nearest')          from the coarsest level down
  outs[i]     = fpn_convs[i](laterals[i])                                ConvModule(out, out, 3, padding=1, norm_cfg, act_cfg=None)
  outs[k]     = F.max_pool2d(outs[k - 1], 1, stride=2)                   the extra levels, k >= len(in_channels)

The laterals are GEMMs on channel-last rows (conv.Conv1x1), the output convolutions conv.Conv3x3, the norms norm_act.BatchNormAct2d.  The
top-down step has a kernel of its own: HipOps.upsample2x_add adds the upsampled coarser level into a copy of the lateral's map in
one pass (a read of the coarse map, a read and a write of the fine one), and its backward is HipOps.pool2x, the sum of each 2 x 2 block
of the gradient, while the gradient itself passes through to the lateral.  No atomics: equal inputs give equal bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .det_layer import BF16, F32, channel_last_rows, kernel_grad, layer_ops, rows_to_map, uncovered
from .norm_act import NORMS, ConvModule, apply_norm_cfg  # noqa: F401  (NORMS stays importable from here)

# Whether fused=None takes the top-down kernels where the backend has them: set from profiles/fpn_bench.md by the rule of
# conv.FUSED_CONV_DEFAULT -- on only if the kernel route wins forward + backward against the faster torch variant at every measured shape.
# It does not.  Whole module, forward + backward, B = 8 (all kernels / torch under bf16 autocast on channels-last inputs, the faster torch
# variant / torch fp32, the form the detector runs): 5.51 / 5.03 / 13.23 ms at B/16 640^2, 12.00 / 11.19 / 32.36 ms at B/16 1024^2,
# 13.61 / 12.22 / 35.06 ms at L/14-336 896^2 -- 2.4 - 2.7 x against fp32, 0.90 - 0.93 x against autocast, whose intermediate maps are bf16
# where this route keeps its fp32 input's type.  The top-down path alone wins at all three (1.28 / 1.22 / 1.19 x; forms 7 / 8 stream at
# 84 - 106 % of 6.3 TB/s) and the all-kernel module is 4 - 5 % faster than the same module with torch's top-down step, but at the 64 <- 32
# level pair the copy + two launches lose to torch (79 against 68 us): not a win at every shape, so the flag stays off.
FUSED_FPN_DEFAULT = False


def _topdown_covered(fine, coarse) -> bool:
    """What upsample2x_add / pool2x cover: two 4-D fp32 / bf16 maps of equal batch and channels on one device, the fine one exactly twice
    the coarse one's size."""
    return (fine.dim() == 4 and coarse.dim() == 4 and fine.dtype in (F32, BF16) and coarse.dtype in (F32, BF16) and fine.device == coarse.device
            and fine.shape[:2] == coarse.shape[:2] and fine.shape[2] == 2 * coarse.shape[2] and fine.shape[3] == 2 * coarse.shape[3]
            and coarse.numel() > 0)


class TopDownFn(torch.autograd.Function):
    """fine + nearest_up2(coarse) on the kernels.  forward: form 7 accumulates into one channel-last copy of `fine`.  The laterals' maps are
    views that _BatchNormActFn / _Conv1x1Fn create inside a custom Function, and autograd refuses an in-place write (mark_dirty) on such a
    view -- it could not rebase their backward -- so the copy it asks for is taken here; its cost is part of every figure in
    profiles/fpn_bench.md.  backward: the gradient passes through to `fine`; `coarse` gets pool2x of it (form 8, overwrite)."""

    @staticmethod
    def forward(ctx, fine, coarse, ops):
        B, C, h, w = coarse.shape
        out = ops.empty((B, 2 * h, 2 * w, C), fine.dtype)
        out.copy_(fine.permute(0, 2, 3, 1))                            # channel-last whatever fine's strides were
        ops.upsample2x_add(channel_last_rows(coarse), out.view(4 * B * h * w, C), B, h, w, C, accumulate=True)
        ctx.ops, ctx.geom, ctx.coarse_dtype = ops, (B, h, w, C), coarse.dtype
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        ops = ctx.ops
        B, h, w, C = ctx.geom
        d_coarse = None
        if ctx.needs_input_grad[1]:
            g = kernel_grad(g)
            dC = ops.empty((B * h * w, C), ctx.coarse_dtype)
            ops.pool2x(channel_last_rows(g), dC, B, h, w, C, accumulate=False)
            d_coarse = rows_to_map(dC, B, h, w)
        return (g if ctx.needs_input_grad[0] else None), d_coarse, None


class FPN(nn.Module):
    """mmdet 2.28's FPN with the options of the F-ViT configs; the reference's config dict (minus `type`) constructs it unchanged, and a
    reference state dict -- lateral_convs.{i}.conv.weight, lateral_convs.{i}.bn.{weight, bias, running_mean, running_var,
    num_batches_tracked}, fpn_convs.{i}. ...; with norm_cfg=None .conv.bias and no bn -- loads with strict=True.

    Options other than the defaults start_level=0, end_level=-1, add_extra_convs=False, no_norm_on_lateral=False, act_cfg=None,
    upsample_cfg=dict(mode='nearest') raise NotImplementedError naming the option.  Initialisation is mmdet's
    init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform'): Xavier-uniform convolution weights, zero biases.

    ops / fused reach every layer: fused=True = the kernels or NotImplementedError (also for a level that is not exactly twice the next
    one), False = torch throughout, None = each layer's FUSED_*_DEFAULT and FUSED_FPN_DEFAULT for the top-down step.
    forward(inputs): a tuple of len(in_channels) maps [B, in_i, H_i, W_i] -> a tuple of num_outs maps [B, out_channels, ., .], each of its
    input's dtype (the extra levels of the last output's)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False, relu_before_extra_convs=False,
                 no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode="nearest"), init_cfg=None,
                 ops=None, fused=None):
        super().__init__()
        assert isinstance(in_channels, (list, tuple)) and len(in_channels) >= 1
        options = dict(start_level=(start_level, 0), end_level=(end_level, -1), add_extra_convs=(add_extra_convs, False),
                       relu_before_extra_convs=(relu_before_extra_convs, False), no_norm_on_lateral=(no_norm_on_lateral, False),
                       conv_cfg=(conv_cfg, None), act_cfg=(act_cfg, None), upsample_cfg=(dict(upsample_cfg), dict(mode="nearest")))
        for name, (got, only) in options.items():
            if got != only:
                raise NotImplementedError(f"FPN: {name}={got!r} is not built here (only {name}={only!r}, what the F-ViT configs use)")
        assert num_outs >= len(in_channels), "num_outs counts the extra levels on top of the len(in_channels) pyramid levels"
        self.in_channels = list(in_channels)
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.ops = ops
        self.fused = fused
        norm = norm_cfg is not None
        self.lateral_convs = nn.ModuleList(ConvModule(c, out_channels, norm, None, ops=ops, fused=fused, kernel_size=1) for c in in_channels)
        self.fpn_convs = nn.ModuleList(ConvModule(out_channels, out_channels, norm, None, ops=ops, fused=fused, kernel_size=3) for _ in in_channels)
        for m in self.modules():                                       # mmdet's init_cfg (cited, not run): mmcv xavier_init, bias 0
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        apply_norm_cfg(self, norm_cfg)

    # ------------------------------------------------------------------------------------------ the top-down step
    def _topdown_backend(self, fine, coarse):
        """The backend whose FPN_TOPDOWN kernels add `coarse` into `fine`, or None (-> torch); NotImplementedError where fused=True cannot be met."""
        k = layer_ops(fine, "FPN_TOPDOWN", self.ops, self.fused, FUSED_FPN_DEFAULT)
        if k is not None and not _topdown_covered(fine, coarse):
            return uncovered(self.fused, f"the top-down step from {tuple(coarse.shape)} {coarse.dtype} to {tuple(fine.shape)} {fine.dtype}",
                             "a level exactly twice the next one, fp32 / bf16 maps")
        return k

    def _merge(self, fine, coarse):
        """fine + nearest_up(coarse): mmdet's laterals[i - 1] + F.interpolate(laterals[i], size=prev_shape, mode='nearest')."""
        k = self._topdown_backend(fine, coarse)
        if k is None:
            return fine + F.interpolate(coarse, size=fine.shape[2:], mode="nearest")
        return TopDownFn.apply(fine, coarse, k)

    def forward(self, inputs):
        assert len(inputs) == self.num_ins, f"FPN takes {self.num_ins} maps, got {len(inputs)}"
        merged = [conv(x) for conv, x in zip(self.lateral_convs, inputs)]
        for i in range(self.num_ins - 1, 0, -1):
            merged[i - 1] = self._merge(merged[i - 1], merged[i])
        outs = [conv(x) for conv, x in zip(self.fpn_convs, merged)]
        for _ in range(self.num_outs - self.num_ins):                  # the subsample [..., ::2, ::2]: tiny, torch's
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return tuple(outs)
