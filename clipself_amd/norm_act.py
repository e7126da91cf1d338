"""Batch norm with a fused ReLU on channel-last maps, and the detector's ConvModule (include/clipself_bn.h).

Every convolution of the F-ViT detector sits in an mmcv ConvModule (mmcv/cnn/bricks/conv_module.py: conv -> norm -> act, the submodules
named `conv`, `bn` (build_norm_layer's abbreviation of BN / SyncBN / MMSyncBN) and `activate`) with norm_cfg=dict(type='SyncBN') and a
ReLU.  BatchNormAct2d is nn.BatchNorm2d -- parameters, buffers, names, state dict -- whose training-mode forward is three passes over
the map held as rows [N*H*W, C]:

  bn_stats      this rank's record (mean, M2, count), one read of the map;
  bn_finalize   the records of all ranks merged by count (torch.nn.SyncBatchNorm's merge), scale = gamma * rstd and
                shift = beta - mean * scale computed once, the running statistics updated;
  bn_apply      y = relu(fmaf(x, scale, shift)), one read and one write;

and whose backward is two: bn_bwd_reduce (sum g, sum g * xhat: dbeta and dgamma, with the ReLU mask recomputed from x and the stored scale
and shift) and bn_bwd_apply.  Only x and the state are kept for the backward.  No atomics: equal inputs give equal bits.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from .conv import Conv1x1, Conv3x3
from .det_layer import BF16, F32, KernelLayer, channel_last_rows, kernel_grad, rows_to_map

NORMS = ("BN", "SyncBN", "MMSyncBN")          # what build_norm_layer abbreviates to `bn`: all of them are BatchNormAct2d here
REC_EXTRA, ST_EXTRA = 4, 4          # include/clipself_bn.h: a record is 2*C + 4 floats, a state 4*C + 4
ACTS = {None: 0, "relu": 1}

# Whether fused=None takes the kernels where the backend has them: set from profiles/batchnorm_bench.md by the rule of FUSED_CONV_DEFAULT --
# on only if the kernel route wins forward + backward against the faster torch variant (F.relu out of place or in place, same input) at
# every measured shape.  It does: 11.5 x / 10.5 x at the box head's 200 704 x 256 (fp32 / bf16 maps; torch's channel-last batch norm is
# slow at N = 4096), 1.45 x / 1.68 x at rpn640, 1.61 x / 1.79 x at rpn1024, 1.50 x at the neck's 131 072 x 768 in fp32.  The bf16 margins
# rest on the host keeping up: the five launches need ~160 us of Python per layer and step, the kernels 165 us at rpn640; an earlier run
# with 30 us more host work per call tied torch there (286 against 283 us).
FUSED_BN_DEFAULT = True


class BatchNormAct2d(KernelLayer, nn.BatchNorm2d):
    """nn.BatchNorm2d (training semantics of nn.SyncBatchNorm when torch.distributed runs with more than one rank) followed by `act`
    (None or "relu"), on the HIP kernels when the tensors live on a backend with BATCHNORM and the case is covered: C % 8 == 0, a momentum
    that is a number, an fp32 / bf16 input, fp32 parameters and buffers.  F.batch_norm (+ F.relu) otherwise.

    fused: True = the kernels or NotImplementedError, False = torch, None = FUSED_BN_DEFAULT where the kernels can run.
    forward(x): x [N, C, H, W] -> [N, C, H, W] of x's dtype with channel-last strides (kernel route).  A channel-last x is used in place,
    anything else is made channel-last once by torch."""
    FLAG = "BATCHNORM"
    COVERAGE = "C % 8 == 0, a numeric momentum, fp32 / bf16 input, fp32 parameters and buffers"

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act=None, process_group=None, ops=None,
                 fused=None, **kw):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats, **kw)
        assert act in ACTS, f"act is None or 'relu', got {act!r}"
        self.act = act
        self.process_group = process_group
        self.ops = ops
        self.fused = fused

    def extra_repr(self):
        return super().extra_repr() + f", act={self.act}"

    # ------------------------------------------------------------------------------------------ dispatch
    def covered(self, x) -> bool:
        tensors = [t for t in (self.weight, self.bias, self.running_mean, self.running_var) if t is not None]
        return (self.num_features % 8 == 0 and self.momentum is not None and x.dim() == 4 and x.dtype in (F32, BF16)
                and x.shape[1] == self.num_features and x.numel() > 0 and all(t.dtype == F32 and t.device == x.device for t in tensors))

    def describe(self):
        return f"BatchNormAct2d({self.num_features}, momentum={self.momentum})"

    def fused_default(self):
        return FUSED_BN_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            y = super().forward(x)
            return F.relu(y) if self.act == "relu" else y
        batch_stats = self.training or (self.running_mean is None and self.running_var is None)
        if batch_stats and x.numel() // x.shape[1] == 1 and self._world() == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            with torch.no_grad():
                self.num_batches_tracked.add_(1)                      # on the device: nothing is read back
        return _BatchNormActFn.apply(x, self.weight, self.bias, self, k, batch_stats)

    # ------------------------------------------------------------------------------------------ the collective
    def _world(self) -> int:
        """Ranks whose statistics are merged: the process group's size in training mode, 1 otherwise (as nn.SyncBatchNorm)."""
        if self.training and dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.process_group)
        return 1

    def _syncs(self) -> bool:
        """Whether _reduce_sums may change its argument: more than one rank, or a subclass that stands in for ranks."""
        return self._world() > 1 or type(self)._reduce_sums is not BatchNormAct2d._reduce_sums

    def _gather_records(self, rec):
        """This rank's record [2*C + 4] -> the records of all ranks [R, 2*C + 4] in rank order (one all_gather; a copy of bits)."""
        world = self._world()
        if world == 1:
            return rec.view(1, -1)
        out = rec.new_empty((world, rec.numel()))
        dist.all_gather_into_tensor(out, rec, group=self.process_group)
        return out

    def _reduce_sums(self, sums):
        """This rank's sum g | sum g * xhat [2*C] -> their sums over all ranks (one all_reduce, in place)."""
        if self._world() > 1:
            dist.all_reduce(sums, group=self.process_group)
        return sums


_rows = channel_last_rows                      # the name it had here, for callers written before it moved to det_layer


class _BatchNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops, batch_stats):
        N, C, H, W = x.shape
        M = N * H * W
        act = ACTS[mod.act]
        X = channel_last_rows(x)
        gamma = None if weight is None else weight.detach()
        beta = None if bias is None else bias.detach()
        block = ops.empty((6 * C + ST_EXTRA + REC_EXTRA,), F32)          # the state and this rank's record: one allocation
        st = block[:4 * C + ST_EXTRA]
        if batch_stats:
            rec = block[4 * C + ST_EXTRA:]
            ops.bn_stats(X, rec)
            recs = mod._gather_records(rec)
            track = mod.training and mod.track_running_stats
            ops.bn_finalize(recs, C, gamma, beta, mod.eps, mod.momentum, mod.running_mean if track else None,
                            mod.running_var if track else None, st)
        else:
            ops.bn_finalize(None, C, gamma, beta, mod.eps, 0.0, mod.running_mean, mod.running_var, st)
        Y = ops.empty((M, C), x.dtype)
        ops.bn_apply(X, st, act, Y)
        ctx.mod, ctx.ops, ctx.act, ctx.geom, ctx.batch_stats = mod, ops, act, (N, H, W, C), batch_stats
        ctx.affine = (weight is not None, bias is not None)
        ctx.save_for_backward(X, st, gamma)
        return rows_to_map(Y, N, H, W)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops, act = ctx.mod, ctx.ops, ctx.act
        N, H, W, C = ctx.geom
        X, st, gamma = ctx.saved_tensors
        dY = channel_last_rows(kernel_grad(d_out))
        sums = ops.empty((2 * C,), F32)
        ops.bn_bwd_reduce(dY, X, st, act, sums)
        reduce = ctx.needs_input_grad[0] and ctx.batch_stats and mod._syncs()
        own = sums.clone() if reduce else sums                           # this rank's own sums, copied out before the all-reduce
        dgamma = own[C:] if ctx.affine[0] and ctx.needs_input_grad[1] else None
        dbeta = own[:C] if ctx.affine[1] and ctx.needs_input_grad[2] else None
        dx = None
        if ctx.needs_input_grad[0]:
            if reduce:
                sums = mod._reduce_sums(sums)
            dX = ops.empty((N * H * W, C), X.dtype)
            ops.bn_bwd_apply(dY, X, st, act, sums, gamma, dX)
            dx = rows_to_map(dX, N, H, W)
        return dx, dgamma, dbeta, None, None, None


def apply_norm_cfg(owner, norm_cfg):
    """What a head does with its config's norm_cfg once its layers stand: a type outside NORMS is refused in the owner's name, and
    requires_grad=False freezes every batch norm's parameters (build_norm_layer: param.requires_grad = requires_grad)."""
    if norm_cfg is None:
        return
    if norm_cfg.get("type") not in NORMS:
        raise NotImplementedError(f"{type(owner).__name__}: norm_cfg={norm_cfg!r} is not built here (type one of {NORMS}, or norm_cfg=None)")
    if not norm_cfg.get("requires_grad", True):
        for m in owner.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.requires_grad_(False)


class ConvModule(nn.Module):
    """The F-ViT form of mmcv's ConvModule(in_channels, out_channels, 3, padding=1, norm_cfg=dict(type='SyncBN'), act_cfg=dict(type='ReLU')):
    `conv` (Conv3x3; bias=False when a norm follows, mmcv's bias='auto') then `bn` (BatchNormAct2d carrying the activation), the order and
    the names of mmcv/cnn/bricks/conv_module.py, so a reference checkpoint's ....conv.weight, ....bn.weight, ....bn.bias,
    ....bn.running_mean, ....bn.running_var and ....bn.num_batches_tracked load with strict=True.  kernel_size=1 builds the same module
    around Conv1x1 (padding 0): with act=None, the lateral convolutions of fpn.FPN."""

    def __init__(self, in_channels, out_channels, norm=True, act="relu", ops=None, fused=None, kernel_size=3):
        super().__init__()
        assert act in ACTS, f"act is None or 'relu', got {act!r}"
        assert kernel_size in (1, 3), f"kernel_size is 1 or 3, got {kernel_size!r}"
        self.act = act
        conv = Conv3x3 if kernel_size == 3 else Conv1x1               # kernel_size=1, act=None: the FPN's laterals (mmcv's act_cfg=None)
        self.conv = conv(in_channels, out_channels, bias=not norm, ops=ops, fused=fused)
        self.bn = BatchNormAct2d(out_channels, act=act, ops=ops, fused=fused) if norm else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            return self.bn(x)
        return F.relu(x) if self.act == "relu" else x
