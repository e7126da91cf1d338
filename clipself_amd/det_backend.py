"""What the detector modules (det_post, det_targets, det_losses, det_masks, det_proposals, roi_extractor) share on the way to the kernels:
the one lazily built HipOps, the rule that picks a backend for a tensor, and the two tensor conversions every wrapper needs."""
from __future__ import annotations

import torch

_ops = None


def hip_ops():
    """The process-wide HipOps of the detector modules (one set of workspace caches), built on first use."""
    global _ops
    if _ops is None:
        from .hip import HipOps
        _ops = HipOps()
    return _ops


def kernel_ops(t, flag, ops=None, fused=None, default=True):
    """The backend whose `flag` kernels (DET_POST, ASSIGN, LOSS, MASK, RPN, ROI_EXTRACT) serve tensor t, or None (-> the torch route).
    fused=False never takes the kernels, fused=True insists on them (NotImplementedError where they cannot run), fused=None takes them
    where the backend has them and `default` (the module's FUSED_*_DEFAULT) is true."""
    if fused is False:
        return None
    if not t.is_cuda:
        if fused:
            raise NotImplementedError("fused=True needs CUDA tensors: the kernels have no CPU form")
        return None
    if ops is None:
        ops = hip_ops()
    if not getattr(ops, flag, False):
        if fused:
            raise NotImplementedError(f"fused=True: backend {getattr(ops, 'name', ops)!r} has no {flag} kernels")
        return None
    return ops if fused or default else None


def as_i32(t, device):
    """A table of row offsets or labels (tensor, host list or None) as a contiguous int32 tensor on `device`."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.int32).contiguous()
    return torch.tensor([int(v) for v in t], dtype=torch.int32, device=device)


def f32c(t):
    """t as contiguous fp32 (mmdet's force_fp32); differentiable, so a caller that wants no graph detaches first."""
    t = t.float()
    return t if t.is_contiguous() else t.contiguous()
