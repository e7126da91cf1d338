"""fp64 restatement of one guarded cs_adamw_step (include/clipself_hip.h) in plain torch: flat p / g / m / v, one flag byte per 64 elements
(bit0 = the granule has a gradient, bit1 = weight decay applies), gradient norm over the active granules, clip coefficient with
clip_grad_norm_'s arithmetic, the non-finite-step skip, decoupled weight decay.  tests/test_adamw_guard_cpu.py holds it against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW; tests/test_gpu_adamw_guard.py holds the kernels against it."""
import math

import torch

GRANULE = 64


def granule_mask(flags, bit):
    return (flags.cpu() & bit).bool().repeat_interleave(GRANULE)


def grad_norm(g, flags, grad_scale=1.0):
    """L2 norm of grad_scale * g over the active granules, fp64; what inactive granules hold does not enter."""
    act = granule_mask(flags, 1)
    gs = g.detach().cpu().double()[act] * float(torch.tensor(grad_scale, dtype=torch.float32))
    return float(gs.square().sum().sqrt())


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0 (clipping off)."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def guarded_step(p, g, m, v, flags, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """-> dict(p, m, v: new fp64 tensors; norm, coef: floats; applied: bool).  The inputs are left alone."""
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    act, dec = granule_mask(flags, 1), granule_mask(flags, 2)
    norm = grad_norm(g, flags, grad_scale)
    coef = clip_coef(norm, max_norm)
    if skip_nonfinite and not math.isfinite(norm):
        return dict(p=p, m=m, v=v, norm=norm, coef=coef, applied=False)
    gg = torch.where(act, g, torch.zeros_like(g)) * (float(torch.tensor(grad_scale, dtype=torch.float32)) * coef)
    bc1 = 1.0 - beta1 ** step
    bc2s = math.sqrt(1.0 - beta2 ** step)
    pn = torch.where(dec, p * (1.0 - lr * wd), p)
    mn = beta1 * m + (1 - beta1) * gg
    vn = beta2 * v + (1 - beta2) * gg * gg
    pn = pn - (lr / bc1) * (mn / (vn.sqrt() / bc2s + eps))
    return dict(p=torch.where(act, pn, p), m=torch.where(act, mn, m), v=torch.where(act, vn, v), norm=norm, coef=coef, applied=True)
