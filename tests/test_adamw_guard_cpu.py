"""CPU side of the guarded AdamW step (gradient norm, clipping and the non-finite-step skip inside cs_adamw_step): the fp64 reference the
GPU tests use is itself held against torch, the new flag parses, and a backend without the feature (RefOps) keeps the torch clipping
path bit for bit and refuses to skip."""
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from _adamw_guard_ref import clip_coef, grad_norm, guarded_step
from clipself_amd.config import tiny_cfg
from clipself_amd.init import seeded_visual_state, synthetic_batch
from clipself_amd.open_clip.model import CustomCLIP
from clipself_amd.training.clipself import CLIPSelf
from clipself_amd.training.optim import FlatAdamW
from clipself_amd.training.precision import get_autocast
from clipself_amd.training.train import train_step
from oracle.ops_ref import RefOps

ROOT = Path(__file__).resolve().parent.parent


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_reference_equals_clip_grad_norm_and_torch_adamw():
    """Five tensors laid out like the flat store (64-element granules, two of them with weight decay, inactive granules holding NaN
    gradients in between) == clip_grad_norm_ + torch.optim.AdamW on those tensors, 3 steps, the bound of test_adamw_matches_torch.  The
    gradient scale changes per step so that the clip bites on steps 1 and 2 and not on step 3."""
    gen = torch.Generator().manual_seed(5)
    sizes, decay = [64, 192, 128, 64, 320], [False, True, False, False, True]
    gaps = [64, 0, 64, 64, 0, 64]                                    # inactive granules before / between / after the tensors
    n = sum(sizes) + sum(gaps)
    assert n % 256 == 0
    flags, spans, o = torch.zeros(n // 64, dtype=torch.uint8), [], 0
    for gap, size, dec in zip(gaps, sizes, decay):
        o += gap
        flags[o // 64:(o + size) // 64] = 1 | (2 if dec else 0)
        spans.append((o, o + size))
        o += size
    p = torch.randn(n, generator=gen, dtype=torch.float64) * 0.02
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    params = [torch.nn.Parameter(p[a:b].clone()) for a, b in spans]
    lr, wd, max_norm = 1e-3, 0.1, 1.0
    opt = torch.optim.AdamW([dict(params=[q for q, d in zip(params, decay) if not d], weight_decay=0.0),
                             dict(params=[q for q, d in zip(params, decay) if d], weight_decay=wd)], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    coefs = []
    for step, scale in enumerate((1.0, 0.3, 0.01), start=1):
        g = torch.full((n,), float("nan"), dtype=torch.float64)
        for (a, b), q in zip(spans, params):
            g[a:b] = torch.randn(b - a, generator=gen, dtype=torch.float64) * scale
            q.grad = g[a:b].clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        out = guarded_step(p, g, m, v, flags, lr, 0.9, 0.999, 1e-8, wd, step, max_norm=max_norm)
        assert out["applied"] and abs(out["norm"] - float(total)) <= 1e-12 * float(total)
        coefs.append(out["coef"])
        p, m, v = out["p"], out["m"], out["v"]
        for (a, b), q in zip(spans, params):
            assert rel(p[a:b], q) < 1e-6, (step, a)
            assert rel(m[a:b], opt.state[q]["exp_avg"]) < 1e-6 and rel(v[a:b], opt.state[q]["exp_avg_sq"]) < 1e-6, (step, a)
    assert coefs[0] < 0.1 and coefs[1] < 0.5 and coefs[2] == 1.0, coefs
    act = (flags & 1).bool().repeat_interleave(64)
    assert torch.isfinite(p).all() and bool((m[~act] == 0).all())     # the NaN gradients of inactive granules never entered


def test_reference_skip_and_scale_rules():
    n = 256
    flags = torch.tensor([1, 3, 0, 1], dtype=torch.uint8)
    g = torch.ones(n)
    p, m, v = torch.ones(n), torch.zeros(n), torch.zeros(n)
    assert grad_norm(g, flags, 0.5) == pytest.approx(0.5 * (192 ** 0.5), rel=1e-12)
    assert clip_coef(10.0, 0.0) == 1.0 and clip_coef(10.0, None) == 1.0 and clip_coef(0.5, 1.0) == 1.0
    assert clip_coef(10.0, 1.0) == pytest.approx(1.0 / (10.0 + 1e-6), rel=1e-15)
    g[70] = float("inf")
    out = guarded_step(p, g, m, v, flags, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, skip_nonfinite=True)
    assert not out["applied"] and torch.equal(out["p"], p.double()) and torch.equal(out["m"], m.double())
    g[70], g[130] = 1.0, float("nan")                                  # granule 2 is inactive
    out = guarded_step(p, g, m, v, flags, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, skip_nonfinite=True)
    assert out["applied"] and torch.isfinite(out["p"]).all() and torch.equal(out["p"][128:192], p[128:192].double())


def test_constants_and_capability_attribute():
    """The header's macros and hip.py agree, and adamw.hip takes them from the header (it keeps no number of its own); HipOps announces
    the feature, RefOps (no such attribute) does not."""
    from clipself_amd import hip
    header = (ROOT / "include" / "clipself_hip.h").read_text()
    head = int(re.search(r"^#define CS_ADAMW_GUARD_HEAD (\d+)$", header, re.M).group(1))
    span = int(re.search(r"^#define CS_ADAMW_GUARD_SPAN (\d+)$", header, re.M).group(1))
    src = (ROOT / "clipself_amd" / "csrc" / "adamw.hip").read_text()
    assert '#include "../../include/clipself_hip.h"' in src and "CS_ADAMW_GUARD_HEAD" in src and "CS_ADAMW_GUARD_SPAN" in src
    assert not re.search(r"GUARD_(HEAD|SPAN) = \d", src)
    assert head == hip.ADAMW_GUARD_HEAD and span == hip.ADAMW_GUARD_SPAN
    assert span % 256 == 0
    assert hip.HipOps.ADAMW_GUARD is True and not hasattr(RefOps, "ADAMW_GUARD")
    numel = hip.HipOps.adamw_guard_numel
    assert [numel(n) for n in (256, span, span + 256, 3 * span - 256)] == [head + 1, head + 1, head + 2, head + 3]
    assert len(hip.SIGNATURES["cs_adamw_step"][1]) == 18


def test_flag_parsing():
    from clipself_amd.training.params import parse_args
    assert parse_args([]).skip_nonfinite_steps is False
    assert parse_args(["--skip-nonfinite-steps"]).skip_nonfinite_steps is True


def _args(**kw):
    base = dict(device="cpu", precision="amp", distributed=False, skip_scheduler=True, grad_clip_norm=None, multiscale=False,
                extract_type="v2", cosine_weight=1.0)
    base.update(kw)
    return SimpleNamespace(**base)


def _pair(cfg):
    student, teacher = CustomCLIP(cfg, ops=RefOps(), trainable=True), CustomCLIP(cfg, ops=RefOps(), trainable=False)
    for mdl in (student, teacher):
        mdl.visual.engine.load_state(seeded_visual_state(cfg, 1))
    student.lock_image_tower(unlocked_groups=cfg.layers)
    student.train()
    teacher.eval()
    return student, teacher


def test_backend_without_the_guard_keeps_the_torch_clipping_path_bit_for_bit():
    """RefOps has no ADAMW_GUARD: train_step(--grad-clip-norm) must still be clip_grad_norm_ on the parameter views followed by the plain
    optimizer step -- the same bits as those two calls made by hand on an identical model."""
    cfg, clip = tiny_cfg(), 0.05
    batch = synthetic_batch(2, 3, cfg.image_size, cfg.image_size, seed=40)
    a, teacher = _pair(cfg)
    opt_a = FlatAdamW(a, lr=1e-3, weight_decay=0.1)
    assert not opt_a.guard_available()
    train_step(a, CLIPSelf(), batch, opt_a, None, 0, teacher, _args(grad_clip_norm=clip))
    b, _ = _pair(cfg)
    opt_b = FlatAdamW(b, lr=1e-3, weight_decay=0.1)
    opt_b.zero_grad()
    args = _args()
    with get_autocast(args.precision)():
        losses, _, _ = CLIPSelf()(batch, b, teacher, None, torch.device("cpu"), None, False, args)
    sum(losses.values()).backward()
    before = float(b.visual.engine.grad.norm())
    torch.nn.utils.clip_grad_norm_([p for p in b.parameters() if p.grad is not None], clip, norm_type=2.0)
    opt_b.step()
    ea, eb = a.visual.engine, b.visual.engine
    assert before > 2 * clip and float(eb.grad.norm()) <= clip * 1.001, "the clip threshold must actually bite in this scenario"
    for name in ("grad", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name
    assert torch.equal(ea.shadow.view(torch.int16), eb.shadow.view(torch.int16))
    assert ea.guard is None and opt_a.grad_stats() is None
    # the optimizer's own max_norm falls back to the same torch call on such a backend
    c, _ = _pair(cfg)
    opt_c = FlatAdamW(c, lr=1e-3, weight_decay=0.1)
    opt_c.zero_grad()
    with get_autocast(args.precision)():
        losses, _, _ = CLIPSelf()(batch, c, teacher, None, torch.device("cpu"), None, False, args)
    sum(losses.values()).backward()
    opt_c.step(max_norm=clip)
    assert torch.equal(c.visual.engine.master, eb.master) and torch.equal(c.visual.engine.grad, eb.grad)


def test_skip_nonfinite_raises_on_a_backend_without_the_guard():
    cfg = tiny_cfg()
    student, teacher = _pair(cfg)
    opt = FlatAdamW(student, lr=1e-3, weight_decay=0.1)
    with pytest.raises(NotImplementedError, match="ref"):
        opt.step(skip_nonfinite=True)
    assert opt.step_count == 0
    with pytest.raises(NotImplementedError, match="ref"):
        student.visual.engine.adamw_step(1, 1e-3, 0.1, skip_nonfinite=True)
    batch = synthetic_batch(2, 3, cfg.image_size, cfg.image_size, seed=40)
    with pytest.raises(NotImplementedError):
        train_step(student, CLIPSelf(), batch, opt, None, 0, teacher, _args(skip_nonfinite_steps=True))
