"""TEST INFRASTRUCTURE -- golden vectors of the reference's training step through mask-attention pooling (extract_type='v1',
open_clip/transformer.py:659-671,736-834).  Runs only where the reference checkout exists:   python tools/gen_golden_maskattn_grad.py

Drives the real reference like oracle/gen_golden.py::_run_steps (its CLIPSelf.__call__, AdamW groups, cosine schedule) with
args.extract_type = "v1" on the tiny OpenAI-CLIP ViT and writes tests/golden/tiny_openai_maskattn_grad*.npz (several files, each below 1 MiB):

  student seed 3, TEACHER seed 4.  With shared weights the passenger of a box is nearly the crop's CLS feature (first loss 0.002) and bf16
      feature noise is several percent of the gradient; a different teacher gives an O(1) loss.  Asserted: first loss >= 0.5.
  batches synthetic_batch(2, 3, size, 32, seed=41 + step) with box [1, 2] invalidated: 3 + 2 valid boxes, i.e. a padding passenger and the
      reference's boolean-indexed (non-dense) rois path.
  recipes blocks/ (lock L), stem/ (L + 2), stem64/ (L + 2 on a 64-px image: rescaled grid, N = 65), all/ (no lock), 3 steps each, GELU;
      q/blocks/ one QuickGELU step.
  stored  losses, lrs, the grad-None list, first-step gradients (every tensor for all/, a handful otherwise), final non-block weights.
"""
from __future__ import annotations

import json
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from clipself_amd.config import tiny_openai_cfg                   # noqa: E402
from clipself_amd.init import synthetic_batch                     # noqa: E402
from oracle.gen_golden import TINY, _build_openai, _optimizer     # noqa: E402
from oracle.ref_import import import_reference                    # noqa: E402

STUDENT_SEED, TEACHER_SEED, SEED_B = 3, 4, 41
# block tensors whose first-step gradient is kept for the recipes other than all/ (which keeps every tensor): the last block's in_proj
# (its q and k rows are non-zero on this path) where the file size allows, block 0's, and a few vectors
SOME = {"blocks/": ("resblocks.0.ln_1.weight", "resblocks.0.ln_2.weight", "resblocks.0.attn.in_proj_weight", "resblocks.1.attn.in_proj_weight",
                    "resblocks.1.attn.in_proj_bias", "resblocks.0.mlp.c_proj.bias"),
        "q/blocks/": ("resblocks.0.ln_1.weight", "resblocks.1.attn.in_proj_weight", "resblocks.1.attn.in_proj_bias"),
        "stem/": ("resblocks.0.ln_1.weight", "resblocks.0.ln_2.weight", "resblocks.0.attn.in_proj_weight", "resblocks.1.attn.in_proj_bias"),
        "stem64/": ("resblocks.0.ln_1.weight", "resblocks.0.ln_2.weight", "resblocks.0.attn.in_proj_weight", "resblocks.1.attn.in_proj_bias")}
# no committed file above 1 MiB: the vectors are spread over tiny_openai_maskattn_grad{,_stem,_all,_all_b0,_all_b1}.npz, which the tests merge
FILES = {"blocks/": "", "q/blocks/": "", "stem/": "_stem", "stem64/": "_stem", "all/": "_all"}


def batch_for(step, size, crop):
    images, boxes, crops = synthetic_batch(2, 3, size, crop, seed=SEED_B + step)
    boxes[1, 2, -1] = 0                                           # 3 + 2 valid boxes
    return images, boxes, crops


def run(oc, cfg, unlocked, steps, size):
    from training.clipself import CLIPSelf
    from training.scheduler import cosine_lr
    student, teacher = _build_openai(oc, cfg, STUDENT_SEED), _build_openai(oc, cfg, TEACHER_SEED)
    if unlocked is not None:
        student.lock_image_tower(unlocked_groups=unlocked)
    student.train()
    teacher.eval()
    opt, groups = _optimizer(student, TINY["lr"], TINY["wd"])
    sched = cosine_lr(opt, TINY["lr"], TINY["warmup"], TINY["total"])
    method = CLIPSelf()
    args = SimpleNamespace(multiscale=False, extract_type="v1", cosine_weight=1.0)
    losses, lrs, grads = [], [], None
    for step in range(steps):
        batch = batch_for(step, size, cfg.image_size)
        lrs.append(sched(step))
        opt.zero_grad()
        out, _, _ = method(batch, student, teacher, None, "cpu", None, False, args)
        total = sum(out.values())
        total.backward()
        if step == 0:
            grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in student.named_parameters() if p.requires_grad}
        opt.step()
        with torch.no_grad():
            student.logit_scale.clamp_(0, math.log(100))
        losses.append(float(total.detach()))
    return student, losses, lrs, grads, groups


def main():
    oc = import_reference()
    blobs = {}
    L = tiny_openai_cfg().layers
    for tag, quick, unlocked, steps, size in (("blocks/", False, L, 3, 32), ("stem/", False, L + 2, 3, 32), ("stem64/", False, L + 2, 3, 64),
                                              ("all/", False, None, 3, 32), ("q/blocks/", True, L, 1, 32)):
        cfg = tiny_openai_cfg(quick)
        assert cfg.image_size == 32
        student, losses, lrs, grads, groups = run(oc, cfg, unlocked, steps, size)
        blob = blobs.setdefault(FILES[tag], {})
        assert losses[0] >= 0.5, (tag, losses)
        blob[tag + "losses"], blob[tag + "lrs"] = np.array(losses, np.float64), np.array(lrs, np.float64)
        blob[tag + "recipe"] = np.array(json.dumps(dict(TINY, seed_w=STUDENT_SEED, seed_t=TEACHER_SEED, seed_b=SEED_B, steps=steps, unlocked=unlocked,
                                                        lock=unlocked is not None, image_size=size, quick=quick)))
        blob[tag + "trainable"] = np.array(sorted(n for n, k in groups.items() if n.startswith("visual.") and k != "frozen"))
        none = []
        for n, g in grads.items():
            if g is None:
                none.append(n)
            elif n.startswith("visual.") and ".resblocks." in n and tag == "all/":
                blobs.setdefault("_all_b" + n.split(".resblocks.")[1].split(".")[0], {})[tag + "grad/" + n] = g.numpy()
            elif n.startswith("visual.") and (".resblocks." not in n or n.endswith(SOME[tag])):
                blob[tag + "grad/" + n] = g.numpy()
        blob[tag + "grad_none"] = np.array(none)
        if steps > 1:
            for n, p in student.named_parameters():
                if n.startswith("visual.") and p.requires_grad and ".resblocks." not in n:
                    blob[tag + "final/" + n] = p.detach().numpy()
        print(tag, "losses", losses, "grad_none", none)
    for suffix, blob in blobs.items():
        out = ROOT / "tests" / "golden" / f"tiny_openai_maskattn_grad{suffix}.npz"
        np.savez_compressed(out, **blob)
        assert out.stat().st_size < 2 ** 20, out
        print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
