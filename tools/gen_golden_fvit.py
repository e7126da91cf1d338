"""TEST INFRASTRUCTURE -- golden vectors of the reference's detector backbone pass.  Runs only where the reference checkout exists:
    python tools/gen_golden_fvit.py

F-ViT/models/evaclip_vit.py itself cannot be imported (it needs mmcv and mmdet), so this script imports the real reference tower
(oracle/ref_import.import_reference), builds a seeded four-block EVA02 miniature with its factory -- registered the way
oracle/gen_golden.py::_register_tiny does -- and calls that tower's own modules in the order EvaCLIPViT.forward does (:61-106) in evaluation
mode: patch embedding, class token, rescaled position table, every block but the last with a tap after each listed index, the last block's
forward_without_attn, final norm, head, L2 normalisation.  CPU, fp32.  Neither weights nor images are stored (the tests regenerate both from the recorded seeds):

  tests/golden/tiny_fvit_backbone.npz      2 images at the native 32 x 32 (4 x 4 tokens), out_indices [0, 1, 2, 3]
  tests/golden/tiny_fvit_backbone_g6.npz   the same tower at 48 x 48 (6 x 6 tokens): bicubic position-table rescale, recalculated rotary tables
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from clipself_amd.config import tiny_cfg                           # noqa: E402
from clipself_amd.init import seeded_visual_state                  # noqa: E402
from oracle.gen_golden import _build, _register_tiny               # noqa: E402
from oracle.ref_import import import_reference                     # noqa: E402

SEED, LAYERS, OUT_INDICES = 13, 4, [0, 1, 2, 3]


def backbone_pass(visual, images, out_indices):
    """The tower's modules in the backbone's order; returns ([B, C, h, w] per tapped block, [B, E, h, w])."""
    p = visual.patch_embed.patch_size
    B, h, w = images.shape[0], images.shape[2] // p[0], images.shape[3] // p[1]
    nchw = lambda t: t[:, 1:].permute(0, 2, 1).contiguous().view(B, -1, h, w)
    with torch.no_grad():
        x = torch.cat((visual.cls_token.expand(B, -1, -1), visual.patch_embed(images)), dim=1)
        x = x + visual.rescale_positional_embedding(out_size=(h, w))
        x = visual.patch_dropout(visual.pos_drop(x))                # both identities in evaluation mode
        assert visual.rel_pos_bias is None and visual.fc_norm is None
        taps = []
        last = len(visual.blocks) - 1
        for i, blk in enumerate(visual.blocks[:-1]):
            x = blk(x, rel_pos_bias=None)
            if i in out_indices:
                taps.append(nchw(x))
        x = visual.blocks[-1].forward_without_attn(x)
        if last in out_indices:
            taps.append(nchw(x))
        f = torch.nn.functional.normalize(visual.head(visual.norm(x[:, 1:])), dim=-1)
        return taps, f.view(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


def main():
    torch.manual_seed(0)
    oc = import_reference()
    assert os.environ.get("RoPE") in (None, "1")
    cfg = _register_tiny(oc, dataclasses.replace(tiny_cfg(), layers=LAYERS, name="EVA02-tiny-fvit-test"))
    model = _build(oc, cfg, SEED)
    model.eval()
    assert set(seeded_visual_state(cfg, SEED)) <= set(model.state_dict())
    for name, size, seed in (("tiny_fvit_backbone", cfg.image_size, 41), ("tiny_fvit_backbone_g6", 48, 42)):
        g = np.random.Generator(np.random.PCG64(seed))
        images = g.standard_normal((2, 3, size, size), dtype=np.float32)
        taps, fmap = backbone_pass(model.visual, torch.from_numpy(images), OUT_INDICES)
        # the public dense path of the same model agrees with the module-by-module pass: the pass above is the tower's own arithmetic
        ref = model.encode_dense(torch.from_numpy(images), normalize=False, keep_shape=True)
        assert torch.allclose(ref, fmap, atol=1e-6), float((ref - fmap).abs().max())
        assert len(taps) == 4 and all(bool(torch.isfinite(t).all()) for t in taps + [fmap])
        meta = {"seed": SEED, "cfg": cfg.name, "layers": LAYERS, "out_indices": OUT_INDICES, "image_size": size, "image_seed": seed}
        out = ROOT / "tests" / "golden" / f"{name}.npz"
        np.savez_compressed(out, feature_map=fmap.numpy().astype(np.float32), meta=np.array(json.dumps(meta)),
                            **{f"tap{i}": t.numpy().astype(np.float32) for i, t in enumerate(taps)})
        assert out.stat().st_size < 2 ** 20, out
        print(name, "grid", fmap.shape[-1], "|tap| mean", [round(float(t.abs().mean()), 4) for t in taps], out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
