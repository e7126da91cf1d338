"""TEST INFRASTRUCTURE -- per-kernel reference of the detector backbone's token taps: RefOps plus tokens_to_nchw (forms 1 / 2 of
cs_transpose_bf16, include/clipself_hip.h) in torch.  The frozen oracle/ops_ref.RefOps deliberately lacks it: a tower on plain RefOps refuses
encode_dense(taps=...).  Also the golden backbone fixtures' loader, the model builder and the error measures of
profiles/fvit_backbone_parity.md."""
import dataclasses
import json
from pathlib import Path

import numpy as np
import torch

from oracle.ops_ref import RefOps

# Asserted bounds of the golden comparisons on the MI355X (profiles/fvit_backbone_parity.md): 3 x the worst measurement over both fixtures
# (taps 5.360e-3, map 6.235e-3 rel-L2, 5.620e-5 1 - cos, all on tiny_fvit_backbone)
BOUND_TAP_REL_L2, BOUND_MAP_REL_L2, BOUND_MAP_ONE_MINUS_COS = 1.61e-2, 1.88e-2, 1.69e-4

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ("tiny_fvit_backbone", "tiny_fvit_backbone_g6")
LAYERS, OUT_INDICES = 4, [0, 1, 2, 3]


class RefOpsBackbone(RefOps):
    name = "ref+taps"
    TOKEN_TAPS = True

    def tokens_to_nchw(self, x, B, N, C, out):
        """out[b, c, p] = x[b*N + 1 + p, c]; one rounding (RNE) when out is bf16."""
        assert x.dtype == torch.float32 and x.shape[0] == B * N and out.is_contiguous() and tuple(out.shape[:2]) == (B, C)
        out.copy_(x[:, :C].reshape(B, N, C)[:, 1:].permute(0, 2, 1).reshape(out.shape).to(out.dtype))


def backbone_cfg():
    """The seeded four-block EVA02 miniature of the fixtures (tools/gen_golden_fvit.py)."""
    from clipself_amd.config import tiny_cfg
    return dataclasses.replace(tiny_cfg(), layers=LAYERS, name="EVA02-tiny-fvit-test")


def load_fixture(name):
    """-> (images fp32 [B, 3, S, S], [four taps fp32 [B, C, h, w]], map fp32 [B, E, h, w], seed)."""
    with np.load(GOLDEN / f"{name}.npz") as g:
        meta = json.loads(str(g["meta"]))
        taps = [torch.from_numpy(g[f"tap{i}"]) for i in range(len(meta["out_indices"]))]
        assert meta["out_indices"] == OUT_INDICES and meta["layers"] == LAYERS
        S = meta["image_size"]
        images = np.random.Generator(np.random.PCG64(meta["image_seed"])).standard_normal((2, 3, S, S), dtype=np.float32)
        return torch.from_numpy(images), taps, torch.from_numpy(g["feature_map"]), meta["seed"]


def build_tower(ops, seed, cfg=None):
    """Frozen CustomCLIP of the miniature with the seeded visual state loaded -> its visual tower."""
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import CustomCLIP
    cfg = cfg or backbone_cfg()
    model = CustomCLIP(cfg, ops=ops, trainable=False, with_text=False)
    model.visual.engine.load_state(seeded_visual_state(cfg, seed))
    return model.visual


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def one_minus_cos(got, want):
    """max over positions of 1 - cos between the channel vectors of two [B, E, h, w] maps."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((1.0 - torch.nn.functional.cosine_similarity(got, want, dim=1)).max())
