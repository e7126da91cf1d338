"""TEST INFRASTRUCTURE -- per-kernel reference of the text tower's attention: RefOps plus cs_attn_query_fwd(allow == NULL), causal
self-attention, in torch at the kernel's rounding points (include/clipself_hip.h).  The frozen oracle/ops_ref.RefOps deliberately lacks it:
a model on plain RefOps refuses encode_text.  Also the golden text fixtures' loader and the two error measures of profiles/text_tower_parity.md."""
import json
from pathlib import Path

import numpy as np
import torch

from oracle.ops_ref import RefOps

# Asserted bounds of the golden comparisons (profiles/text_tower_parity.md): 3 x the worst MI355X measurement over the four fixtures
BOUND_REL_L2, BOUND_ONE_MINUS_COS = 2.2e-2, 1.2e-4
# Two runs of the SAME rounding points (HIP against the CPU RefOpsText run of the same model; trimmed against untrimmed; chunked against
# whole) differ only where another fp32 summation order flips a bf16 rounding: rel-L2 of the features (profiles/text_tower_parity.md)
BOUND_SAME_ROUNDING = 2.0 ** -8

GOLDEN = Path(__file__).resolve().parent / "golden"
# fixture file -> (arch, quick_gelu, context) of clipself_amd.config.tiny_text_cfg
FIXTURES = {"tiny_text_openai": ("openai", False, 16), "tiny_text_openai_quickgelu": ("openai", True, 16), "tiny_text_eva": ("eva02", False, 16),
            "tiny_text_ctx77": ("openai", False, 77)}


class RefOpsText(RefOps):
    name = "ref+text"
    ATTN_CAUSAL = True

    def attn_query_fwd(self, q, kv, allow, out, B, Q, Ntok, H, scale, lse=None):
        """allow=None: query row r of a sequence attends keys 0..r -- fp32 scores, exp(s - max) rounded to bf16 for P.V, fp32 row sum of the
        unrounded exponentials, one rounding of the output (modelled on tests/_maskattn_ref.RefOpsExtra.attn_query_fwd)."""
        if allow is not None:
            assert lse is None
            return super().attn_query_fwd(q, kv, allow, out, B, Q, Ntok, H, scale)
        assert Q == Ntok and lse is None and Ntok <= 128
        C = H * 64
        heads = lambda t: t[:, :C].float().reshape(B, Ntok, H, 64).permute(0, 2, 1, 3)
        s = (heads(q) @ heads(kv[:, :C]).transpose(-1, -2)) * scale
        s = s.masked_fill(torch.ones(Ntok, Ntok, dtype=torch.bool).triu_(1), float("-inf"))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (self._r(e) @ heads(kv[:, C:2 * C])) / e.sum(-1, keepdim=True)
        out[:, :C] = o.permute(0, 2, 1, 3).reshape(B * Ntok, C).to(torch.bfloat16)


def load_fixture(name):
    """-> (cfg, ids int64 [B, ctx], features fp32 [B, E], {state-dict key: shape}, seed)."""
    from clipself_amd.config import tiny_text_cfg
    arch, quick, ctx = FIXTURES[name]
    with np.load(GOLDEN / f"{name}.npz") as g:
        ids, feats, meta = torch.from_numpy(g["ids"]).long(), torch.from_numpy(g["features"]), json.loads(str(g["meta"]))
    return tiny_text_cfg(arch, quick, ctx), ids, feats, {k: tuple(v) for k, v in meta["state_shapes"].items()}, meta["seed"]


def build_model(cfg, ops, seed):
    """The model family of cfg (trainable=False) with the seeded text state loaded."""
    from clipself_amd.init import seeded_text_state
    from clipself_amd.open_clip import CLIP, CustomCLIP
    model = (CLIP if cfg.arch == "openai" else CustomCLIP)(cfg, ops=ops, trainable=False)
    res = model.load_state_dict(seeded_text_state(cfg, seed), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    return model


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def one_minus_cos(got, want):
    """max over rows of 1 - cos(got_row, want_row)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((1.0 - torch.nn.functional.cosine_similarity(got, want, dim=-1)).max())
