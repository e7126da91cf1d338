"""Inference engine of the frozen text tower (`encode_text`): the reference's TextTransformer (eva_clip/transformer.py:642-737, the EVA
family's `model.text`) and the text half of open_clip's CLIP (model.py:199-212,269-281) on the kernels of the vision towers.

  embedding   transformer.py:724-726   token_embedding(ids) + positional_embedding            (torch row gather: glue)
  block       transformer.py:232-244   x += out_proj(MHA(ln_1 x, causal mask)); x += c_proj(act(c_fc(ln_2 x)))   -- the OpenAI-CLIP
                                       block with LayerNorm eps 1e-5: what follows the attention is engine_openai.block_fwd_mlp
  attention   transformer.py:714-720   additive triu(-inf) mask = causal self-attention: ops.attn_query_fwd(allow=None)
  head        transformer.py:731-736   ln_final(x)[arange, ids.argmax(-1)] @ text_projection

The tower is frozen and never differentiated.  A batch is trimmed to its longest prompt, L_eff = max(eot) + 1: under the causal mask row
`eot` sees positions <= eot only and ln_final / the projection are per-row, so the positions behind the last end-of-text token of the batch
change nothing that is returned -- exact, not an approximation (trim=False runs the full context; tests compare the two).
"""
from __future__ import annotations

import torch

from .config import TowerCfg
from .engine_base import BF16, EPI_BF16, EPI_F32, F32
from .engine_openai import block_fwd_mlp

LN_EPS = 1e-5                     # nn.LayerNorm default: the text towers of both families (transformer.py:52-58)
MAX_CONTEXT = 128                 # cs_attn_query_fwd(allow=NULL)
_MATRICES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def validate_ids(text, cfg: TowerCfg):
    """ValueError unless `text` is an integer tensor [B, text_context] of ids in [0, text_vocab) -- checked where the tensor lives, before
    any kernel runs (an id outside the table would be an out-of-bounds row gather)."""
    if not isinstance(text, torch.Tensor) or text.dim() != 2 or text.is_floating_point() or text.is_complex() or text.dtype == torch.bool:
        raise ValueError(f"encode_text takes an integer tensor of token ids [batch, {cfg.text_context}], got "
                         f"{tuple(text.shape) if isinstance(text, torch.Tensor) else type(text).__name__}"
                         f"{' ' + str(text.dtype) if isinstance(text, torch.Tensor) else ''}")
    if text.shape[1] != cfg.text_context:
        raise ValueError(f"token ids must be exactly text_context = {cfg.text_context} wide, got {text.shape[1]}")
    if text.numel():
        lo, hi = (int(v) for v in torch.aminmax(text))
        if lo < 0 or hi >= cfg.text_vocab:
            raise ValueError(f"token ids must lie in [0, {cfg.text_vocab}), got [{lo}, {hi}]")


class TextEngine:
    """params: reference name (without the family's prefix) -> fp32 tensor on `device`, the live parameters of FrozenTextTower.  The bf16
    MFMA operands (and text_projection^T for the NT head GEMM) are built on the first encode() and rebuilt after invalidate(), which
    FrozenTextTower calls from every load_state_dict; in-place edits of the parameters are also noticed through their version counters.
    A write that goes through `param.data` advances no counter: call invalidate() after one.  A model that never encodes text allocates
    nothing."""

    def __init__(self, cfg: TowerCfg, ops, params: dict, device):
        W, H = cfg.text_width, cfg.text_heads
        if W % H or W // H != 64 or W % 64 or cfg.embed_dim % 64:
            raise NotImplementedError(f"{cfg.name}: the text tower runs on the head-dim-64 attention kernels (text width {W} / {H} heads; "
                                      f"width and embed_dim multiples of 64)")
        if cfg.text_context > MAX_CONTEXT:
            raise NotImplementedError(f"{cfg.name}: text context {cfg.text_context} > {MAX_CONTEXT} tokens")
        if not getattr(ops, "ATTN_CAUSAL", False):
            raise NotImplementedError(f"encode_text needs causal self-attention, attn_query_fwd(allow=None), which the kernel backend "
                                      f"{getattr(ops, 'name', type(ops).__name__)!r} does not provide (no ATTN_CAUSAL)")
        self.cfg, self.ops, self.p, self.device = cfg, ops, params, device
        self.w = {}
        self._key = None

    def invalidate(self):
        """The parameters changed: the next encode() rebuilds the bf16 shadows."""
        self._key = None
        self.w = {}

    def _versions(self):
        try:
            return tuple(t._version for t in self.p.values())
        except RuntimeError:              # inference tensors carry no version counter: rebuild every time
            return None

    def sync_shadow(self):
        key = self._versions()
        if self.w and key is not None and key == self._key:
            return
        with torch.no_grad():
            self.w = {n: t.detach().to(BF16).contiguous() for n, t in self.p.items() if n.endswith(_MATRICES)}
            self.w["text_projection_t"] = self.p["text_projection"].detach().T.to(BF16).contiguous()      # [E, W]
        self._key = key

    def _block(self, i, x, B, L):
        """transformer.py:232-244 in place on the fp32 stream x [B*L, W]: ln_1, in_proj and the causal attention here, the rest of the
        block is engine_openai.block_fwd_mlp, shared with the vision tower."""
        ops, cfg, p, w = self.ops, self.cfg, self.p, self.w
        W, H, M = cfg.text_width, cfg.text_heads, B * L
        b = f"transformer.resblocks.{i}."
        ln1 = ops.empty((M, W), BF16)
        ops.layernorm_fwd(x, p[b + "ln_1.weight"], p[b + "ln_1.bias"], ln1, None, None, LN_EPS)
        qkv = ops.empty((M, 3 * W), BF16)
        ops.gemm_nt(ln1, w[b + "attn.in_proj_weight"], qkv, bias=p[b + "attn.in_proj_bias"], epi=EPI_BF16)
        att = ops.empty((M, W), BF16)
        ops.attn_query_fwd(qkv[:, :W], qkv[:, W:], None, att, B, L, L, H, 64 ** -0.5)
        block_fwd_mlp(ops, p, w, b, LN_EPS, cfg.quick_gelu, x, att)

    @torch.no_grad()
    def encode(self, text, trim: bool = True, chunk: int = 4096):
        """text: integer ids [B, text_context] (validated by the caller's validate_ids) -> fp32 [B, embed_dim], unnormalised."""
        ops, cfg, p = self.ops, self.cfg, self.p
        W, E = cfg.text_width, cfg.embed_dim
        self.sync_shadow()
        text = text.to(self.device)
        outs = []
        for k0 in range(0, text.shape[0], chunk):
            ids = text[k0:k0 + chunk]
            B = ids.shape[0]
            eot = ids.argmax(dim=-1)                                    # the first maximum wins, as in the reference's indexing
            L = int(eot.max()) + 1 if trim else cfg.text_context
            x = (p["token_embedding.weight"].detach()[ids[:, :L]] + p["positional_embedding"].detach()[:L]).reshape(B * L, W).contiguous()
            for i in range(cfg.text_layers):
                self._block(i, x, B, L)
            rows = x.view(B, L, W)[torch.arange(B, device=self.device), eot].contiguous()
            lnf = ops.empty((B, W), BF16)
            ops.layernorm_fwd(rows, p["ln_final.weight"], p["ln_final.bias"], lnf, None, None, LN_EPS)
            out = ops.empty((B, E), F32)
            ops.gemm_nt(lnf, self.w["text_projection_t"], out, epi=EPI_F32)
            outs.append(out)
        if not outs:
            return torch.zeros((0, E), dtype=F32, device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs)
