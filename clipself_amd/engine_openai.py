"""Step engine of the OpenAI-CLIP vision transformer on the CLIPSelf hot path: the flat-buffer
machinery and tower-level drivers of engine_base.TowerEngine and the same kernels as the EVA02 engine, with this tower family's layout, stem,
block schedule and head.  Where the reference
does each stage (paths under /root/reference/src/open_clip/):

  stem            transformer.py:551-569     conv1 (no bias; im2row + GEMM) + class_embedding + positional_embedding, ln_pre
  block           transformer.py:232-244     x += out_proj(MHA(ln_1 x)); x += c_proj(act(c_fc(ln_2 x)))
  attention       transformer.py:203,217-230 nn.MultiheadAttention: fused in_proj [3C,C] (+bias on q, k and v), softmax(qk^T/8)v
  last dense blk  transformer.py:247-260     out_proj(v-slice of in_proj(ln_1 x)), no attention (maskclip style)
  MLP             transformer.py:209-213,31-34   GELU (erf) or QuickGELU
  image head      transformer.py:486-494     ln_post(x[:,0]) @ proj
  dense head      transformer.py:576-587     normalize(ln_post(x[:,1:]) @ proj)
  mask attention  transformer.py:660-671,736-834   extract_type='v1' / encode_masks(mask_attn=True): extra query tokens (mask_attn_pool / backward_mask_attn)
  lock            transformer.py:391-422     groups = [stem, positional_embedding, blocks..., last block]; the last n train
                                             (n > L: positional_embedding, then conv1 / class_embedding / ln_pre: _stem_bwd)

The frozen teacher runs TowerEngine.encode_image like the EVA02 one: CLS-query-only last block (TowerEngine._block_fwd_cls), ln_1 / ln_2
folded into the in_proj / c_fc GEMMs with the residual GEMMs emitting the bf16 copy and the row statistics of the stream
(`_teacher_block_folded`).  The head of the backward pass (workspaces, ln_post, proj) is TowerEngine's too, for backward_dense and
backward_mask_attn alike.

The block's forward behind the attention core -- out_proj (+x), ln_2, c_fc + activation, c_proj (+x1) -- is written once, in block_fwd_mlp
below (the twin of _block_bwd_mlp): every row set of this engine runs it through `_block_tail` (image tokens, the CLS rows, mask-attention
passengers) and so does the text tower (engine_text.py).

Differences to the EVA02 schedule: no RoPE (the attention kernels run without tables: rope_tables), no sub-LayerNorms, `proj` is a bias-free
[C,E] matrix kept transposed for the forward GEMM, and the last dense block owns no never-reached *tensor* (q/k are rows of the one
in_proj_weight parameter, whose gradient rows stay zero -- exactly what autograd hands torch's AdamW).
"""
from __future__ import annotations

import os

import torch

from .config import TowerCfg
from .engine_base import (BF16, DX_F32_ACCUM, DX_F32_ASSIGN, EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_PATCH_F32, EPI_QGELU_BF16,
                          EPI_RESID_F32, F32, TowerEngine, _round_up)


def clip_vit_layout(cfg: TowerCfg, prefix: str = "visual."):
    """Allocation groups in layer order with the reference's state-dict names (transformer.py:355-389,190-215)."""
    C, Hd, E, p = cfg.width, cfg.hidden, cfg.embed_dim, cfg.patch_size
    Kp = _round_up(3 * p * p, 64)
    t = lambda name, shape, storage=None: (name, shape, storage if storage is not None else shape)
    groups = [[t(prefix + "class_embedding", (C,))], [t(prefix + "positional_embedding", (cfg.tokens, C))],
              [t(prefix + "conv1.weight", (C, 3, p, p), (C, Kp))], [t(prefix + "ln_pre.weight", (C,))], [t(prefix + "ln_pre.bias", (C,))]]
    for i in range(cfg.layers):
        b = f"{prefix}{ClipVitEngine.BLOCK_TAG}{i}."
        groups += [[t(b + "ln_1.weight", (C,))], [t(b + "ln_1.bias", (C,))],
                   [t(b + "attn.in_proj_weight", (3 * C, C))], [t(b + "attn.in_proj_bias", (3 * C,))],
                   [t(b + "attn.out_proj.weight", (C, C))], [t(b + "attn.out_proj.bias", (C,))],
                   [t(b + "ln_2.weight", (C,))], [t(b + "ln_2.bias", (C,))],
                   [t(b + "mlp.c_fc.weight", (Hd, C))], [t(b + "mlp.c_fc.bias", (Hd,))],
                   [t(b + "mlp.c_proj.weight", (C, Hd))], [t(b + "mlp.c_proj.bias", (C,))]]
    groups += [[t(prefix + "ln_post.weight", (C,))], [t(prefix + "ln_post.bias", (C,))], [t(prefix + "proj", (C, E))]]
    return groups


def act_epilogue(quick_gelu: bool):
    """The GEMM epilogue that applies this family's MLP activation (transformer.py:31-34,209-213)."""
    return EPI_QGELU_BF16 if quick_gelu else EPI_GELU_BF16


def block_fwd_mlp(ops, p, w, b, eps, quick_gelu, x, att, save=None, inplace=True):
    """Row-wise half of a block's forward behind the attention core: x1 = x + out_proj(att), x2 = x1 + c_proj(act(c_fc(ln_2 x1))) -> x2.
    p / w: fp32 parameters and bf16 matrices by name, b: the block's name prefix, x fp32 [rows, C], att bf16 [rows, C].  inplace: x1 and x2
    are x itself.  save (dict): the activations _block_bwd_mlp needs are kept and put into it -- c_fc's output before the activation
    (fc, hence the separate activation pass) and ln_2's row statistics; otherwise the activation is c_fc's epilogue."""
    R, C = x.shape
    Hd = w[b + "mlp.c_fc.weight"].shape[0]
    keep = save is not None
    x1 = x if inplace else ops.empty((R, C), F32)
    ops.gemm_nt(att, w[b + "attn.out_proj.weight"], x1, bias=p[b + "attn.out_proj.bias"], extra=x, epi=EPI_RESID_F32)
    ln2 = ops.empty((R, C), BF16)
    m2, r2 = (ops.empty((R,), F32), ops.empty((R,), F32)) if keep else (None, None)
    ops.layernorm_fwd(x1, p[b + "ln_2.weight"], p[b + "ln_2.bias"], ln2, m2, r2, eps)
    hid = ops.empty((R, Hd), BF16)
    if keep:
        fc = ops.empty((R, Hd), BF16)
        ops.gemm_nt(ln2, w[b + "mlp.c_fc.weight"], fc, bias=p[b + "mlp.c_fc.bias"], epi=EPI_BF16)
        ops.gelu_fwd(fc, hid, quick_gelu)
    else:
        ops.gemm_nt(ln2, w[b + "mlp.c_fc.weight"], hid, bias=p[b + "mlp.c_fc.bias"], epi=act_epilogue(quick_gelu))
    x2 = x1 if inplace else ops.empty((R, C), F32)
    ops.gemm_nt(hid, w[b + "mlp.c_proj.weight"], x2, bias=p[b + "mlp.c_proj.bias"], extra=x1, epi=EPI_RESID_F32)
    if keep:
        save.update(x1=x1, ln2=ln2, st2=(m2, r2), fc=fc, hid=hid)
    return x2


class ClipVitEngine(TowerEngine):
    BLOCK_TAG, NORM1, FINAL_NORM, RESID_BIAS = "transformer.resblocks.", "ln_1", "ln_post", "mlp.c_proj.bias"
    HEAD_FWD_TRANSPOSED = True                                  # proj^T serves the forward head GEMM of frozen towers too

    def __init__(self, cfg: TowerCfg, ops, trainable: bool = False, prefix: str = "visual."):
        if cfg.hidden % 64 or cfg.width % 64 or cfg.embed_dim % 64:
            raise NotImplementedError(f"{cfg.name}: width, MLP width and embed_dim must be multiples of 64")
        super().__init__(cfg, ops, trainable=trainable, prefix=prefix)
        # (fold_block_ln here: ln_1 / ln_2 inside the in_proj / c_fc GEMM epilogues; cls_only_last_block: forward() consumes x[:, 0] alone,
        # transformer.py:486-494)
        self.fold_cls_block = True                              # ln_1 of the CLS-only block folded into its K|V GEMM (A/B switch)
        # lock() with more groups than blocks (transformer.py:391-422): 1 = positional_embedding trains, 2 = conv1 / class_embedding / ln_pre too
        self.stem_level = 0
        self._ctx_mask = None                                   # mask_attn_pool(need_grad=True) -> backward_mask_attn (its own slot: a v2 context survives)

    def _layout(self):
        return clip_vit_layout(self.cfg, self.prefix)

    def _pos_table(self, views):
        return views[self.prefix + "positional_embedding"]

    # ------------------------------------------------------------------------------------------ hooks of the tower drivers
    def _cls_block_folds(self):
        return self.fold_cls_block

    def _lo_plane(self, last, cls_folded):
        return last > 1 or cls_folded

    def _bwd_widths(self):
        return self.cfg.width, max(self.cfg.hidden, 3 * self.cfg.width)

    def _head(self, rows, out):
        """out[M,E] f32 = bf16(rows) . proj   (no bias: transformer.py:492-493,583-584)."""
        self.ops.gemm_nt(rows, self.wt["head_fwd"][:, :self.cfg.width], out, epi=EPI_F32)

    def _head_dgrad(self, d_feats, d_lnf):
        self.ops.gemm_nt(d_feats, self.w[self.prefix + "proj"], d_lnf, epi=EPI_BF16)      # [M,E] . proj^T: proj [C,E] is already "W^T"

    def _head_wgrad(self, d_feats, lnf, ws):
        """dproj [C,E] = LN(x)^T . dfeats   (transformer.py:583-584: tokens @ proj; no bias)."""
        self._wgrad(lnf, d_feats, self.g[self.prefix + "proj"])

    # ------------------------------------------------------------------------------------------ parameters
    def sync_transposed(self, blocks=None):
        """proj^T [E,C] for the forward head GEMM (every tower), and W^T shadows of the trainable blocks for the dgrad GEMMs."""
        pairs = [(self.w[self.prefix + "proj"], self._wt_alloc("head_fwd", self.cfg.width, self.cfg.embed_dim))]
        if self.trainable:
            pairs += self._block_wt_pairs(blocks)
        self.ops.transpose_bf16_batched(pairs)

    def _block_linears(self, i):
        b = self._b(i)
        return (("qkv", self.w[b + "attn.in_proj_weight"]), ("proj", self.w[b + "attn.out_proj.weight"]),
                ("fc", self.w[b + "mlp.c_fc.weight"]), ("cproj", self.w[b + "mlp.c_proj.weight"]))

    def _qkv_operands(self, i):
        b = self._b(i)
        return self.w[b + "attn.in_proj_weight"], self.p[b + "attn.in_proj_bias"]

    def _build_folds(self):
        """gamma (.) W in bf16, its row sums and W.beta + b for ln_1 -> in_proj and ln_2 -> c_fc of every block (one-time, after a load)."""
        self.fold = {}
        with torch.no_grad():
            for i in range(self.cfg.layers):
                b = self._b(i)
                out = {}
                for key, wname, bname, ln in (("qkv", "attn.in_proj_weight", "attn.in_proj_bias", "ln_1"), ("fc", "mlp.c_fc.weight", "mlp.c_fc.bias", "ln_2")):
                    W, bias = self.p[b + wname], self.p[b + bname]
                    Wf = (W * self.p[b + ln + ".weight"][None, :]).to(BF16).contiguous()
                    out[key] = (Wf, Wf.float().sum(dim=1).contiguous(), (W @ self.p[b + ln + ".bias"] + bias).contiguous())
                self.fold[i] = out

    def set_trainable_blocks(self, unlocked_groups: int):
        """VisionTransformer.lock (transformer.py:391-422): of the groups [[conv1, class_embedding, ln_pre], positional_embedding, block 0 ..
        L-1] the last n train; n = 0 freezes everything, n = L + 1 adds the positional embedding, n >= L + 2 the stem (a slice longer than
        the list is the whole list).  ln_post and proj never train in this family (:405-408)."""
        L = self.cfg.layers
        self.stem_level = min(max(unlocked_groups - L, 0), 2)
        super().set_trainable_blocks(min(unlocked_groups, L))               # (clears train_all)
        if unlocked_groups <= 0:
            self.first_trainable = L
            if self.trainable:
                self.flags.zero_()

    def set_trainable_all(self):
        """No lock at all (training.main without --lock-image, src/training/main.py:161-166): besides the stem and the blocks, ln_post and proj
        train (transformer.py:576-584 on the dense path)."""
        self.stem_level = 2
        super().set_trainable_all()

    def _nonblock_trains(self, name):
        if self.train_all:
            return True
        tail = name[len(self.prefix):]
        if tail == "positional_embedding":
            return self.stem_level >= 1
        return self.stem_level >= 2 and tail in ("conv1.weight", "class_embedding", "ln_pre.weight", "ln_pre.bias")

    def _pos_trains(self):
        return self.stem_level >= 1

    # ------------------------------------------------------------------------------------------ tables
    def rope_tables(self, grid: int):
        """No rotary embedding in this family.  On a backend that advertises ATTN_NO_ROPE the attention ops get (None, None) -- kernels
        without tables and without the rotation; elsewhere (the CPU reference), or with CLIPSELF_ATTN_IDENTITY_ROPE=1 (the A/B switch,
        read per call), cos = 1, sin = 0 turn the rotation into the identity.  Same values either way."""
        if getattr(self.ops, "ATTN_NO_ROPE", False) and os.environ.get("CLIPSELF_ATTN_IDENTITY_ROPE", "0") in ("", "0"):
            return None, None
        key = ("rope", grid)
        if key not in self._tables:
            shape = (grid * grid, self.cfg.head_width)
            self._tables[key] = (torch.ones(shape, dtype=F32, device=self.device), torch.zeros(shape, dtype=F32, device=self.device))
        return self._tables[key]

    # ------------------------------------------------------------------------------------------ forward pieces
    def _stem(self, images, keep=None):
        """keep (dict, stem_level > 0): the im2row matrix, ln_pre's input and row statistics for _stem_bwd."""
        ops, cfg, P = self.ops, self.cfg, self.prefix
        B, _, S, _ = images.shape
        p, C = cfg.patch_size, cfg.width
        g = S // p
        N = g * g + 1
        A = ops.empty((B * g * g, self.Kpe), BF16)
        ops.im2row(images.contiguous(), A, p)
        x = ops.empty((B, N, C), F32)
        pos = self.pos_for(g)
        ops.gemm_nt(A, self.storage_of(self.shadow, P + "conv1.weight"), x.view(B * N, C), extra=pos, epi=EPI_PATCH_F32, group=g * g)
        ops.cls_row(x, self.p[P + "class_embedding"], pos)
        y = ops.empty((B, N, C), F32)                       # ln_pre's output is the residual stream
        mean = rstd = None
        if keep is not None:
            mean, rstd = ops.empty((B * N,), F32), ops.empty((B * N,), F32)
            keep.update(patches=A, x_pre=x.view(B * N, C), st=(mean, rstd))
        ops.layernorm_fwd_f32(x.view(B * N, C), self.p[P + "ln_pre.weight"], self.p[P + "ln_pre.bias"], y.view(B * N, C), mean, rstd, cfg.ln_eps)
        return y, g

    def _block_tail(self, i, x, att, save=None, inplace=True):
        """block_fwd_mlp on this tower's parameters: the forward twin of _block_bwd_mlp, for whichever rows x holds."""
        return block_fwd_mlp(self.ops, self.p, self.w, self._b(i), self.cfg.ln_eps, self.cfg.quick_gelu, x, att, save, inplace)

    def _block_fwd(self, i, x, B, N, cos, sin, with_attn=True, save=None, inplace=True):
        ops, cfg = self.ops, self.cfg
        C, H, eps = cfg.width, cfg.heads, cfg.ln_eps
        b = self._b(i)
        M = B * N
        keep = save is not None

        ln1 = ops.empty((M, C), BF16)
        m1, r1 = self._row_stats(M, keep)
        ops.layernorm_fwd(x, self.p[b + "ln_1.weight"], self.p[b + "ln_1.bias"], ln1, m1, r1, eps)
        wqkv, bqkv = self._qkv_operands(i)
        qkv = lse = None
        att = ops.empty((M, C), BF16)
        if with_attn:
            qkv = ops.empty((M, 3 * C), BF16)
            ops.gemm_nt(ln1, wqkv, qkv, bias=bqkv, epi=EPI_BF16)
            lse = ops.empty((B * H, N), F32) if keep else None
            ops.attn_fwd(qkv, cos, sin, att, lse, B, N, H, cfg.head_width ** -0.5)
        else:
            ops.gemm_nt(ln1, wqkv[2 * C:], att, bias=bqkv[2 * C:], epi=EPI_BF16)        # proj_without_attn: the value rows only
        if keep:
            save.update(x0=x, ln1=ln1, st1=(m1, r1), qkv=qkv, lse=lse, att=att, with_attn=with_attn)
        return self._block_tail(i, x, att, save, inplace)

    def _teacher_block_folded(self, i, x, xb, st, B, N, cos, sin, emit_next, lo=None):
        """One frozen-tower block with both LayerNorms folded into the GEMMs (in place on x).  xb / st = bf16 copy and (mean, rstd) of x as
        left by the previous block's c_proj GEMM, or None (first block: plain ln_1 kernel).  Returns (xb, st) for the next block when
        emit_next.  With lo (int16 [M, C]; round 4) the stream lives in the two 16-bit planes (xb, lo) between the first residual GEMM of
        the tower, which reads fp32 x, and the last one (emit_next False), which writes fp32 x again -- cs_gemm_nt_ln_split:
        8 instead of 10 bytes per stream element and residual GEMM, same fp32 values.  This family has no LayerNorm in front of
        out_proj / c_proj (ln=None of _resid_gemm_folded), so the split kernel gets the identity statistics (mean 0, rstd 1, column sums 0: x + 1 * (acc - 0 * 0) + b)."""
        ops, cfg = self.ops, self.cfg
        C, Hd, H, eps = cfg.width, cfg.hidden, cfg.heads, cfg.ln_eps
        b = self._b(i)
        M = B * N
        first = xb is None
        qkv = self._teacher_qkv(i, x, xb, st, M)
        att = ops.empty((M, C), BF16)
        ops.attn_fwd(qkv, cos, sin, att, None, B, N, H, cfg.head_width ** -0.5)
        part = ops.empty(((C + 63) // 64, M, 2), F32)
        xb2 = xb if (lo is not None and not first) else ops.empty((M, C), BF16)
        self._resid_gemm_folded(att, self.w[b + "attn.out_proj.weight"], self.p[b + "attn.out_proj.bias"], None, x, xb2, lo, part, first=first)
        mean, rstd = ops.empty((M,), F32), ops.empty((M,), F32)
        ops.ln_stats_finalize(part, 64, C, mean, rstd, eps)
        Wf, cf, df = self.fold[i]["fc"]
        hid = ops.empty((M, Hd), BF16)
        ops.gemm_nt_ln(xb2, Wf, hid, bias=df, ln_mean=mean, ln_rstd=rstd, ln_colsum=cf, epi=act_epilogue(cfg.quick_gelu))
        self._resid_gemm_folded(hid, self.w[b + "mlp.c_proj.weight"], self.p[b + "mlp.c_proj.bias"], None, x, xb2, lo, part, last=not emit_next)
        if not emit_next:
            return None, None
        ops.ln_stats_finalize(part, 64, C, mean, rstd, eps)
        return xb2, (mean, rstd)

    # ------------------------------------------------------------------------------------------ mask-attention pooling (inference)
    def _allow_table(self, masks, B, Q, N, g):
        """uint8 [B*Q, N], 1 = query q of image b may attend token n: the CLS token and the tokens inside its mask; padding queries see everything."""
        allow = torch.ones((B, Q, N), dtype=torch.uint8, device=self.device)
        for b, m in enumerate(masks):
            assert tuple(m.shape[1:]) == (g, g), f"masks live on the {g}x{g} token grid, got {tuple(m.shape[1:])}"
            allow[b, :m.shape[0], 1:] = m.flatten(1).to(device=self.device, dtype=torch.uint8)
        return allow.view(B * Q, N)

    def mask_attn_pool(self, images, masks, chunk: int = 64, need_grad: bool = False):
        """VisionTransformer.mask_attn_pool / _mask_attn_pool (transformer.py:736-834), the pooling behind extract_type='v1' (:660-671) and
        encode_masks(mask_attn=True).  masks: list over images of bool [n_i, g, g] on the token grid.  Every mask is an extra token -- a copy
        of the image's CLS embedding after ln_pre -- that runs through ALL blocks; the reference's attention mask hides the extra tokens from
        everybody and lets token q see the CLS token plus the image tokens inside its mask, so the image tokens are exactly forward()'s and
        an extra token is a query-only passenger.  Per block: the image tokens' usual q|k|v GEMM, whose k|v columns also serve the Q extra
        queries of the image (cs_attn_query_fwd), then out_proj / MLP on the [B*Q, C] passenger stream with the same GEMM epilogues as the
        blocks.  Images with fewer masks are padded with see-everything tokens whose rows are dropped (:793-795,823-824).  -> fp32 [sum n_i, E]
        With need_grad the whole batch runs in one pass that keeps what backward_mask_attn() needs (_mask_attn_pool_train)."""
        if need_grad:
            return self._mask_attn_pool_train(images, masks)
        ops, cfg, P = self.ops, self.cfg, self.prefix
        C, H, eps, E = cfg.width, cfg.heads, cfg.ln_eps, cfg.embed_dim
        counts = [int(m.shape[0]) for m in masks]
        assert len(masks) == images.shape[0], "one mask list per image"
        Q = max(counts) if counts else 0
        if Q == 0:                                   # no image has a mask: transformer.py:823-824 returns zero rows
            return torch.zeros((0, E), dtype=F32, device=self.device)
        outs = []                                    # an image WITHOUT masks is all padding: see-everything queries whose rows are dropped (:793-795)
        for k0 in range(0, images.shape[0], chunk):
            img = images[k0:k0 + chunk]
            B = img.shape[0]
            x, g = self._stem(img)
            N = g * g + 1
            cos, sin = self.rope_tables(g)
            allow = self._allow_table(masks[k0:k0 + B], B, Q, N, g)
            xf = x.view(B * N, C)
            xm = x[:, :1, :].expand(B, Q, C).reshape(B * Q, C).contiguous()          # fp32 passenger stream
            MQ = B * Q
            for i in range(cfg.layers):
                b_ = self._b(i)
                wqkv, bqkv = self._qkv_operands(i)
                ln1 = ops.empty((B * N, C), BF16)
                ops.layernorm_fwd(xf, self.p[b_ + "ln_1.weight"], self.p[b_ + "ln_1.bias"], ln1, None, None, eps)
                qkv = ops.empty((B * N, 3 * C), BF16)
                ops.gemm_nt(ln1, wqkv, qkv, bias=bqkv, epi=EPI_BF16)
                lnm = ops.empty((MQ, C), BF16)
                ops.layernorm_fwd(xm, self.p[b_ + "ln_1.weight"], self.p[b_ + "ln_1.bias"], lnm, None, None, eps)
                qm = ops.empty((MQ, C), BF16)
                ops.gemm_nt(lnm, wqkv[:C], qm, bias=bqkv[:C], epi=EPI_BF16)
                attm = ops.empty((MQ, C), BF16)
                ops.attn_query_fwd(qm, qkv[:, C:], allow, attm, B, Q, N, H, cfg.head_width ** -0.5)
                self._block_tail(i, xm, attm)
                if i + 1 < cfg.layers:                      # the image tokens move on (they never see the passengers); not needed after the last block
                    att = ops.empty((B * N, C), BF16)
                    ops.attn_fwd(qkv, cos, sin, att, None, B, N, H, cfg.head_width ** -0.5)
                    self._block_tail(i, xf, att)
            lnp = ops.empty((MQ, C), BF16)
            ops.layernorm_fwd(xm, self.p[P + "ln_post.weight"], self.p[P + "ln_post.bias"], lnp, None, None, eps)
            pooled = ops.empty((MQ, E), F32)
            self._head(lnp, pooled)
            pooled = pooled.view(B, Q, E)
            outs += [pooled[b, :n] for b, n in enumerate(counts[k0:k0 + B])]
        return torch.cat(outs)

    # ------------------------------------------------------------------------------------------ mask-attention pooling (training)
    def _mask_attn_pool_train(self, images, masks):
        """mask_attn_pool() that keeps the activations of the trainable blocks (and of a trainable stem) for backward_mask_attn().  One row
        stream [B*N + B*Q, C] per block -- the image tokens, then the passengers -- so LayerNorm, the GEMMs and the activation stay single
        launches; only attention tells the two row sets apart (cs_attn_fwd on the image rows, cs_attn_query_fwd with its log-sum-exp on the
        passengers, whose queries are the q columns of their rows of the q|k|v matrix).  The image tokens' output of the last block is
        consumed by nobody: after its q|k|v GEMM that block runs on the passenger rows alone."""
        ops, cfg, P = self.ops, self.cfg, self.prefix
        C, H, eps, E = cfg.width, cfg.heads, cfg.ln_eps, cfg.embed_dim
        counts = [int(m.shape[0]) for m in masks]
        assert len(masks) == images.shape[0], "one mask list per image"
        Q = max(counts) if counts else 0
        if Q == 0:
            self._ctx_mask = dict(empty=True)
            return torch.zeros((0, E), dtype=F32, device=self.device)
        B = images.shape[0]
        stem_keep = {} if self._pos_trains() else None
        x, g = self._stem(images, stem_keep)
        N = g * g + 1
        BN, MQ = B * N, B * Q
        M = BN + MQ
        cos, sin = self.rope_tables(g)
        allow = self._allow_table(masks, B, Q, N, g)
        scale = cfg.head_width ** -0.5
        xs = ops.empty((M, C), F32)
        xs[:BN] = x.view(BN, C)
        xs[BN:] = x[:, :1, :].expand(B, Q, C).reshape(MQ, C)
        saves = {}
        for i in range(cfg.layers):
            b_ = self._b(i)
            last = i == cfg.layers - 1
            keep = i >= self.first_trainable
            R0 = BN if last else 0                                  # first row that continues past the attention
            R = M - R0
            ln1 = ops.empty((M, C), BF16)
            m1, r1 = self._row_stats(M, keep)
            ops.layernorm_fwd(xs, self.p[b_ + "ln_1.weight"], self.p[b_ + "ln_1.bias"], ln1, m1, r1, eps)
            qkv = ops.empty((M, 3 * C), BF16)
            wqkv, bqkv = self._qkv_operands(i)
            ops.gemm_nt(ln1, wqkv, qkv, bias=bqkv, epi=EPI_BF16)
            att = ops.empty((R, C), BF16)
            lse = None
            if not last:
                lse = ops.empty((B * H, N), F32) if keep else None
                ops.attn_fwd(qkv[:BN], cos, sin, att[:BN], lse, B, N, H, scale)
            lse_m = ops.empty((B * H, Q), F32) if keep else None
            ops.attn_query_fwd(qkv[BN:, :C], qkv[:BN, C:], allow, att[BN - R0:], B, Q, N, H, scale, **(dict(lse=lse_m) if keep else {}))
            if keep:
                saves[i] = dict(x0=xs, ln1=ln1, st1=(m1, r1), qkv=qkv, lse=lse, lse_m=lse_m, att=att, with_attn=True, R0=R0)
            xs = self._block_tail(i, xs[R0:], att, saves.get(i), inplace=not keep)
        xm = xs                                                      # [B*Q, C]: what the last block left
        lnp = ops.empty((MQ, C), BF16)
        mean, rstd = ops.empty((MQ,), F32), ops.empty((MQ,), F32)
        ops.layernorm_fwd(xm, self.p[P + "ln_post.weight"], self.p[P + "ln_post.bias"], lnp, mean, rstd, eps)
        pooled = ops.empty((MQ, E), F32)
        self._head(lnp, pooled)
        valid = torch.tensor([b * Q + r for b, n in enumerate(counts) for r in range(n)], dtype=torch.long, device=self.device)
        self._ctx_mask = dict(B=B, N=N, Q=Q, g=g, saves=saves, xL=xm, stf=(mean, rstd), lnf=lnp if self.train_all else None, cos=cos, sin=sin,
                              stem=stem_keep, allow=allow, valid=valid)
        return pooled.index_select(0, valid)

    def backward_mask_attn(self, d_pooled):
        """d_pooled: fp32 [sum n_i, E], the gradient w.r.t. what mask_attn_pool(need_grad=True) returned.  The twin of backward_dense on the
        [image tokens ; passengers] row stream: ln_post / proj from the passenger rows (train_all), per block the row-wise backward on both
        row sets and cs_attn_bwd with the passengers as its `extra` rows (the last block: passengers only, no image rows), then the
        passengers' gradient at the input of block 0 joins their image's CLS row -- they started as copies of it -- ahead of the stem.
        Padding passengers carry a zero upstream gradient and contribute exact zeros.  Hooks fire in backward_dense's order."""
        ops, cfg = self.ops, self.cfg
        c = self._ctx_mask
        if c is None:
            raise RuntimeError("backward_mask_attn() without a preceding mask_attn_pool(need_grad=True)")
        self._ctx_mask = None
        if c.get("empty"):
            return
        B, N, Q, C, E, H = c["B"], c["N"], c["Q"], cfg.width, cfg.embed_dim, cfg.heads
        BN, MQ = B * N, B * Q
        M = BN + MQ
        d_full = ops.zeros((MQ, E), F32)
        d_full.index_copy_(0, c["valid"], d_pooled.to(F32))
        d_feats = ops.empty((MQ, E), BF16)
        ops.cast_f32_bf16(d_full, d_feats)
        d_lnf = ops.empty((MQ, C), BF16)
        self._head_dgrad(d_feats, d_lnf)
        g = ops.zeros((M, C), F32)                    # image rows: nobody consumes the last block's image tokens
        gb = ops.zeros((M, C), BF16)
        ws = self._bwd_workspaces(M, B, N, Q)
        self._final_norm_bwd(c, d_feats, d_lnf, g[BN:], gb[BN:], ws)                # the head saw the passenger rows alone
        for i in range(cfg.layers - 1, self.first_trainable - 1, -1):
            s = c["saves"].pop(i)
            R0 = s["R0"]
            d_att = self._block_bwd_mlp(i, s, g[R0:], gb[R0:], ws)
            d_qkv = ops.empty((M, 3 * C), BF16)
            d_qkv[BN:, C:] = 0                                    # passenger rows: dq | 0 | 0
            qkv, att = s["qkv"], s["att"]
            extra = dict(q=qkv[BN:, :C], o=att[BN - R0:], dout=d_att[BN - R0:], lse=s["lse_m"], allow=c["allow"], dq=d_qkv[BN:, :C], Q=Q)
            if R0 == 0:
                ops.attn_bwd(qkv[:BN], att[:BN], d_att[:BN], s["lse"], c["cos"], c["sin"], d_qkv[:BN], ws[0], B, N, H, cfg.head_width ** -0.5,
                             extra=extra)
            else:
                ops.attn_bwd(qkv[:BN], None, None, None, c["cos"], c["sin"], d_qkv[:BN], ws[0], B, N, H, cfg.head_width ** -0.5, extra=extra)
            self._block_bwd_ln1(i, s, d_qkv, 0, g, gb, ws, next_bias=self._resid_bias(i - 1) if i > 0 else None)
            if self.grad_ready_hook is not None:
                self.grad_ready_hook(i)
        if c["stem"] is not None:
            g3 = g[:BN].view(B, N, C)
            g3[:, 0, :] += g[BN:].view(B, Q, C).sum(dim=1)       # every passenger started as a copy of its image's CLS row
            self._stem_bwd(g[:BN], c["stem"], B, N, c["g"], ws[0])
            if self.grad_ready_hook is not None:
                self.grad_ready_hook("stem")

    # ------------------------------------------------------------------------------------------ backward
    def _block_bwd(self, i, s, g, gb, B, N, cos, sin, ws, next_bias=None, gq=None):
        """g: fp32 [M,C] gradient w.r.t. the block output; updated in place to the gradient w.r.t. its input.  gb: its bf16 copy, already summed
        into this block's c_proj bias gradient by the LayerNorm backward that produced it; on return gb is the copy of the new g and its column
        sums have gone to `next_bias` (block i-1's c_proj bias gradient, or None).  gq: always None here (no fp8 dgrad in this family)."""
        ops, cfg = self.ops, self.cfg
        C, H = cfg.width, cfg.heads
        d_att = self._block_bwd_mlp(i, s, g, gb, ws)
        if s["with_attn"]:
            d_qkv = ops.empty((B * N, 3 * C), BF16)
            ops.attn_bwd(s["qkv"], s["att"], d_att, s["lse"], cos, sin, d_qkv, ws[0], B, N, H, cfg.head_width ** -0.5)
            self._block_bwd_ln1(i, s, d_qkv, 0, g, gb, ws, next_bias)
        else:
            self._block_bwd_ln1(i, s, d_att, 2 * C, g, gb, ws, next_bias)         # q/k rows keep their zero gradient

    def _block_bwd_mlp(self, i, s, g, gb, ws):
        """Row-wise half of a block's backward behind the attention: the MLP branch, ln_2 (g updated in place to the gradient w.r.t. x1, gb its
        bf16 copy, whose column sums go to out_proj's bias) and out_proj.  -> d_att, bf16 [rows, C]."""
        ops, cfg = self.ops, self.cfg
        C, Hd = cfg.width, cfg.hidden
        b = self._b(i)
        M = g.shape[0]
        G = self.g
        # ---- MLP: x2 = x1 + c_proj(act(c_fc(ln_2 x1))) --------------------------------------------
        self._wgrad(gb, s["hid"], G[b + "mlp.c_proj.weight"])
        d_hid = ops.empty((M, Hd), BF16)
        ops.gemm_nt(gb, self.wt[(i, "cproj")][:, :C], d_hid, epi=EPI_BF16)                   # [M,C] . c_proj[C,Hd]
        d_fc = ops.empty((M, Hd), BF16)
        ops.gelu_bwd(d_hid, s["fc"], d_fc, cfg.quick_gelu)
        ops.colsum_bf16(d_fc, G[b + "mlp.c_fc.bias"], ws[1])
        self._wgrad(d_fc, s["ln2"], G[b + "mlp.c_fc.weight"])
        d_ln2 = ops.empty((M, C), BF16)
        ops.gemm_nt(d_fc, self.wt[(i, "fc")][:, :Hd], d_ln2, epi=EPI_BF16)                   # [M,Hd] . c_fc[Hd,C]
        ops.layernorm_bwd(d_ln2, s["x1"], self.p[b + "ln_2.weight"], *s["st2"], g, DX_F32_ACCUM,
                          G[b + "ln_2.weight"], G[b + "ln_2.bias"], True, ws[0], dx_copy=gb, copy_colsum=G[b + "attn.out_proj.bias"])
        # ---- attention branch: x1 = x0 + out_proj(att) ------------------------------------------
        self._wgrad(gb, s["att"], G[b + "attn.out_proj.weight"])
        d_att = ops.empty((M, C), BF16)
        ops.gemm_nt(gb, self.wt[(i, "proj")][:, :C], d_att, epi=EPI_BF16)
        return d_att

    def _block_bwd_ln1(self, i, s, d, col0, g, gb, ws, next_bias=None):
        """... and the half in front of it: d = gradient w.r.t. columns [col0, 3C) of the q|k|v GEMM's output (col0 = 2C: the value third alone,
        the block without attention) -> in_proj's gradients, then ln_1 (g += the gradient w.r.t. the block input; gb / next_bias as in
        _block_bwd)."""
        ops, cfg = self.ops, self.cfg
        C = cfg.width
        b = self._b(i)
        G = self.g
        d_ln1 = ops.empty((d.shape[0], C), BF16)
        ops.colsum_bf16(d, G[b + "attn.in_proj_bias"][col0:], ws[1])                         # q, k and v all carry a bias here
        self._wgrad(d, s["ln1"], G[b + "attn.in_proj_weight"][col0:])
        ops.gemm_nt(d, self.wt[(i, "qkv")][:, col0:3 * C], d_ln1, epi=EPI_BF16)
        ops.layernorm_bwd(d_ln1, s["x0"], self.p[b + "ln_1.weight"], *s["st1"], g, DX_F32_ACCUM,
                          G[b + "ln_1.weight"], G[b + "ln_1.bias"], True, ws[0], dx_copy=gb if next_bias is not None else None,
                          copy_colsum=next_bias)

    def _stem_bwd(self, g, keep, B, N, grid, ws):
        """Gradients of the stem from g = d loss / d (ln_pre output) fp32 [B*N, C]  (transformer.py:551-569: x = ln_pre(cat(class_embedding,
        conv1(img)) + positional_embedding)).  ln_pre backward (its gamma / beta at stem level 2), then: positional_embedding <- sum over images
        (_pos_grad), class_embedding <- the CLS rows, conv1.weight <- dY^T . im2row(images) (no
        bias).  Once per step on [B*N, C]; the row bookkeeping is tensor code, the LayerNorm backward and the contraction are the kernels."""
        ops, cfg, P = self.ops, self.cfg, self.prefix
        C, M = cfg.width, B * N
        lvl2 = self.stem_level >= 2
        d_pre = ops.empty((M, C), F32)
        ops.layernorm_bwd(g.to(BF16), keep["x_pre"], self.p[P + "ln_pre.weight"], *keep["st"], d_pre, DX_F32_ASSIGN,
                          self.g[P + "ln_pre.weight"] if lvl2 else None, self.g[P + "ln_pre.bias"] if lvl2 else None, True, ws)
        d3 = d_pre.view(B, N, C)
        d_pos = d3.sum(dim=0)                                                    # [N, C]
        self._pos_grad(d_pos, grid)
        if lvl2:
            self.g[P + "class_embedding"].view(C).add_(d_pos[0])
            gp = d3[:, 1:, :].to(BF16).reshape(B * (N - 1), C)                   # patch rows, in the im2row matrix's row order
            self._wgrad(gp, keep["patches"], self.storage_of(self.grad, P + "conv1.weight"))
