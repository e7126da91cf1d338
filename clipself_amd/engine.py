"""Step engine of the EVA02 vision tower on the CLIPSelf hot path: an explicit forward / hand-written backward
schedule over the C-ABI kernels (clipself_amd/hip.py), with all parameters in flat buffers.

No tracing compiler and no autograd graph inside the tower: the schedule below *is* the program.  What each stage
computes, and where the reference does it (paths under /root/reference/src/open_clip/eva_clip/):

  stem            eva_vit_model.py:537-544   patch-embed conv (im2row + GEMM) + cls_token + pos_embed
  block           eva_vit_model.py:300-307   x += attn(norm1(x)); x += mlp(norm2(x))
  attention       eva_vit_model.py:174-247   q/k/v proj (+q_bias, none, +v_bias) -> RoPE(q,k) -> softmax(qk^T/8)v
                                              -> inner_attn_ln -> proj                 (rope.py:148-164)
  last dense blk  eva_vit_model.py:249-256,317-324   proj(inner_attn_ln(v_proj(norm1 x)+v_bias)), no attention
  SwiGLU          eva_vit_model.py:98-105    w3(ffn_ln(silu(w1 x) * (w2 x)))
  teacher head    eva_vit_model.py:565-569,585   head(norm(x)[:,0])
  dense head      eva_vit_model.py:615-623   normalize(head(norm(x[:,1:])))
  RoI pooling     eva_vit_model.py:625-629,655-664

Memory layout (MI355X: 288 GB HBM3E -- nothing is recomputed, nothing is re-laid-out):
  * one fp32 master buffer for every parameter of the tower, tensors back-to-back on 64-element boundaries, in
    layer order; [Wq;Wk;Wv], [q_bias;0;v_bias], [W1;W2], [b1;b2] are *adjacent* so the fused QKV / SwiGLU GEMMs read
    them as single matrices without any packing step;
  * a same-layout bf16 shadow (MFMA operand), and for the student same-layout fp32 grad / exp_avg / exp_avg_sq (one
    flat AdamW launch, one contiguous all-reduce bucket per block) plus transposed bf16 shadows for the dgrad GEMMs;
  * residual stream fp32 [B*N, C]; every GEMM operand bf16; LayerNorm / softmax statistics fp32.

The flat store, the trainable flags, the fold guard and the tower-level drivers (encode_image, encode_dense, backward_dense, AdamW) are
family-neutral and live in engine_base.TowerEngine, and so does the schedule code both families share (the CLS-only last block, the q|k|v
head of the folded teacher block, the head of the backward pass); this module holds what names EVA02 parameters: layout, stem, blocks, head,
fp8 operands.  The stacked matrices are read through one accessor (`_stacked`), a block's four linears are listed once (`_block_linears`),
and the block behind the attention core is written once (`_block_tail`).

The engine is backend-agnostic on purpose: `ops` is clipself_amd.hip.HipOps in the product; the CPU test-suite
injects the per-kernel references (oracle/ops_ref.py) to verify this schedule -- in particular the hand-written
backward -- against the monolithic autograd oracle without a GPU.  The product never constructs anything but HipOps.
"""
from __future__ import annotations

import math
import os

import torch

from .config import TowerCfg
from .engine_base import (ALIGN, BF16, DX_BF16, DX_F32_ACCUM, DX_F32_ASSIGN, EPI_ATOMIC_F32, EPI_BF16, EPI_F32, EPI_GELU_BF16,  # noqa: F401
                          EPI_PATCH_F32, EPI_QGELU_BF16, EPI_RESID_F32, EPI_RESID_LN_F32, EPI_SWIGLU_BF16, F32, TowerEngine, _round_up,
                          is_no_decay, padded_hidden)


def param_groups_layout(cfg: TowerCfg, prefix: str = "visual."):
    """Allocation groups (tensors of a group are contiguous, group starts are 64-aligned), in layer order.
    Entries are (name, logical shape, storage shape): names/logical shapes are the reference's state-dict entries; the
    storage of the SwiGLU hidden dimension and of the patch-embed contraction is zero-padded to a multiple of 64 so
    that every GEMM sees K % 64 == 0 and 16-byte rows (EVA02-L/14: hidden 2730 -> 2752, 3*14*14 = 588 -> 640; for
    B/16 both are already multiples of 64 and storage == logical).  Names containing '._' are private padding."""
    C, Hd, E, p = cfg.width, cfg.hidden, cfg.embed_dim, cfg.patch_size
    Hp, Kp = padded_hidden(cfg), _round_up(3 * p * p, 64)
    t = lambda name, shape, storage=None: (name, shape, storage if storage is not None else shape)
    groups = [[t(prefix + "cls_token", (1, 1, C))], [t(prefix + "pos_embed", (1, cfg.tokens, C))],
              [t(prefix + "patch_embed.proj.weight", (C, 3, p, p), (C, Kp))], [t(prefix + "patch_embed.proj.bias", (C,))]]
    for i in range(cfg.layers):
        b = f"{prefix}{EvaEngine.BLOCK_TAG}{i}."
        groups += [
            [t(b + "norm1.weight", (C,))], [t(b + "norm1.bias", (C,))],
            [t(b + "attn.q_proj.weight", (C, C)), t(b + "attn.k_proj.weight", (C, C)), t(b + "attn.v_proj.weight", (C, C))],
            [t(b + "attn.q_bias", (C,)), t(b + "attn._k_bias_zero", (C,)), t(b + "attn.v_bias", (C,))],
            [t(b + "attn.inner_attn_ln.weight", (C,))], [t(b + "attn.inner_attn_ln.bias", (C,))],
            [t(b + "attn.proj.weight", (C, C))], [t(b + "attn.proj.bias", (C,))],
            [t(b + "norm2.weight", (C,))], [t(b + "norm2.bias", (C,))],
            [t(b + "mlp.w1.weight", (Hd, C), (Hp, C)), t(b + "mlp.w2.weight", (Hd, C), (Hp, C))],
            [t(b + "mlp.w1.bias", (Hd,), (Hp,)), t(b + "mlp.w2.bias", (Hd,), (Hp,))],
            [t(b + "mlp.ffn_ln.weight", (Hd,), (Hp,))], [t(b + "mlp.ffn_ln.bias", (Hd,), (Hp,))],
            [t(b + "mlp.w3.weight", (C, Hd), (C, Hp))], [t(b + "mlp.w3.bias", (C,))],
        ]
    groups += [[t(prefix + "norm.weight", (C,))], [t(prefix + "norm.bias", (C,))],
               [t(prefix + "head.weight", (E, C))], [t(prefix + "head.bias", (E,))]]
    return groups


class EvaEngine(TowerEngine):
    BLOCK_TAG, NORM1, FINAL_NORM, RESID_BIAS = "blocks.", "norm1", "norm", "mlp.w3.bias"
    STACKED = {"attn.q_proj.weight": 3, "attn.q_bias": 3, "mlp.w1.weight": 2, "mlp.w1.bias": 2}      # first tensor of a stacked group: tensors in it (_stacked)
    FP8_MAX_ROW = 8192                        # widest row cs_quant_rows_fp8 quantises (one row per wave, held in registers)

    def _layout(self):
        return param_groups_layout(self.cfg, self.prefix)

    def _pos_table(self, views):
        return views[self.prefix + "pos_embed"][0]

    def _never_reached(self, i: int, name: str) -> bool:
        """Tensors of block i the dense path never differentiates.  The last block runs without attention, so its q/k projections
        and q_bias never get a gradient and torch's AdamW skips them (no decay either) -- SURVEY.md D7."""
        return i == self.cfg.layers - 1 and (name.rsplit(".", 2)[-2:] in (["q_proj", "weight"], ["k_proj", "weight"])
                                             or name.endswith("attn.q_bias"))

    def __init__(self, cfg: TowerCfg, ops, trainable: bool = False, prefix: str = "visual."):
        super().__init__(cfg, ops, trainable=trainable, prefix=prefix)
        # Frozen towers fold the two sub-LayerNorms (inner_attn_ln ahead of proj, ffn_ln ahead of w3) into the following GEMM:
        # gamma goes into a bf16 copy of the weight, beta and the row statistics into the GEMM epilogue, and the statistics
        # come out of the producing kernels' epilogues -- the LN passes over [M,C] and [M,hidden] disappear (_block_tail_folded).
        # fold_block_ln (norm1 / norm2 into the q|k|v and W1|W2 GEMMs, behind the guard) builds on it; the sub-LayerNorm folds themselves
        # are never worse than the plain schedule (their input is a stored bf16 tensor either way) and need no guard.
        self.fold_sub_ln = not trainable
        # BASELINE configs[4] "fp8 MFMA weights": the forward linears of the non-folded (training / dense) schedule run on e4m3 operands --
        # weight shadows quantised per output row (refreshed after every AdamW step), activations per token row by cs_quant_rows_fp8,
        # contraction by the block-scaled fp8 MFMA, fp32 accumulate; backward (dgrad / wgrad) keeps the bf16 operands.  enable_fp8_forward().
        self.fp8_forward = False
        self.w8 = {}
        # enable_fp8_forward(dgrad=True): the four dgrad GEMMs of a block (dX = dY . W) also contract e4m3 x e4m3 -- dY quantised per token
        # row, the transposed weight shadows per input-feature row, both scales factor out of the contraction over the output features;
        # wgrad (contraction over tokens: per-row scales do not factor out) stays bf16
        self.fp8_dgrad = False
        self.wt8 = {}
        # the SwiGLU backward also reduces its output's columns (the w1 | w2 bias gradients): bit-identical to the separate colsum pass
        # (A/B switch CLIPSELF_NO_FUSED_SWIGLU_COLSUM=1)
        self.fused_swiglu_colsum = os.environ.get("CLIPSELF_NO_FUSED_SWIGLU_COLSUM") != "1"

    # ------------------------------------------------------------------------------------------ hooks of the tower drivers
    def _wants_folds(self):
        return self.fold_sub_ln

    def _fold_pass(self, images):
        return self.fold_sub_ln and self.block_folds_active(images)      # (short-circuit: no lazy calibration without the sub-LN folds)

    def _lo_plane(self, last, cls_folded):
        return last > 0

    def _bwd_widths(self):
        return max(self.cfg.width, self.Hp), max(2 * self.Hp, 3 * self.cfg.width)

    def _bwd_gq(self, M):
        C = self.cfg.width
        return (self.ops.empty((M, _round_up(C, 128)), torch.uint8), self.ops.empty((M,), F32)) if self.fp8_dgrad and C <= 3072 else None

    def _head(self, rows, out):
        """out[M,E] f32 = bf16(rows) . head.weight^T + head.bias   (eva_vit_model.py:585,617)."""
        self.ops.gemm_nt(rows, self.w[self.prefix + "head.weight"], out, bias=self.p[self.prefix + "head.bias"], epi=EPI_F32)

    def _head_dgrad(self, d_feats, d_lnf):
        self.ops.gemm_nt(d_feats, self.wt["head"][:, :self.cfg.embed_dim], d_lnf, epi=EPI_BF16)

    def _head_wgrad(self, d_feats, lnf, ws):
        """bias = column sums, weight = dY^T . LN(x)   (eva_vit_model.py:616-617)."""
        self.ops.colsum_bf16(d_feats, self.g[self.prefix + "head.bias"], ws[1])
        self._wgrad(d_feats, lnf, self.g[self.prefix + "head.weight"])

    # ------------------------------------------------------------------------------------------ derived operands
    def sync_shadow(self):
        super().sync_shadow()
        if self.fp8_forward:
            self.sync_fp8()

    def _build_folds(self):
        """gamma (.) W in bf16, its row sums, and W.beta + b for proj and w3 of every block (one-time, after a weight load)."""
        cfg, C, Hl = self.cfg, self.cfg.width, self.cfg.hidden
        self.fold = {}
        with torch.no_grad():
            for i in range(cfg.layers):
                b = self._b(i)
                out = {}
                for key, wname, ln, bname, K in (("proj", "attn.proj.weight", "attn.inner_attn_ln", "attn.proj.bias", C),
                                                 ("w3", "mlp.w3.weight", "mlp.ffn_ln", "mlp.w3.bias", Hl)):
                    W = self.storage_of(self.master, b + wname)                    # [C, K padded]
                    g, beta = self.p[b + ln + ".weight"][:K], self.p[b + ln + ".bias"][:K]
                    Wf = torch.zeros_like(W, dtype=BF16)
                    Wf[:, :K] = (W[:, :K] * g[None, :]).to(BF16)
                    out[key] = (Wf, Wf.float().sum(dim=1).contiguous(), (W[:, :K] @ beta + self.p[b + bname]).contiguous())
                if self.fold_block_ln:
                    # norm1 -> [Wq;Wk;Wv] and norm2 -> [W1;W2]: the stacked matrices and biases are adjacent in the flat store
                    for key, wname, bias_name, ln in (("qkv", "attn.q_proj.weight", "attn.q_bias", "norm1"),
                                                     ("w12", "mlp.w1.weight", "mlp.w1.bias", "norm2")):
                        W, bias = self._stacked(self.master, wname, i), self._stacked(self.master, bias_name, i)
                        g, beta = self.p[b + ln + ".weight"], self.p[b + ln + ".bias"]
                        Wf = (W * g[None, :]).to(BF16).contiguous()
                        out[key] = (Wf, Wf.float().sum(dim=1).contiguous(), (W @ beta + bias).contiguous())
                self.fold[i] = out

    def sync_transposed(self, blocks=None):
        """W^T shadows for the dgrad GEMMs (dx = dy . W needs W with the contraction dimension contiguous)."""
        pairs = self._block_wt_pairs(blocks)
        pairs.append((self.w[self.prefix + "head.weight"], self._wt_alloc("head", self.cfg.embed_dim, self.cfg.width)))
        self.ops.transpose_bf16_batched(pairs)          # one launch (49 matrices per step for B/16)

    # ------------------------------------------------------------------------------------------ fp8 forward operands
    def _fp8_rows(self, X):
        """bf16 [M,K] -> (e4m3 bytes [M, K padded to 128], fp32 row scales [M])."""
        M, K = X.shape
        q = self.ops.empty((M, _round_up(K, 128)), torch.uint8)
        sc = self.ops.empty((M,), F32)
        self.ops.quant_rows_fp8(X, q, sc)
        return q, sc

    def sync_fp8(self, blocks=None):
        """e4m3 shadows (+ per-output-row scales) of the four weight matrices of every block, from the bf16 shadows."""
        for i in (range(self.cfg.layers) if blocks is None else blocks):
            linears = self._block_linears(i)
            for key, W in linears:
                self.w8[(i, key)] = self._fp8_rows(W)
            if self.fp8_dgrad and i >= self.first_trainable:
                for key, W in linears:                     # ... and of their W^T shadows (the columns past W's row count are padding)
                    self.wt8[(i, key)] = self._fp8_rows(self.wt[(i, key)][:, :W.shape[0]])

    def _dgrad(self, i, key, dY, out, cols=None, q=None):
        """out (bf16) = dY . W for the linear `key` of block i, through the transposed shadow (contraction over the output features, or over
        the column range `cols` of them); with fp8_dgrad on e4m3 operands."""
        n = dY.shape[1]
        lo, hi = cols if cols is not None else (0, n)
        if not self.fp8_dgrad or lo % 128 or (hi - lo) % 8:
            self.ops.gemm_nt(dY, self.wt[(i, key)][:, lo:hi], out, epi=EPI_BF16)
            return
        q, sy = q if q is not None else self._fp8_rows(dY)            # q: (codes, scales) already produced by the kernel that wrote dY
        w8, sw = self.wt8[(i, key)]
        self.ops.gemm_nt_f8(q, w8[:, lo:lo + q.shape[1]], out, sy, sw, epi=EPI_BF16)

    def enable_fp8_forward(self, on: bool = True, dgrad: bool = False):
        if on and not self.trainable:
            raise RuntimeError("fp8 forward operands belong to the training schedule; a frozen tower keeps its bf16 operands "
                               "(teacher targets and evaluation features must not depend on the run's precision flag)")
        widest = max(self.cfg.width, self.Hp) if not dgrad else max(3 * self.cfg.width, 2 * self.Hp)
        if on and widest > self.FP8_MAX_ROW:
            raise NotImplementedError(f"amp_fp8: cs_quant_rows_fp8 keeps a row in registers and covers rows up to {self.FP8_MAX_ROW} wide; "
                                      f"this tower's widest GEMM operand is {widest}")
        self.fp8_forward = bool(on)
        self.fp8_dgrad = bool(on and dgrad)
        self.w8, self.wt8 = {}, {}
        if on:
            self.sync_fp8()

    def _ln(self, x, gamma, beta, y, mean, rstd, eps):
        """LayerNorm forward; under fp8_forward also the e4m3 copy of its output (cs_layernorm_fwd_q8) for the linear that consumes it.
        Returns (q8, scale) or None."""
        if not self.fp8_forward:
            self.ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, eps)
            return None
        M = x.shape[0]
        q = self.ops.empty((M, _round_up(y.shape[1], 128)), torch.uint8)
        sc = self.ops.empty((M,), F32)
        self.ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, eps, q8=q, q_scale=sc)
        return q, sc

    def _linear(self, i, key, X, W, out, bias, extra=None, epi=EPI_BF16, rows=None, xq=None):
        """out = X . W^T + bias (+ extra): the bf16 MFMA GEMM, or -- fp8_forward -- the e4m3 GEMM on the quantised copy of X (xq: already
        produced by the LayerNorm that wrote X) and the weight's e4m3 shadow (`rows` = row range of the stacked weight that W is a slice of)."""
        if not self.fp8_forward:
            self.ops.gemm_nt(X, W, out, bias=bias, extra=extra, epi=epi)
            return
        xq, sx = xq if xq is not None else self._fp8_rows(X)
        w8, sw = self.w8[(i, key)]
        if rows is not None:
            w8, sw = w8[rows[0]:rows[1]], sw[rows[0]:rows[1]]
        self.ops.gemm_nt_f8(xq, w8, out, sx, sw, bias=bias, extra=extra, epi=epi)

    def _set_flags(self):
        super()._set_flags()
        if self.trainable:                      # the e4m3 W^T shadows follow the bf16 ones: frozen blocks drop theirs, training ones get them
            for key in [k for k in self.wt8 if k[0] < self.first_trainable]:
                del self.wt8[key]
            if self.fp8_forward and self.fp8_dgrad:
                self.sync_fp8(range(self.first_trainable, self.cfg.layers))

    def adamw_step(self, *args, **kw):
        super().adamw_step(*args, **kw)
        if self.fp8_forward:
            self.sync_fp8(range(self.first_trainable, self.cfg.layers))

    # ------------------------------------------------------------------------------------------ tables
    def rope_tables(self, grid: int):
        """cos/sin [grid*grid, 64] (rope.py:118-142,179-214): 16 frequencies theta^(-2i/32), positions
        arange(grid)/grid*pt_seq_len, each repeated twice, row block then column block."""
        key = ("rope", grid)
        if key not in self._tables:
            half = self.cfg.head_width // 2
            freqs = 1.0 / (10000.0 ** (torch.arange(0, half, 2)[: half // 2].float() / half))
            t = torch.arange(grid).float() / grid * self.cfg.pt_hw_seq_len
            ang = (t[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
            full = torch.cat([ang[:, None, :].expand(grid, grid, half), ang[None, :, :].expand(grid, grid, half)], dim=-1)
            full = full.reshape(grid * grid, self.cfg.head_width)
            self._tables[key] = (full.cos().contiguous().to(self.device), full.sin().contiguous().to(self.device))
        return self._tables[key]

    # ------------------------------------------------------------------------------------------ forward pieces
    def _stem(self, images, keep=None):
        ops, cfg, P = self.ops, self.cfg, self.prefix
        B, _, S, _ = images.shape
        p, C = cfg.patch_size, cfg.width
        g = S // p
        N, Kpe = g * g + 1, self.Kpe                       # contraction zero-padded to a multiple of 64 (3*14*14 -> 640)
        A = ops.empty((B * g * g, Kpe), BF16)
        ops.im2row(images.contiguous(), A, p)              # writes the zero padding columns too
        x = ops.empty((B, N, C), F32)
        pos = self.pos_for(g)
        ops.gemm_nt(A, self.storage_of(self.shadow, P + "patch_embed.proj.weight"), x.view(B * N, C),
                    bias=self.p[P + "patch_embed.proj.bias"], extra=pos, epi=EPI_PATCH_F32, group=g * g)
        ops.cls_row(x, self.p[P + "cls_token"].view(C), pos)
        if keep is not None:
            keep["patches"] = A                  # operand of the patch-embedding weight gradient
        return x, g

    def _stacked(self, buf, name, i):
        """A stacked group of block i inside a flat buffer (master, shadow, grad) as ONE matrix / vector -- [Wq;Wk;Wv] [3C, C],
        [q_bias;0;v_bias] [3C], [W1;W2] [2 Hp, C], [b1;b2] [2 Hp] --, named by its first tensor: the group's tensors have one storage shape
        and are adjacent in the flat store (param_groups_layout)."""
        o, st = self.offsets[self._b(i) + name]
        n = self.STACKED[name]
        return buf[o:o + n * math.prod(st)].view(n * st[0], *st[1:])

    def _qkv_operands(self, i):
        return self._stacked(self.shadow, "attn.q_proj.weight", i), self._stacked(self.master, "attn.q_bias", i)

    def _w12(self, i):
        return self._stacked(self.shadow, "mlp.w1.weight", i), self._stacked(self.master, "mlp.w1.bias", i)

    def _block_linears(self, i):
        b = self._b(i)
        return (("qkv", self._stacked(self.shadow, "attn.q_proj.weight", i)), ("proj", self.w[b + "attn.proj.weight"]),
                ("w12", self._stacked(self.shadow, "mlp.w1.weight", i)), ("w3", self.storage_of(self.shadow, b + "mlp.w3.weight")))

    def _block_fwd(self, i, x, B, N, cos, sin, with_attn=True, save=None, inplace=True):
        """x: fp32 [B*N, C].  Returns the block output (x itself when inplace)."""
        ops, cfg = self.ops, self.cfg
        C, H, eps = cfg.width, cfg.heads, cfg.ln_eps
        b = self._b(i)
        M = B * N
        keep = save is not None

        ln1 = ops.empty((M, C), BF16)
        m1, r1 = self._row_stats(M, keep)
        q1 = self._ln(x, self.p[b + "norm1.weight"], self.p[b + "norm1.bias"], ln1, m1, r1, eps)
        wqkv, bqkv = self._qkv_operands(i)
        qkv = lse = None
        if with_attn and not keep and inplace and self.fold_sub_ln:
            qkv = ops.empty((M, 3 * C), BF16)
            ops.gemm_nt(ln1, wqkv, qkv, bias=bqkv, epi=EPI_BF16)
            att = ops.empty((M, C), BF16)
            part = ops.empty((H, M, 2), F32)
            ops.attn_fwd_stats(qkv, cos, sin, att, None, part, B, N, H, cfg.head_width ** -0.5)
            return self._block_tail_folded(i, x, att, part)
        if with_attn:
            qkv = ops.empty((M, 3 * C), BF16)
            self._linear(i, "qkv", ln1, wqkv, qkv, bqkv, xq=q1)
            att = ops.empty((M, C), BF16)
            lse = ops.empty((B * H, N), F32) if keep else None
            ops.attn_fwd(qkv, cos, sin, att, lse, B, N, H, cfg.head_width ** -0.5)
        else:
            att = ops.empty((M, C), BF16)      # v only: every token "attends" to itself (proj_without_attn)
            self._linear(i, "qkv", ln1, wqkv[2 * C:], att, bqkv[2 * C:], rows=(2 * C, 3 * C), xq=q1)
        x2 = self._block_tail(i, x, att, save, inplace)
        if keep:
            save.update(x0=x, ln1=ln1, st1=(m1, r1), qkv=qkv, lse=lse, att=att, with_attn=with_attn)
        return x2

    def _block_tail(self, i, x, att, save=None, inplace=True):
        """Everything after the attention core, for whichever rows x fp32 [M, C] / att bf16 [M, C] hold: inner_attn_ln -> proj (+x) -> norm2 ->
        SwiGLU -> ffn_ln -> w3 (+x1).  inplace: x1 and x2 are x itself; save (dict): what _block_bwd needs is kept and put into it."""
        ops, cfg = self.ops, self.cfg
        C, Hd, Hl, eps = cfg.width, self.Hp, cfg.hidden, cfg.ln_eps      # Hd: padded storage width, Hl: logical
        b, M = self._b(i), x.shape[0]
        keep = save is not None
        iln = ops.empty((M, C), BF16)
        m2, r2 = self._row_stats(M, keep)
        q2 = self._ln(att, self.p[b + "attn.inner_attn_ln.weight"], self.p[b + "attn.inner_attn_ln.bias"], iln, m2, r2, eps)
        x1 = x if inplace else ops.empty((M, C), F32)
        self._linear(i, "proj", iln, self.w[b + "attn.proj.weight"], x1, self.p[b + "attn.proj.bias"], extra=x, epi=EPI_RESID_F32, xq=q2)

        ln2 = ops.empty((M, C), BF16)
        m3, r3 = self._row_stats(M, keep)
        q3 = self._ln(x1, self.p[b + "norm2.weight"], self.p[b + "norm2.bias"], ln2, m3, r3, eps)
        w12, b12 = self._w12(i)
        hid = ops.empty((M, Hd), BF16)
        x12 = None
        if keep or self.fp8_forward:
            x12 = ops.empty((M, 2 * Hd), BF16)
            # (a W1|W2 epilogue that stores x1 | x2 AND silu(x1) * x2 was built and measured in round 4: 129.8 us against 112.3 us for GEMM +
            # cs_swiglu_fwd at 12 608 rows -- the un-overlapped epilogue costs more than the HBM-rate elementwise pass it replaces)
            self._linear(i, "w12", ln2, w12, x12, b12, xq=q3)
            ops.swiglu_fwd(x12, hid)
        else:
            ops.gemm_nt(ln2, w12, hid, bias=b12, epi=EPI_SWIGLU_BF16, group=Hd)
        fln = (ops.zeros if Hd != Hl else ops.empty)((M, Hd), BF16)   # padding columns feed the W3 GEMM: must be exact zeros
        m4, r4 = self._row_stats(M, keep)
        q4 = self._ln(hid[:, :Hl], self.p[b + "mlp.ffn_ln.weight"], self.p[b + "mlp.ffn_ln.bias"], fln[:, :Hl], m4, r4, eps)
        x2 = x1 if inplace else ops.empty((M, C), F32)
        self._linear(i, "w3", fln, self.storage_of(self.shadow, b + "mlp.w3.weight"), x2, self.p[b + "mlp.w3.bias"], extra=x1,
                     epi=EPI_RESID_F32, xq=q4)
        if keep:
            save.update(iln=iln, st2=(m2, r2), x1=x1, ln2=ln2, st3=(m3, r3), x12=x12, hid=hid, fln=fln, st4=(m4, r4))
        return x2

    def _block_tail_folded(self, i, x, att, att_part):
        """_block_tail for a frozen tower with both sub-LayerNorms folded into proj / w3 (in place on x)."""
        ops, cfg = self.ops, self.cfg
        C, Hd, Hl, eps = cfg.width, self.Hp, cfg.hidden, cfg.ln_eps
        b, M = self._b(i), x.shape[0]
        f = self.fold[i]
        mean, rstd = ops.empty((M,), F32), ops.empty((M,), F32)
        ops.ln_stats_finalize(att_part, 64, C, mean, rstd, eps)
        Wp, cp, dp = f["proj"]
        ops.gemm_nt_ln(att, Wp, x, bias=dp, extra=x, ln_mean=mean, ln_rstd=rstd, ln_colsum=cp, epi=EPI_RESID_LN_F32)

        ln2 = ops.empty((M, C), BF16)
        ops.layernorm_fwd(x, self.p[b + "norm2.weight"], self.p[b + "norm2.bias"], ln2, None, None, eps)
        w12, b12 = self._w12(i)
        hid = ops.empty((M, Hd), BF16)
        part = ops.empty((4 * ((Hd + 127) // 128), M, 2), F32)
        ops.gemm_nt_ln(ln2, w12, hid, bias=b12, stats_part=part, epi=EPI_SWIGLU_BF16, group=Hd)
        ops.ln_stats_finalize(part, 32, Hl, mean, rstd, eps)
        W3, c3, d3 = f["w3"]
        ops.gemm_nt_ln(hid, W3, x, bias=d3, extra=x, ln_mean=mean, ln_rstd=rstd, ln_colsum=c3, epi=EPI_RESID_LN_F32)
        return x

    def _teacher_block_folded(self, i, x, xb, st, B, N, cos, sin, emit_next, lo=None):
        """One frozen-tower block with all four LayerNorms folded into the GEMMs (in place on x).  xb / st = bf16 copy and (mean, rstd)
        of x for norm1 as left by the previous block's w3 GEMM, or None (first block: plain norm1 kernel).  Returns (xb, st) for the
        next block when emit_next.  With lo (int16 [M, C]) the stream lives in the planes (xb, lo) between the first residual GEMM of the
        tower, which reads fp32 x, and the last one (emit_next False), which writes fp32 x again (cs_gemm_nt_ln_split)."""
        ops, cfg = self.ops, self.cfg
        C, Hd, Hl, H, eps = cfg.width, self.Hp, cfg.hidden, cfg.heads, cfg.ln_eps
        M = B * N
        f = self.fold[i]
        first = xb is None
        qkv = self._teacher_qkv(i, x, xb, st, M)
        att = ops.empty((M, C), BF16)
        part_a = ops.empty((H, M, 2), F32)
        ops.attn_fwd_stats(qkv, cos, sin, att, None, part_a, B, N, H, cfg.head_width ** -0.5)
        mean, rstd = ops.empty((M,), F32), ops.empty((M,), F32)
        ops.ln_stats_finalize(part_a, 64, C, mean, rstd, eps)
        Wp, cp, dp = f["proj"]
        part_x = ops.empty(((C + 63) // 64, M, 2), F32)
        xb2 = xb if (lo is not None and not first) else ops.empty((M, C), BF16)
        self._resid_gemm_folded(att, Wp, dp, (mean, rstd, cp), x, xb2, lo, part_x, first=first)
        mean2, rstd2 = ops.empty((M,), F32), ops.empty((M,), F32)
        ops.ln_stats_finalize(part_x, 64, C, mean2, rstd2, eps)
        W12, c12, d12 = f["w12"]
        hid = ops.empty((M, Hd), BF16)
        part_h = ops.empty((4 * ((Hd + 127) // 128), M, 2), F32)
        ops.gemm_nt_ln(xb2, W12, hid, bias=d12, ln_mean=mean2, ln_rstd=rstd2, ln_colsum=c12, stats_part=part_h, epi=EPI_SWIGLU_BF16,
                       group=Hd)
        ops.ln_stats_finalize(part_h, 32, Hl, mean, rstd, eps)
        W3, c3, d3 = f["w3"]
        self._resid_gemm_folded(hid, W3, d3, (mean, rstd, c3), x, xb2, lo, part_x, last=not emit_next)
        if not emit_next:
            return None, None
        ops.ln_stats_finalize(part_x, 64, C, mean2, rstd2, eps)
        return xb2, (mean2, rstd2)

    # ------------------------------------------------------------------------------------------ backward
    def _block_bwd(self, i, s, g, gb, B, N, cos, sin, ws, next_bias=None, gq=None):
        """g: fp32 [M,C] gradient w.r.t. the block output; updated in place to the gradient w.r.t. its input.  gb: its bf16 copy, already
        summed into this block's w3 bias gradient by the LayerNorm backward that produced it (the final norm's, or norm1's of block i+1);
        on return gb is the copy of the new g and its column sums have gone to `next_bias` (block i-1's w3 bias gradient, or None).
        gq (fp8_dgrad): (e4m3 codes, row scales) of gb, written by the same LayerNorm backwards (cs_layernorm_bwd_q8)."""
        q8a = dict(q8=gq[0], q_scale=gq[1]) if gq is not None else {}
        ops, cfg = self.ops, self.cfg
        C, Hd, Hl, H = cfg.width, self.Hp, cfg.hidden, cfg.heads
        b = self._b(i)
        M = B * N
        G = self.g
        # ---- MLP: x2 = x1 + w3(ffn_ln(silu(x1')*x2')) ------------------------------------------
        self._wgrad(gb, s["fln"], self.storage_of(self.grad, b + "mlp.w3.weight"))
        d_fln = ops.empty((M, Hd), BF16)
        self._dgrad(i, "w3", gb, d_fln, q=gq)                                               # [M,C] . W3[C,Hd]
        d_hid = (ops.zeros if Hd != Hl else ops.empty)((M, Hd), BF16)
        ops.layernorm_bwd(d_fln[:, :Hl], s["hid"][:, :Hl], self.p[b + "mlp.ffn_ln.weight"], *s["st4"], d_hid[:, :Hl], DX_BF16,
                          G[b + "mlp.ffn_ln.weight"], G[b + "mlp.ffn_ln.bias"], True, ws[0])
        d_x12 = ops.empty((M, 2 * Hd), BF16)
        g12b = self._stacked(self.grad, "mlp.w1.bias", i)
        q12 = None
        if self.fp8_dgrad and Hd <= 4096:
            q12 = (ops.empty((M, _round_up(2 * Hd, 128)), torch.uint8), ops.empty((M,), F32))
            ops.swiglu_bwd(d_hid, s["x12"], d_x12, q8=q12[0], q_scale=q12[1])
            ops.colsum_bf16(d_x12, g12b, ws[1])
        elif self.fused_swiglu_colsum:
            ops.swiglu_bwd_colsum(d_hid, s["x12"], d_x12, g12b, ws[1])      # d x1|x2 and the w1 | w2 bias gradients in one pass
        else:
            ops.swiglu_bwd(d_hid, s["x12"], d_x12)
            ops.colsum_bf16(d_x12, g12b, ws[1])
        self._wgrad(d_x12, s["ln2"], self._stacked(self.grad, "mlp.w1.weight", i))
        d_ln2 = ops.empty((M, C), BF16)
        self._dgrad(i, "w12", d_x12, d_ln2, q=q12)                                          # [M,2Hd] . W12[2Hd,C]
        # norm2's backward adds into the stream gradient and hands back its bf16 copy + column sums (= the proj bias gradient)
        ops.layernorm_bwd(d_ln2, s["x1"], self.p[b + "norm2.weight"], *s["st3"], g, DX_F32_ACCUM,
                          G[b + "norm2.weight"], G[b + "norm2.bias"], True, ws[0], dx_copy=gb, copy_colsum=G[b + "attn.proj.bias"], **q8a)
        # ---- attention branch: x1 = x0 + proj(inner_ln(att)) -------------------------------------
        self._wgrad(gb, s["iln"], G[b + "attn.proj.weight"])
        d_iln = ops.empty((M, C), BF16)
        self._dgrad(i, "proj", gb, d_iln, q=gq)
        d_att = ops.empty((M, C), BF16)
        ops.layernorm_bwd(d_iln, s["att"], self.p[b + "attn.inner_attn_ln.weight"], *s["st2"], d_att, DX_BF16,
                          G[b + "attn.inner_attn_ln.weight"], G[b + "attn.inner_attn_ln.bias"], True, ws[0])
        d_ln1 = ops.empty((M, C), BF16)
        if s["with_attn"]:
            d_qkv = ops.empty((M, 3 * C), BF16)
            ops.attn_bwd(s["qkv"], s["att"], d_att, s["lse"], cos, sin, d_qkv, ws[0], B, N, H, cfg.head_width ** -0.5)
            # one pass over d_q|d_k|d_v into the adjacent [q_bias; (k: no bias, eva_vit_model.py:178); v_bias] gradient slots; the middle slot
            # belongs to no parameter and goes back to zero (the flat gradient's norm must be the parameters' gradient norm)
            gqb = self._stacked(self.grad, "attn.q_bias", i)
            ops.colsum_bf16(d_qkv, gqb, ws[1])
            gqb[C:2 * C].zero_()
            self._wgrad(d_qkv, s["ln1"], self._stacked(self.grad, "attn.q_proj.weight", i))
            self._dgrad(i, "qkv", d_qkv, d_ln1)
        else:
            ops.colsum_bf16(d_att, G[b + "attn.v_bias"], ws[1])
            self._wgrad(d_att, s["ln1"], G[b + "attn.v_proj.weight"])
            self._dgrad(i, "qkv", d_att, d_ln1, cols=(2 * C, 3 * C))
        ops.layernorm_bwd(d_ln1, s["x0"], self.p[b + "norm1.weight"], *s["st1"], g, DX_F32_ACCUM,
                          G[b + "norm1.weight"], G[b + "norm1.bias"], True, ws[0], dx_copy=gb if next_bias is not None else None,
                          copy_colsum=next_bias, **(q8a if next_bias is not None else {}))

    def _stem_bwd(self, g, keep, B, N, grid, ws):
        """Gradients of the stem from g = d loss / d (stem output) fp32 [B*N, C]  (eva_vit_model.py:537-544: x = cat(cls, conv(img)) + pos):
        pos_embed <- sum over images (_pos_grad), cls_token <- the CLS rows, patch_embed.proj <- bias = column sums of the patch rows,
        weight = dY^T . im2row(images).  Runs once per step on [B*N, C] tensors; the row bookkeeping (dropping the CLS rows, the sum over
        images) is plain tensor code, the contraction is the wgrad kernel."""
        ops, cfg, P = self.ops, self.cfg, self.prefix
        C = cfg.width
        g3 = g.view(B, N, C)
        d_pos = g3.sum(dim=0)                                                   # [N, C]
        self.g[P + "cls_token"].view(C).add_(d_pos[0])
        self._pos_grad(d_pos, grid)
        gp = g3[:, 1:, :].to(BF16).reshape(B * (N - 1), C)                      # patch rows, in the im2row matrix's row order
        ops.colsum_bf16(gp, self.g[P + "patch_embed.proj.bias"])          # (allocates its own row-block workspace: once per step)
        self._wgrad(gp, keep["patches"], self.storage_of(self.grad, P + "patch_embed.proj.weight"))
