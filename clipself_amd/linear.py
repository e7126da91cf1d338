"""The box head's fully connected layers, Linear (+ ReLU), as GEMMs on channel-last RoI rows (include/clipself_hip.h).

`nn.Linear(in, out)` followed by ReLU on bf16 rows X [rows, in] is one call of cs_gemm_nt with the ReLU epilogue (EPI_RELU_BF16):
Y = relu(X . Wp^T + bias), rounded once to bf16.  The first FC of the head contracts the whole RoI map (in = C * P = 256 * 49 against 512
outputs): few output tiles with a long contraction behind each, which the deterministic split-K form of that call serves (`splits`).

`spatial=(C, P)` is mmdet's `x.flatten(1)` without moving data: the channel-last map [K, C, h, w] of the convolutions in front is the
rows [K*P, C] = [K, P*C], and the weights are packed once as  Wp[o, p*C + c] = weight[o, c*P + p].  The backward is the same family:

  dZ   dY where the saved Y > 0, else 0, cast to bf16 -- the one pointwise op left to torch (on [rows, out], at most 4 MB in the head);
  dX = dZ . Wp        cs_gemm_nt(dZ, WpT), in x's dtype; with `spatial` returned as the channel-last map;
  dW = dZ^T . X       cs_gemm_wgrad_tn; with `spatial` permuted back from (p, c) to (c, p) order (a torch permute of [out, P, C] fp32);
  db                  a column sum of dZ (cs_colsum_bf16).

No atomics: equal inputs give equal bits.  Operands are bf16, accumulation is fp32, parameter gradients are fp32.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .det_layer import BF16, EPI_BF16, EPI_RELU_BF16, F32, KernelLayer, bias_f32, epi_for, packed, pad_cols, rows2d, rows_bf16, wgrad

ACTS = {None: EPI_BF16, "relu": EPI_RELU_BF16}

# Whether fused=None takes the kernels where the backend has them: set from profiles/fc_bench.md by the rule of FUSED_CONV_DEFAULT -- on only
# if the kernel route wins forward + backward against the faster torch variant (fp32, or bf16 autocast) at the training shape
# (4096 x 12544 x 512).  It does: 270 us against 498 us under bf16 autocast (the faster one) and 1575 us in fp32, the form the detector runs;
# the whole ConvFCBBoxHead forward + backward takes 6.9 ms against 8.2 ms with torch's FCs behind the same convolutions.
FUSED_FC_DEFAULT = True


def pack_weights(weight, spatial=None):
    """(Wp bf16 [out, in], WpT bf16 [in, out rounded up to 64]) of a [out, in] weight.  With spatial=(C, P):
    Wp[o, p*C + c] = weight[o, c*P + p], the order of channel-last rows.  WpT[i, o] = Wp[o, i] is the dgrad's B operand; its zero columns
    pad the contraction to cs_gemm_nt's K tile."""
    out, inf = weight.shape
    wb = weight.detach().to(BF16)
    if spatial is not None:
        C, P = spatial
        wb = wb.view(out, C, P).permute(0, 2, 1).reshape(out, P * C)
    Wp = wb.contiguous()
    outp = (out + 63) // 64 * 64
    WpT = Wp.new_zeros(inf, outp)
    WpT[:, :out] = Wp.t()
    return Wp, WpT


def relu_gate(Y, dY):
    """dZ bf16 = dY where the saved output Y > 0, else 0: the ReLU's gate rides on the cast to bf16 that the gradient needs anyway.  The
    mask comes from the layer's own output, never from dY."""
    return torch.where(Y > 0, dY, torch.zeros((), dtype=dY.dtype, device=dY.device)).to(BF16)


def unpack_wgrad(dWp, spatial=None):
    """The packed weight gradient [out, in] in nn.Linear's layout: with spatial=(C, P) permuted back from (p, c) to (c, p) order."""
    if spatial is None:
        return dWp
    C, P = spatial
    return dWp.view(dWp.shape[0], P, C).permute(0, 2, 1).reshape(dWp.shape[0], C * P)


class LinearAct(KernelLayer, nn.Linear):
    """nn.Linear(in_features, out_features) -- its parameters, names, initialisation and state dict -- followed by `act` (None or "relu"),
    whose forward and backward run on the HIP kernels when the tensors live on a backend with LINEAR_ACT, in_features % 64 == 0 and
    out_features % 8 == 0 (what cs_gemm_nt and cs_gemm_wgrad_tn take); F.linear (+ F.relu) otherwise.

    spatial: (C, P) makes the layer take the 4-D map [K, C, h, w] with h*w == P and compute nn.Linear(x.flatten(1)).
    fused:   True = the kernels or NotImplementedError, False = torch, None = FUSED_FC_DEFAULT where the kernels can run.
    splits:  K slices of the forward GEMM; None = chosen by the library, an integer forces it (the benchmark, the tests).
    forward(x): x [..., in_features] (or the map) fp32 / bf16 -> [..., out_features] of x's dtype; on the kernel route the values are bf16's."""
    FLAG = "LINEAR_ACT"
    COVERAGE = "in % 64 == 0, out % 8 == 0, fp32 parameters, fp32 / bf16 input"

    def __init__(self, in_features, out_features, bias=True, act=None, spatial=None, ops=None, fused=None, splits=None, **kw):
        super().__init__(in_features, out_features, bias=bias, **kw)
        assert act in ACTS, f"act is None or 'relu', got {act!r}"
        assert spatial is None or (len(spatial) == 2 and spatial[0] * spatial[1] == in_features), \
            f"spatial=(C, P) needs C * P == in_features, got {spatial} for {in_features}"
        assert splits is None or splits >= 1, splits
        self.act = act
        self.spatial = None if spatial is None else (int(spatial[0]), int(spatial[1]))
        self.ops = ops
        self.fused = fused
        self.splits = splits

    def extra_repr(self):
        return super().extra_repr() + f", act={self.act}, spatial={self.spatial}"

    # ------------------------------------------------------------------------------------------ dispatch
    def covered(self, x) -> bool:
        """What the kernels cover: fp32 parameters, an fp32 / bf16 input of the layer's shape, in % 64 == 0, out % 8 == 0."""
        if self.spatial is None:
            shape_ok = x.dim() >= 1 and x.shape[-1] == self.in_features
        else:
            shape_ok = x.dim() == 4 and x.shape[1] == self.spatial[0] and x.shape[2] * x.shape[3] == self.spatial[1]
        return (self.in_features % 64 == 0 and self.out_features % 8 == 0 and self.weight.dtype == F32 and x.dtype in (F32, BF16)
                and shape_ok and x.numel() > 0 and x.device == self.weight.device)

    def describe(self):
        return f"LinearAct({self.in_features}, {self.out_features}, spatial={self.spatial})"

    def fused_default(self):
        return FUSED_FC_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            y = F.linear(x.flatten(1) if self.spatial is not None else x, self.weight, self.bias)
            return F.relu(y) if self.act == "relu" else y
        return _LinearActFn.apply(x, self.weight, self.bias, self, k)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(Wp bf16 [out, in], WpT bf16 [in, out rounded up to 64], bias fp32 [out] | None), see pack_weights.  Rebuilt when the parameters'
        version counters (or their storage) change."""
        return packed(self, lambda: (*pack_weights(self.weight, self.spatial), bias_f32(self.bias)))

    def _splitk_ws(self, ops, M, N, K):
        """(splits argument, fp32 workspace | None) of the forward GEMM: the module's own grow-only buffer of splits * M * N floats."""
        s = self.splits if self.splits is not None else ops.gemm_nt_splits(M, N, K)
        if s <= 1:
            return 1, None
        ws = self.__dict__.get("_splitk_buf")
        if ws is None or ws.numel() < s * M * N or ws.device != self.weight.device:
            ws = self.__dict__["_splitk_buf"] = ops.empty((s * M * N,), F32)
        return (0 if self.splits is None else s), ws


class _LinearActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops):
        inf, out = mod.in_features, mod.out_features
        Wp, _, b32 = mod.gemm_weights()
        if mod.spatial is not None:
            X = rows_bf16(ops, x).reshape(x.shape[0], inf)             # [K*P, C] seen as [K, P*C]: no data moves for a channel-last bf16 map
        else:
            X = rows2d(ops, x, inf)
        rows = X.shape[0]
        Y = ops.empty((rows, out), BF16)
        splits, ws = mod._splitk_ws(ops, rows, out, inf)
        ops.gemm_nt(X, Wp, Y, b32, extra=ws, epi=ACTS[mod.act], splits=splits)
        ctx.mod, ctx.ops, ctx.x_shape, ctx.x_dtype, ctx.has_bias = mod, ops, tuple(x.shape), x.dtype, bias is not None
        ctx.save_for_backward(X, Y)
        y = Y if x.dtype == BF16 else Y.to(x.dtype)
        return y.view(rows, out) if mod.spatial is not None else y.view(*x.shape[:-1], out)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops = ctx.mod, ctx.ops
        inf, out = mod.in_features, mod.out_features
        X, Y = ctx.saved_tensors
        rows = X.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        dY = d_out.reshape(rows, out)
        dZ = relu_gate(Y, dY) if mod.act == "relu" else dY.to(BF16)
        dZp = pad_cols(ops, dZ)                                        # zero columns pad the dgrad's contraction to the K tile
        if dZp is dZ:
            dZp = dZ = dZ.contiguous()
        else:
            dZ = dZp[:, :out]
        dx = dw = db = None
        if need_x:
            _, WpT, _ = mod.gemm_weights()
            dX = ops.empty((rows, inf), ctx.x_dtype)
            ops.gemm_nt(dZp, WpT, dX, None, epi=epi_for(ctx.x_dtype))
            if mod.spatial is not None:
                K, C, h, w = ctx.x_shape
                dx = dX.view(K, h, w, C).permute(0, 3, 1, 2)             # the channel-last map: the batch norm in front takes it in place
            else:
                dx = dX.view(ctx.x_shape)
        if need_w:
            dWp = ops.zeros((out, inf), F32)
            wgrad(ops, mod, dZ, X, dWp)
            dw = unpack_wgrad(dWp, mod.spatial)
        if need_b:
            db = ops.zeros((out,), F32)
            ops.colsum_bf16(dZ, db)
        return dx, dw, db, None, None


# ------------------------------------------------------------------------------------------------ thin Linear (the box head's fc_reg)
THIN_MAX_N = 16                                            # cs_gemm_nt epilogues 10 / 11 / 12: one 16-column MFMA tile


class LinearThin(KernelLayer, nn.Linear):
    """nn.Linear(in_features, out_features) with out_features <= 16 -- its parameters, names, initialisation and state dict -- on the thin
    streaming kernels (the ROWS forms of epilogues 10 / 11 / 12 of cs_gemm_nt) when the tensors live on a backend with THIN_HEADS and
    in_features % 64 == 0; F.linear otherwise.  The box head's fc_reg (512 | 1024 -> 4), which LinearAct (out % 8 == 0) does not take.

    fused: True = the kernels or NotImplementedError, False = F.linear, None = conv.FUSED_THIN_DEFAULT where the kernels can run.
    forward(x): x [..., in_features] fp32 or bf16, read in place where its rows are 16-byte aligned -> **fp32** [..., out_features] on the
    kernel route WHATEVER x's dtype (acc + bias, not rounded again): what det_losses.bbox_head_loss and det_post.delta2bbox take without
    a copy.  The input gradient comes back in x's dtype; the parameter gradients are fp32, from HipOps.thin_wgrad where the backend has
    THIN_WGRAD (and conv.THIN_WGRAD_DEFAULT), from the padded route of conv.thin_param_grads otherwise."""
    FLAG = "THIN_HEADS"
    COVERAGE = "in % 64 == 0, out <= 16, fp32 parameters, fp32 / bf16 input"

    def __init__(self, in_features, out_features, bias=True, ops=None, fused=None, **kw):
        super().__init__(in_features, out_features, bias=bias, **kw)
        self.ops = ops
        self.fused = fused

    def covered(self, x) -> bool:
        return (self.in_features % 64 == 0 and self.out_features <= THIN_MAX_N and self.weight.dtype == F32 and x.dtype in (F32, BF16)
                and x.dim() >= 1 and x.shape[-1] == self.in_features and x.numel() > 0 and x.device == self.weight.device)

    def describe(self):
        return f"LinearThin({self.in_features}, {self.out_features})"

    def fused_default(self):
        from . import conv
        return conv.FUSED_THIN_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.linear(x, self.weight, self.bias)
        return _LinearThinFn.apply(x, self.weight, self.bias, self, k)

    def gemm_weights(self):
        """(W bf16 [out, in], bias fp32 [out] | None), rebuilt when the parameters' version counters (or their storage) change."""
        return packed(self, lambda: (self.weight.detach().to(BF16).contiguous(), bias_f32(self.bias)))


def _thin_rows2d(ops, x, width):
    """x [..., width] fp32 / bf16 -> rows [rows, width] for the thin forms: x itself where its rows are dense enough to be read in place
    (unit column stride, 16-byte aligned rows and base), a contiguous copy otherwise."""
    X = x.reshape(-1, width)
    unit = 4 if X.dtype == F32 else 8
    if X.stride(1) != 1 or (X.shape[0] > 1 and (X.stride(0) < width or X.stride(0) % unit)) or X.data_ptr() % 16:
        X = X.contiguous()
    return X.detach()


class _LinearThinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops):
        inf, out = mod.in_features, mod.out_features
        W, b32 = mod.gemm_weights()
        X = _thin_rows2d(ops, x, inf)
        Y = ops.empty((X.shape[0], out), F32)
        ops.thin_fwd(X, W, b32, Y, R=0)
        ctx.mod, ctx.ops, ctx.x_shape, ctx.x_dtype, ctx.has_bias = mod, ops, tuple(x.shape), x.dtype, bias is not None
        if any(ctx.needs_input_grad[1:3]):
            ctx.save_for_backward(X)
        return Y.view(*x.shape[:-1], out)

    @staticmethod
    def backward(ctx, d_out):
        from .conv import thin_param_grads, thin_wgrad_direct          # conv imports nothing from here
        mod, ops = ctx.mod, ctx.ops
        inf, out = mod.in_features, mod.out_features
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        dY = d_out.reshape(-1, out).to(F32).contiguous()
        rows = dY.shape[0]
        dx = dw = db = None
        if need_x:
            W, _ = mod.gemm_weights()
            dX = ops.empty((rows, inf), ctx.x_dtype)
            ops.thin_dgrad(dY, W, dX, R=0)
            dx = dX.view(ctx.x_shape)
        if need_w or need_b:
            (X,) = ctx.saved_tensors
            if thin_wgrad_direct(ops):
                ((dw, db),) = thin_param_grads(ops, mod, dY, X, [out], [(need_w, need_b)], R=0)
            else:                                                      # the padded route: bf16 dY rows [rows, 16], bf16 X
                dYr = ops.zeros((rows, THIN_MAX_N), BF16)
                dYr[:, :out] = dY
                Xb = X
                if X.dtype != BF16 and need_w:
                    Xb = ops.empty((rows, inf), BF16)
                    ops.cast_f32_bf16(X if X.is_contiguous() else X.contiguous(), Xb)
                ((dw, db),) = thin_param_grads(ops, mod, dYr, Xb, [out], [(need_w, need_b)])
            if dw is not None:
                dw = dw.reshape(out, inf)
        return dx, dw, db, None, None
