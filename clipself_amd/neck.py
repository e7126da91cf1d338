"""The detector neck's transposed convolutions as GEMMs on the token stream.

`ConvTranspose2d(kernel_size=2, stride=2)` has no overlapping outputs: every input position (a token) owns one 2 x 2 output patch, so the
layer is one GEMM  Y[M, 4*Cout] = X[M, Cin] . Wg^T + bias  on token-major rows followed by a fixed permutation of Y into [B, Cout, 2h, 2w]
(HipOps.rows_to_nchw).  The frozen tower already holds X in that layout: `TokenRows` carries its bf16 stream to the first layer as it is.
The backward is the same GEMM family: the weight gradient dY^T . X (cs_gemm_wgrad_tn), the bias gradient a column sum of dY
(cs_colsum_bf16), the input gradient dY . Wg (cs_gemm_nt); dY is the output gradient brought to rows by HipOps.nchw_to_rows.  No atomics:
the same inputs give the same bits.

Operands are bf16, accumulation is fp32, and each result is rounded once, at its output type.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from .det_layer import CHUNK_BYTES  # noqa: F401  (the bound of a rows buffer keeps its public name here)
from .det_layer import BF16, F32, backend_device, epi_for, kernel_grad, packed, row_chunks, wgrad


class TokenRows(NamedTuple):
    """The tower's stream as a Deconv2x2 operand: rows bf16 [B * (h*w + off), C], token-major, `off` CLS rows in front of each image's
    h*w patch rows (TowerEngine.encode_dense(tap_rows=...))."""
    rows: torch.Tensor
    B: int
    h: int
    w: int
    off: int

    def nchw(self, dtype=F32):
        """The [B, C, h, w] map of the same values (what a torch convolution reads)."""
        C = self.rows.shape[1]
        return self.rows.view(self.B, self.h * self.w + self.off, C)[:, self.off:].permute(0, 2, 1).reshape(self.B, C, self.h, self.w).to(dtype)


class Deconv2x2(nn.ConvTranspose2d):
    """nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) -- its parameters, names, initialisation and state dict -- whose forward and
    backward run as GEMMs on token rows when `ops` (a kernel backend with DECONV_ROWS) is set, the tensors live on that backend's device,
    Cin % 64 == 0 and Cout % 16 == 0; F.conv_transpose2d otherwise.  forward(x): x an NCHW tensor (fp32 / bf16; the output has its type) or
    a TokenRows (output fp32, or `out_dtype`)."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2, bias=True, ops=None, out_dtype=F32, **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, bias=bias, **kw)
        assert self.kernel_size == (2, 2) and self.stride == (2, 2) and self.padding == (0, 0) and self.output_padding == (0, 0) \
            and self.dilation == (1, 1) and self.groups == 1 and self.padding_mode == "zeros", "Deconv2x2 is ConvTranspose2d(k=2, s=2) and nothing else"
        self.ops = ops
        self.out_dtype = out_dtype

    # ------------------------------------------------------------------------------------------ dispatch
    def fused_rows(self) -> bool:
        """True when a TokenRows on the backend's device would take the GEMM path: what the owner asks before it orders rows from the tower."""
        if self.ops is None or not getattr(self.ops, "DECONV_ROWS", False):
            return False
        if self.in_channels % 64 or self.out_channels % 16 or self.weight.dtype != F32:
            return False
        return self.weight.device == backend_device(self.ops)

    def fused(self, x) -> bool:
        """True when forward(x) takes the GEMM path."""
        if not self.fused_rows():
            return False
        t = x.rows if isinstance(x, TokenRows) else x
        if not isinstance(x, TokenRows) and (t.dim() != 4 or t.dtype not in (F32, BF16)):
            return False
        return t.device == backend_device(self.ops)

    def forward(self, x, output_size=None):
        if output_size is None and self.fused(x):
            if isinstance(x, TokenRows):
                assert x.rows.dtype == BF16 and x.rows.shape[1] == self.in_channels and x.rows.shape[0] == x.B * (x.h * x.w + x.off)
                return _DeconvFn.apply(x.rows, self.weight, self.bias, self, (x.B, x.h, x.w, x.off), self.out_dtype)
            B, C, h, w = x.shape
            assert C == self.in_channels
            return _DeconvFn.apply(x, self.weight, self.bias, self, None, x.dtype)
        if isinstance(x, TokenRows):
            x = x.nchw(self.weight.dtype)
        return super().forward(x, output_size)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(Wg bf16 [4*Cout, Cin], Wg^T bf16 [Cin, 4*Cout], bias4 fp32 [4*Cout] | None): Wg[(2*di + dj)*Cout + co, ci] = weight[ci, co, di, dj].
        Rebuilt when the parameters' version counters (or their storage) change."""
        return packed(self, self._pack)

    def _pack(self):
        Cin, Cout, b = self.in_channels, self.out_channels, self.bias
        wb = self.weight.detach().to(BF16)
        Wg = wb.permute(2, 3, 1, 0).reshape(4 * Cout, Cin).contiguous()
        WgT = wb.permute(0, 2, 3, 1).reshape(Cin, 4 * Cout).contiguous()
        return Wg, WgT, None if b is None else b.detach().to(F32).repeat(4).contiguous()


class _DeconvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, geom, out_dtype):
        ops, Cin, Cout = mod.ops, mod.in_channels, mod.out_channels
        Wg, _, bias4 = mod.gemm_weights()
        if geom is None:                                   # NCHW input -> bf16 rows, no CLS rows
            B, _, h, w = x.shape
            off = 0
            X = ops.empty((B * h * w, Cin), BF16)
            ops.nchw_to_rows(x.contiguous(), B, h, w, Cin, 1, 0, X)
        else:
            (B, h, w, off), X = geom, x
        R = h * w + off
        out = ops.empty((B, Cout, 2 * h, 2 * w), out_dtype)
        esize = 4 if out_dtype == F32 else 2
        epi = epi_for(out_dtype)
        Y = None
        for b0, nb in row_chunks(B, R * 4 * Cout * esize):                   # whole images per chunk
            if Y is None or Y.shape[0] != nb * R:
                Y = ops.empty((nb * R, 4 * Cout), out_dtype)
            ops.gemm_nt(X[b0 * R:(b0 + nb) * R], Wg, Y, bias4, epi=epi)
            ops.rows_to_nchw(Y, nb, h, w, Cout, 2, off, out[b0:b0 + nb])
        ctx.mod, ctx.geom, ctx.x_nchw, ctx.x_dtype = mod, (B, h, w, off), geom is None, x.dtype
        ctx.has_bias = bias is not None
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(X)
        return out

    @staticmethod
    def backward(ctx, d_out):
        mod = ctx.mod
        ops, Cin, Cout = mod.ops, mod.in_channels, mod.out_channels
        B, h, w, off = ctx.geom
        (X,) = ctx.saved_tensors
        R = h * w + off
        need_x, need_w, need_b = ctx.needs_input_grad[0] and ctx.x_nchw, ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        d_out = kernel_grad(d_out).contiguous()
        _, WgT, _ = mod.gemm_weights()
        dWg = ops.zeros((4 * Cout, Cin), F32) if need_w else None
        col = ops.zeros((4 * Cout,), F32) if need_b else None
        dx = ops.empty((B, Cin, h, w), ctx.x_dtype) if need_x else None
        dY = dXr = None
        for b0, nb in row_chunks(B, R * 4 * Cout * 2):
            M = nb * R
            if dY is None or dY.shape[0] != M:
                dY = ops.empty((M, 4 * Cout), BF16)
            ops.nchw_to_rows(d_out[b0:b0 + nb], nb, h, w, Cout, 2, off, dY)
            if need_w:
                wgrad(ops, mod, dY, X[b0 * R:(b0 + nb) * R], dWg)
            if need_b:
                ops.colsum_bf16(dY, col)
            if need_x:
                if dXr is None or dXr.shape[0] != M:
                    dXr = ops.empty((M, Cin), ctx.x_dtype)
                ops.gemm_nt(dY, WgT, dXr, None, epi=epi_for(ctx.x_dtype))
                ops.rows_to_nchw(dXr, nb, h, w, Cin, 1, 0, dx[b0:b0 + nb])
        dw = dWg.view(2, 2, Cout, Cin).permute(3, 2, 0, 1).contiguous() if need_w else None
        db = col.view(4, Cout).sum(0) if need_b else None
        return dx, dw, db, None, None, None

