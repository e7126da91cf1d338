"""The detector heads' 3 x 3 convolutions as implicit GEMMs on channel-last maps (include/clipself_conv.h).

`Conv2d(Cin, Cout, 3, padding=1)` on a map held as bf16 rows [N*H*W, Cin] is the GEMM  Y[M, Cout] = A[M, 9*Cin] . Wg^T + bias  whose A
rows are the map's rows shifted by the nine taps (zeros where a tap leaves the image).  HipOps.conv3x3 gathers A on the fly; the explicit
matrix (HipOps.im2col3x3) exists for the weight gradient and as a second route.  The backward is the same family, as in neck.Deconv2x2:

  input gradient   dX = conv3x3(dY rows, WgT), the flipped and transposed weights (Cout % 64 == 0; otherwise im2col(dY) . WgT^T);
  weight gradient  dWg[Cout, 9*Cin] += dY^T . cols  (cs_gemm_wgrad_tn on chunks of the explicit matrix under CHUNK_BYTES);
  bias gradient    a column sum of the dY rows (cs_colsum_bf16).

No atomics: equal inputs give equal bits.  Operands are bf16, accumulation is fp32, each result is rounded once, at its output type.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .det_backend import kernel_ops
from .neck import CHUNK_BYTES, EPI_BF16, EPI_F32, _version, _wgrad

BF16, F32 = torch.bfloat16, torch.float32

# Whether fused=None takes the kernels where the backend has them: set from profiles/conv3x3_bench.md by the rule of FUSED_SCORES_DEFAULT
# and FUSED_PROPOSALS_DEFAULT -- on only if the kernel route wins forward + backward against the faster torch variant at all four shapes.
# It does: 1.03 - 1.14 x against F.conv2d under bf16 autocast (the faster one), 4.3 - 4.7 x against fp32, the form the detector runs.
FUSED_CONV_DEFAULT = True
ROUTES = ("implicit", "im2col")


def pack_weights(weight):
    """(Wg bf16 [Cout, 9*Cin], WgT bf16 [Cin, 9*Cout]) of a [Cout, Cin, 3, 3] weight:  Wg[co, t*Cin + ci] = weight[co, ci, ky, kx] and
    WgT[ci, t*Cout + co] = weight[co, ci, 2 - ky, 2 - kx], t = ky*3 + kx."""
    Cout, Cin = weight.shape[:2]
    wb = weight.detach().to(BF16)
    Wg = wb.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    WgT = wb.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).contiguous()
    return Wg, WgT


def _pad_k(Wm):
    """A packed weight matrix with K = 9*C padded with zero columns to a multiple of 64 (cs_gemm_nt's K tile): the im2col route of a
    channel count that is no multiple of 64."""
    K = Wm.shape[1]
    Kp = (K + 63) // 64 * 64
    if Kp == K:
        return Wm
    out = Wm.new_zeros(Wm.shape[0], Kp)
    out[:, :K] = Wm
    return out


def _is_channel_last(t):
    """True when t [N, C, H, W] is dense in (n, y, x, c) order, so that its rows [N*H*W, C] are a view."""
    return t.permute(0, 2, 3, 1).is_contiguous()


def _row_chunks(M, row_bytes):
    """[(row0, rows)] covering M rows with chunks of at most CHUNK_BYTES (neck._chunks, on rows instead of images)."""
    n = max(1, min(M, CHUNK_BYTES // max(1, row_bytes)))
    return [(r0, min(n, M - r0)) for r0 in range(0, M, n)]


class Conv3x3(nn.Conv2d):
    """nn.Conv2d(Cin, Cout, 3, padding=1) -- its parameters, names, initialisation and state dict -- whose forward and backward run on the
    HIP kernels when the tensors live on a backend with CONV3X3, Cin % 64 == 0 and Cout % 8 == 0; F.conv2d otherwise.

    fused: True = the kernels or NotImplementedError, False = F.conv2d, None = FUSED_CONV_DEFAULT where the kernels can run.
    route: "implicit" (csc_conv3x3) or "im2col" (csc_im2col3x3 + cs_gemm_nt) for the forward and the input gradient.
    forward(x): x [N, Cin, H, W] fp32 or bf16 of any strides -> [N, Cout, H, W] of x's dtype with channel-last strides (kernel route)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True, ops=None, fused=None, route="implicit", **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        assert self.kernel_size == (3, 3) and self.stride == (1, 1) and self.padding == (1, 1) and self.dilation == (1, 1) \
            and self.groups == 1 and self.padding_mode == "zeros", "Conv3x3 is Conv2d(kernel_size=3, stride=1, padding=1) and nothing else"
        assert route in ROUTES, route
        self.ops = ops
        self.fused = fused
        self.route = route
        self._wcache = None

    # ------------------------------------------------------------------------------------------ dispatch
    def covered(self, x) -> bool:
        """What the kernels cover: fp32 parameters, a 4-D fp32 / bf16 input, Cin % 64 == 0, Cout % 8 == 0."""
        return (self.in_channels % 64 == 0 and self.out_channels % 8 == 0 and self.weight.dtype == F32 and x.dim() == 4
                and x.dtype in (F32, BF16) and x.shape[1] == self.in_channels and x.numel() > 0 and x.device == self.weight.device)

    def kernel_backend(self, x):
        """The backend whose CONV3X3 kernels serve forward(x), or None (-> F.conv2d); NotImplementedError where fused=True cannot be met."""
        ops, fused = self.ops, self.fused
        if fused is not False and ops is not None and not x.is_cuda and getattr(ops, "CONV3X3", False) \
                and ops.empty((1,), F32).device == x.device:
            k = ops if fused or FUSED_CONV_DEFAULT else None          # a host backend (the tests' reference ops) serves host tensors
        else:
            k = kernel_ops(x, "CONV3X3", ops, fused, FUSED_CONV_DEFAULT)
        if k is not None and not self.covered(x):
            if fused:
                raise NotImplementedError(f"fused=True: Conv3x3({self.in_channels}, {self.out_channels}) on {x.dtype} {tuple(x.shape)} is outside "
                                          "the kernels' coverage (Cin % 64 == 0, Cout % 8 == 0, fp32 parameters, fp32 / bf16 input)")
            return None
        return k

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.conv2d(x, self.weight, self.bias, padding=1)
        return _Conv3x3Fn.apply(x, self.weight, self.bias, self, k, self.route)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(Wg bf16 [Cout, 9*Cin], WgT bf16 [Cin, 9*Cout], bias fp32 [Cout] | None), see pack_weights.  Rebuilt when the parameters'
        version counters (or their storage) change."""
        w, b = self.weight, self.bias
        key = (w.data_ptr(), _version(w), w.device, None if b is None else (b.data_ptr(), _version(b)))
        if self._wcache is None or self._wcache[0] != key:
            with torch.no_grad():
                Wg, WgT = pack_weights(w)
                bias = None if b is None else b.detach().to(F32).contiguous()
            self._wcache = (key, Wg, WgT, bias)
        return self._wcache[1:]


def _rows_bf16(ops, t):
    """t [N, C, H, W] fp32 / bf16 of any strides -> bf16 rows [N*H*W, C].  A channel-last bf16 tensor is returned as a view; a channel-last
    fp32 one goes through the cast kernel; a contiguous NCHW one through nchw_to_rows (cast and permutation in one pass)."""
    N, C, H, W = t.shape
    if not _is_channel_last(t) and not t.is_contiguous():
        t = t.contiguous(memory_format=torch.channels_last)
    if _is_channel_last(t):
        rows = t.permute(0, 2, 3, 1).reshape(N * H * W, C)
        if t.dtype == BF16:
            return rows
        out = ops.empty((N * H * W, C), BF16)
        ops.cast_f32_bf16(rows, out)
        return out
    out = ops.empty((N * H * W, C), BF16)
    ops.nchw_to_rows(t, N, H, W, C, 1, 0, out)
    return out


def _conv_rows(ops, route, X, Wm, bias, out, N, H, W):
    """out[M, Co] = conv3x3 of the rows X [M, Ci] with the packed weights Wm [Co, 9*Ci] (+ bias), by either route."""
    M, Ci = X.shape
    if route == "implicit" and Ci % 64 == 0:
        ops.conv3x3(X, Wm, out, bias, N, H, W)
        return
    Wp = _pad_k(Wm)
    Kp = Wp.shape[1]
    epi = EPI_F32 if out.dtype == F32 else EPI_BF16
    cols = None
    for r0, n in _row_chunks(M, Kp * 2):
        if cols is None or cols.shape[0] != n:
            cols = ops.empty((n, Kp), BF16) if Kp == 9 * Ci else ops.zeros((n, Kp), BF16)     # the K padding stays zero: im2col never writes it
        ops.im2col3x3(X, cols[:, :9 * Ci], N, H, W, r0)
        ops.gemm_nt(cols, Wp, out[r0:r0 + n], bias, epi=epi)


class _Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops, route):
        N, Cin, H, W = x.shape
        Cout = mod.out_channels
        Wg, _, b32 = mod.gemm_weights()
        X = _rows_bf16(ops, x)
        Y = ops.empty((N * H * W, Cout), x.dtype)
        _conv_rows(ops, route, X, Wg, b32, Y, N, H, W)
        ctx.mod, ctx.ops, ctx.route, ctx.geom, ctx.x_dtype = mod, ops, route, (N, H, W), x.dtype
        ctx.has_bias = bias is not None
        if any(ctx.needs_input_grad[1:3]):
            ctx.save_for_backward(X)                       # the bf16 map, not the nine times larger matrix
        return Y.view(N, H, W, Cout).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops, route = ctx.mod, ctx.ops, ctx.route
        N, H, W = ctx.geom
        Cin, Cout, M = mod.in_channels, mod.out_channels, N * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        if d_out.dtype not in (F32, BF16):
            d_out = d_out.to(F32)
        dY = _rows_bf16(ops, d_out)
        dx = dw = db = None
        if need_x:
            _, WgT, _ = mod.gemm_weights()
            dX = ops.empty((M, Cin), ctx.x_dtype)
            _conv_rows(ops, route, dY, WgT, None, dX, N, H, W)
            dx = dX.view(N, H, W, Cin).permute(0, 3, 1, 2)
        if need_w:
            (X,) = ctx.saved_tensors
            dWg = ops.zeros((Cout, 9 * Cin), F32)
            cols = None
            for r0, n in _row_chunks(M, 9 * Cin * 2):
                if cols is None or cols.shape[0] != n:
                    cols = ops.empty((n, 9 * Cin), BF16)
                ops.im2col3x3(X, cols, N, H, W, r0)
                _wgrad(ops, mod, dY[r0:r0 + n], cols, dWg)
            dw = dWg.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
        if need_b:
            db = ops.zeros((Cout,), F32)
            ops.colsum_bf16(dY, db)
        return dx, dw, db, None, None, None


# ------------------------------------------------------------------------------------------------ 1 x 1 convolutions (the FPN's laterals)
# Whether fused=None takes the GEMMs where the backend has them: set from profiles/fpn_bench.md (the laterals with their norms, forward +
# backward) by the rule of FUSED_CONV_DEFAULT.  Off: the kernel laterals take 2.53 / 5.59 / 7.14 ms (B/16 640^2, B/16 1024^2, L/14-336 896^2)
# against 1.82 / 4.06 / 5.01 ms of torch under bf16 autocast on channels-last inputs (0.70 - 0.73 x; 1.45 - 1.60 x against torch fp32).
# The GEMMs are not the cost: an fp32 NCHW input pays the rows conversion (10 - 11 %) and, since a layer returns its input's type, fp32
# maps through the norm and both gradients, twice the bytes of autocast's bf16 ones (the per-stage table of profiles/fpn_bench.md).
FUSED_CONV1X1_DEFAULT = False


def pack_weights_1x1(weight):
    """(W bf16 [Cout, Cin], WT bf16 [Cin, Cout rounded up to 64]) of a [Cout, Cin, 1, 1] weight.  WT[ci, co] = W[co, ci] is the input
    gradient's B operand; its zero columns pad that contraction to cs_gemm_nt's K tile (as linear.pack_weights)."""
    Cout, Cin = weight.shape[:2]
    Wm = weight.detach().to(BF16).reshape(Cout, Cin).contiguous()
    WT = Wm.new_zeros(Cin, (Cout + 63) // 64 * 64)
    WT[:, :Cout] = Wm.t()
    return Wm, WT


class Conv1x1(nn.Conv2d):
    """nn.Conv2d(Cin, Cout, 1) -- its parameters, names, initialisation and state dict -- as one GEMM on channel-last rows,
    Y[N*H*W, Cout] = X[N*H*W, Cin] . W^T + bias, when the tensors live on a backend with FPN_TOPDOWN, Cin % 64 == 0 and Cout % 8 == 0 (what
    cs_gemm_nt and cs_gemm_wgrad_tn take); F.conv2d otherwise.  No kernel of its own: cs_gemm_nt forward and for the input gradient,
    cs_gemm_wgrad_tn for the weight gradient, cs_colsum_bf16 for the bias gradient.

    fused: True = the kernels or NotImplementedError, False = F.conv2d, None = FUSED_CONV1X1_DEFAULT where the kernels can run.
    forward(x): x [N, Cin, H, W] fp32 or bf16 of any strides -> [N, Cout, H, W] of x's dtype with channel-last strides (kernel route)."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=True, ops=None, fused=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        assert self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0) and self.dilation == (1, 1) \
            and self.groups == 1, "Conv1x1 is Conv2d(kernel_size=1, stride=1, padding=0) and nothing else"
        self.ops = ops
        self.fused = fused
        self._wcache = None

    # ------------------------------------------------------------------------------------------ dispatch
    def covered(self, x) -> bool:
        """What the kernels cover: fp32 parameters, a 4-D fp32 / bf16 input, Cin % 64 == 0, Cout % 8 == 0."""
        return (self.in_channels % 64 == 0 and self.out_channels % 8 == 0 and self.weight.dtype == F32 and x.dim() == 4
                and x.dtype in (F32, BF16) and x.shape[1] == self.in_channels and x.numel() > 0 and x.device == self.weight.device)

    def kernel_backend(self, x):
        """The backend whose GEMMs serve forward(x), or None (-> F.conv2d); NotImplementedError where fused=True cannot be met."""
        ops, fused = self.ops, self.fused
        if fused is not False and ops is not None and not x.is_cuda and getattr(ops, "FPN_TOPDOWN", False) \
                and ops.empty((1,), F32).device == x.device:
            k = ops if fused or FUSED_CONV1X1_DEFAULT else None       # a host backend (the tests' reference ops) serves host tensors
        else:
            k = kernel_ops(x, "FPN_TOPDOWN", ops, fused, FUSED_CONV1X1_DEFAULT)
        if k is not None and not self.covered(x):
            if fused:
                raise NotImplementedError(f"fused=True: Conv1x1({self.in_channels}, {self.out_channels}) on {x.dtype} {tuple(x.shape)} is outside "
                                          "the kernels' coverage (Cin % 64 == 0, Cout % 8 == 0, fp32 parameters, fp32 / bf16 input)")
            return None
        return k

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.conv2d(x, self.weight, self.bias)
        return _Conv1x1Fn.apply(x, self.weight, self.bias, self, k)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(W bf16 [Cout, Cin], WT bf16 [Cin, Cout rounded up to 64], bias fp32 [Cout] | None), see pack_weights_1x1.  Rebuilt when the
        parameters' version counters (or their storage) change."""
        w, b = self.weight, self.bias
        key = (w.data_ptr(), _version(w), w.device, None if b is None else (b.data_ptr(), _version(b)))
        if self._wcache is None or self._wcache[0] != key:
            with torch.no_grad():
                Wm, WT = pack_weights_1x1(w)
                bias = None if b is None else b.detach().to(F32).contiguous()
            self._wcache = (key, Wm, WT, bias)
        return self._wcache[1:]


class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops):
        N, Cin, H, W = x.shape
        Cout = mod.out_channels
        Wm, _, b32 = mod.gemm_weights()
        X = _rows_bf16(ops, x)
        Y = ops.empty((N * H * W, Cout), x.dtype)
        ops.gemm_nt(X, Wm, Y, b32, epi=EPI_F32 if x.dtype == F32 else EPI_BF16)
        ctx.mod, ctx.ops, ctx.geom, ctx.x_dtype = mod, ops, (N, H, W), x.dtype
        ctx.has_bias = bias is not None
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(X)
        return Y.view(N, H, W, Cout).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops = ctx.mod, ctx.ops
        N, H, W = ctx.geom
        Cin, Cout, M = mod.in_channels, mod.out_channels, N * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        if d_out.dtype not in (F32, BF16):
            d_out = d_out.to(F32)
        dY = _rows_bf16(ops, d_out)
        dx = dw = db = None
        if need_x:
            _, WT, _ = mod.gemm_weights()
            Kp = WT.shape[1]
            if Kp != Cout:                                             # zero columns pad the contraction to the K tile
                dYp = ops.zeros((M, Kp), BF16)
                dYp[:, :Cout] = dY
            else:
                dYp = dY
            dX = ops.empty((M, Cin), ctx.x_dtype)
            ops.gemm_nt(dYp, WT, dX, None, epi=EPI_F32 if ctx.x_dtype == F32 else EPI_BF16)
            dx = dX.view(N, H, W, Cin).permute(0, 3, 1, 2)
        if need_w:
            (X,) = ctx.saved_tensors
            dWm = ops.zeros((Cout, Cin), F32)
            _wgrad(ops, mod, dY, X, dWm)
            dw = dWm.view(Cout, Cin, 1, 1)
        if need_b:
            db = ops.zeros((Cout,), F32)
            ops.colsum_bf16(dY, db)
        return dx, dw, db, None, None
