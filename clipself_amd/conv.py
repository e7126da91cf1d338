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

from .det_layer import (BF16, F32, KernelLayer, bias_f32, conv_covered, epi_for, is_channel_last, kernel_grad, packed, pad_cols, param_steps, params_key,
                        row_chunks, rows_bf16, rows_to_map, wgrad)

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
    """det_layer.pad_cols of a packed weight matrix under the name it had here, for callers written before it moved."""
    return pad_cols(None, Wm)


class _ConvLayer(KernelLayer, nn.Conv2d):
    """What the three convolutions share of their dispatch: the coverage predicate and the name in the refusal."""
    COUT_MULTIPLE = 8
    COVERAGE = "Cin % 64 == 0, Cout % 8 == 0, fp32 parameters, fp32 / bf16 input"

    def covered(self, x) -> bool:
        """What the kernels cover: fp32 parameters, a 4-D fp32 / bf16 input, Cin % 64 == 0, Cout % COUT_MULTIPLE == 0."""
        return conv_covered(self, x, self.COUT_MULTIPLE)

    def describe(self):
        return f"{type(self).__name__}({self.in_channels}, {self.out_channels})"


class Conv3x3(_ConvLayer):
    """nn.Conv2d(Cin, Cout, 3, padding=1) -- its parameters, names, initialisation and state dict -- whose forward and backward run on the
    HIP kernels when the tensors live on a backend with CONV3X3, Cin % 64 == 0 and Cout % 8 == 0; F.conv2d otherwise.

    fused: True = the kernels or NotImplementedError, False = F.conv2d, None = FUSED_CONV_DEFAULT where the kernels can run.
    route: "implicit" (csc_conv3x3) or "im2col" (csc_im2col3x3 + cs_gemm_nt) for the forward and the input gradient.
    forward(x): x [N, Cin, H, W] fp32 or bf16 of any strides -> [N, Cout, H, W] of x's dtype with channel-last strides (kernel route)."""
    FLAG = "CONV3X3"

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True, ops=None, fused=None, route="implicit", **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        assert self.kernel_size == (3, 3) and self.stride == (1, 1) and self.padding == (1, 1) and self.dilation == (1, 1) \
            and self.groups == 1 and self.padding_mode == "zeros", "Conv3x3 is Conv2d(kernel_size=3, stride=1, padding=1) and nothing else"
        assert route in ROUTES, route
        self.ops = ops
        self.fused = fused
        self.route = route

    def fused_default(self):
        return FUSED_CONV_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.conv2d(x, self.weight, self.bias, padding=1)
        return _Conv3x3Fn.apply(x, self.weight, self.bias, self, k, self.route)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(Wg bf16 [Cout, 9*Cin], WgT bf16 [Cin, 9*Cout], bias fp32 [Cout] | None), see pack_weights.  Rebuilt when the parameters'
        version counters (or their storage) change."""
        return packed(self, lambda: (*pack_weights(self.weight), bias_f32(self.bias)))


def _conv_rows(ops, route, X, Wm, bias, out, N, H, W):
    """out[M, Co] = conv3x3 of the rows X [M, Ci] with the packed weights Wm [Co, 9*Ci] (+ bias), by either route."""
    M, Ci = X.shape
    if route == "implicit" and Ci % 64 == 0:
        ops.conv3x3(X, Wm, out, bias, N, H, W)
        return
    Wp = pad_cols(ops, Wm)                                 # K = 9*Ci up to cs_gemm_nt's K tile: a channel count that is no multiple of 64
    Kp = Wp.shape[1]
    epi = epi_for(out.dtype)
    cols = None
    for r0, n in row_chunks(M, Kp * 2):
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
        X = rows_bf16(ops, x)
        Y = ops.empty((N * H * W, Cout), x.dtype)
        _conv_rows(ops, route, X, Wg, b32, Y, N, H, W)
        ctx.mod, ctx.ops, ctx.route, ctx.geom, ctx.x_dtype = mod, ops, route, (N, H, W), x.dtype
        ctx.has_bias = bias is not None
        if any(ctx.needs_input_grad[1:3]):
            ctx.save_for_backward(X)                       # the bf16 map, not the nine times larger matrix
        return rows_to_map(Y, N, H, W)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops, route = ctx.mod, ctx.ops, ctx.route
        N, H, W = ctx.geom
        Cin, Cout, M = mod.in_channels, mod.out_channels, N * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        dY = rows_bf16(ops, kernel_grad(d_out))
        dx = dw = db = None
        if need_x:
            _, WgT, _ = mod.gemm_weights()
            dX = ops.empty((M, Cin), ctx.x_dtype)
            _conv_rows(ops, route, dY, WgT, None, dX, N, H, W)
            dx = rows_to_map(dX, N, H, W)
        if need_w:
            (X,) = ctx.saved_tensors
            dWg = ops.zeros((Cout, 9 * Cin), F32)
            cols = None
            for r0, n in row_chunks(M, 9 * Cin * 2):
                if cols is None or cols.shape[0] != n:
                    cols = ops.empty((n, 9 * Cin), BF16)
                ops.im2col3x3(X, cols, N, H, W, r0)
                wgrad(ops, mod, dY[r0:r0 + n], cols, dWg)
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


class Conv1x1(_ConvLayer):
    """nn.Conv2d(Cin, Cout, 1) -- its parameters, names, initialisation and state dict -- as one GEMM on channel-last rows,
    Y[N*H*W, Cout] = X[N*H*W, Cin] . W^T + bias, when the tensors live on a backend with FPN_TOPDOWN, Cin % 64 == 0 and Cout % 8 == 0 (what
    cs_gemm_nt and cs_gemm_wgrad_tn take); F.conv2d otherwise.  No kernel of its own: cs_gemm_nt forward and for the input gradient,
    cs_gemm_wgrad_tn for the weight gradient, cs_colsum_bf16 for the bias gradient.

    fused: True = the kernels or NotImplementedError, False = F.conv2d, None = FUSED_CONV1X1_DEFAULT where the kernels can run.
    forward(x): x [N, Cin, H, W] fp32 or bf16 of any strides -> [N, Cout, H, W] of x's dtype with channel-last strides (kernel route)."""
    FLAG = "FPN_TOPDOWN"                                   # the backend that has the top-down kernels has the laterals' GEMMs

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=True, ops=None, fused=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        assert self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0) and self.dilation == (1, 1) \
            and self.groups == 1, "Conv1x1 is Conv2d(kernel_size=1, stride=1, padding=0) and nothing else"
        self.ops = ops
        self.fused = fused

    def fused_default(self):
        return FUSED_CONV1X1_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.conv2d(x, self.weight, self.bias)
        return _Conv1x1Fn.apply(x, self.weight, self.bias, self, k)

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(W bf16 [Cout, Cin], WT bf16 [Cin, Cout rounded up to 64], bias fp32 [Cout] | None), see pack_weights_1x1.  Rebuilt when the
        parameters' version counters (or their storage) change."""
        return packed(self, lambda: (*pack_weights_1x1(self.weight), bias_f32(self.bias)))


class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, ops):
        N, Cin, H, W = x.shape
        Cout = mod.out_channels
        Wm, _, b32 = mod.gemm_weights()
        X = rows_bf16(ops, x)
        Y = ops.empty((N * H * W, Cout), x.dtype)
        ops.gemm_nt(X, Wm, Y, b32, epi=epi_for(x.dtype))
        ctx.mod, ctx.ops, ctx.geom, ctx.x_dtype = mod, ops, (N, H, W), x.dtype
        ctx.has_bias = bias is not None
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(X)
        return rows_to_map(Y, N, H, W)

    @staticmethod
    def backward(ctx, d_out):
        mod, ops = ctx.mod, ctx.ops
        N, H, W = ctx.geom
        Cin, Cout, M = mod.in_channels, mod.out_channels, N * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        dY = rows_bf16(ops, kernel_grad(d_out))
        dx = dw = db = None
        if need_x:
            _, WT, _ = mod.gemm_weights()
            dYp = pad_cols(ops, dY)                                    # zero columns pad the contraction to WT's K tile
            dX = ops.empty((M, Cin), ctx.x_dtype)
            ops.gemm_nt(dYp, WT, dX, None, epi=epi_for(ctx.x_dtype))
            dx = rows_to_map(dX, N, H, W)
        if need_w:
            (X,) = ctx.saved_tensors
            dWm = ops.zeros((Cout, Cin), F32)
            wgrad(ops, mod, dY, X, dWm)
            dw = dWm.view(Cout, Cin, 1, 1)
        if need_b:
            db = ops.zeros((Cout,), F32)
            ops.colsum_bf16(dY, db)
        return dx, dw, db, None, None


# ------------------------------------------------------------------------------------------------ thin 1 x 1 convolutions (RPN and mask heads)
# Whether fused=None takes the thin kernels where the backend has them, by the rule of FUSED_CONV_DEFAULT: on only if the kernel route wins
# forward + backward against the faster torch variant at every measured shape.  It does not (profiles/thin_heads_bench.md, B = 8): the
# heads alone win -- rpn_cls | rpn_reg 1.60 / 1.66 x (640^2 / 1024^2) on fp32 channel-last maps, the mask head's tail 1.54 x, the whole
# FCNMaskHead 7.86 against 10.27 ms of torch under bf16 autocast -- but the whole RPNHead over five levels ties autocast at 640^2 (6.32
# against 6.33 ms, 0.95 x when the maps arrive in NCHW; 1.07 x at 1024^2).  Off: fused=True selects the route, as for FUSED_FPN_DEFAULT.
FUSED_THIN_DEFAULT = False
THIN_MAX_N = 16                                            # cs_gemm_nt epilogues 10 / 11: one 16-column MFMA tile
# Whether the thin layers' parameter gradients take epilogue 12 (HipOps.thin_wgrad: dY and X read in place, one launch) where the backend
# has THIN_WGRAD, instead of dy_rows16 + cast_f32_bf16 + cs_gemm_wgrad_tn + cs_colsum_bf16.  Read when called.  Set from
# profiles/thin_wgrad_bench.md: on only if the new route is faster at every measured shape with non-overlapping (min .. max) spreads.
# It is: 4.4 - 5.9 x at rpn640 / rpn1024 (bf16 and fp32 rows) and the mask tail, 2.5 x at fc_reg (4096 x 1024 -> 4).
THIN_WGRAD_DEFAULT = True


def _thin_rows(ops, x):
    """x [N, C, H, W] -> its rows [N*H*W, C] for HipOps.thin_fwd: a channel-last fp32 / bf16 map (what BatchNormAct2d returns) is used in
    place (fp32 rows are rounded to bf16 in the kernel's registers), anything else goes through rows_bf16."""
    N, C, H, W = x.shape
    if x.dtype in (F32, BF16) and is_channel_last(x) and x.data_ptr() % 16 == 0:
        return x.permute(0, 2, 3, 1).reshape(N * H * W, C)
    return rows_bf16(ops, x)


def _thin_packed(convs):
    """(W bf16 [sum N, Cin] in module order, bias fp32 [sum N] | None) of thin convolutions that share an input.  Cached on the first
    module, rebuilt when a parameter's version counter (or storage) changes, as in gemm_weights.  A module without a bias contributes
    zeros when another one has a bias."""
    def build():
        Wp = torch.cat([c.weight.detach().reshape(c.out_channels, c.in_channels) for c in convs]).to(BF16).contiguous()
        if all(c.bias is None for c in convs):
            return Wp, None
        return Wp, torch.cat([c.weight.new_zeros(c.out_channels) if c.bias is None else c.bias.detach() for c in convs]).to(F32).contiguous()
    return packed(convs[0], build, key=tuple((id(c), *params_key(c.weight, c.bias), param_steps(c.weight), param_steps(c.bias)) for c in convs),
                  slot="_thin_cache")


def dy_rows16(ops, grads, M):
    """fp32 NCHW gradients [B, n_i, H, W] (contiguous) -> bf16 rows [M, 16], the modules' columns one behind the other and zeros past
    their sum: the A operand of cs_gemm_wgrad_tn (N = 16) and of cs_colsum_bf16.  32 bytes per row beside the 512 of X."""
    rows = ops.zeros((M, THIN_MAX_N), BF16)
    c0 = 0
    for g in grads:
        B, n, H, W = g.shape
        if B <= 65535 and W < (1 << 19):
            ops.nchw_to_rows(g, B, H, W, n, 1, 0, rows[:, c0:])
        else:
            rows[:, c0:c0 + n] = g.permute(0, 2, 3, 1).reshape(M, n).to(BF16)
        c0 += n
    return rows


def thin_wgrad_direct(ops):
    """Whether the thin layers' parameter gradients take epilogue 12 of cs_gemm_nt (HipOps.thin_wgrad) on this backend."""
    return bool(getattr(ops, "THIN_WGRAD", False)) and THIN_WGRAD_DEFAULT


def thin_wgrad_buffer(ops, mod, M, N, K):
    """mod's own grow-only workspace of HipOps.thin_wgrad, as det_layer.wgrad keeps its one."""
    need = ops.thin_wgrad_workspace(M, N, K)
    ws = mod.__dict__.get("_thin_wgrad_ws")
    if ws is None or ws.numel() < need or ws.device != mod.weight.device:
        ws = mod.__dict__["_thin_wgrad_ws"] = ops.empty((need,), F32)
    return ws


def thin_param_grads(ops, mod, dYr, Xb, widths, need, R=None, dY2=None):
    """[(dW [n_i, Cin, 1, 1] | None, db [n_i] | None)] of the modules in `widths`.  need: [(weight?, bias?)].
    R is None (the padded route): the modules' columns sit in dYr bf16 [M, 16] and Xb is bf16: one cs_gemm_wgrad_tn at N = 16 and one
    cs_colsum_bf16, sliced per module.
    R given (the direct route, thin_wgrad_direct(ops)): dYr is the fp32 gradient as autograd hands it -- rows [M, N] for R == 0, else the
    contiguous NCHW planes of the first module with dY2 those of the second -- and Xb the saved rows, fp32 or bf16, read in place: ONE
    HipOps.thin_wgrad launch gives dW and db of both modules, whichever of them are needed."""
    Cin = Xb.shape[1]
    if R is not None:
        M, N = Xb.shape[0], sum(widths)
        dW, db = ops.empty((N, Cin), F32), ops.empty((N,), F32)
        ops.thin_wgrad(dYr, Xb, dW, db=db, R=R, dY2=dY2, workspace=thin_wgrad_buffer(ops, mod, M, N, Cin))
        out, c0 = [], 0
        for n, (w, b) in zip(widths, need):
            out.append((dW[c0:c0 + n].reshape(n, Cin, 1, 1) if w else None, db[c0:c0 + n] if b else None))
            c0 += n
        return out
    dW = db = None
    if any(w for w, _ in need):
        dW = ops.zeros((THIN_MAX_N, Cin), F32)
        wgrad(ops, mod, dYr, Xb, dW)
    if any(b for _, b in need):
        db = ops.zeros((THIN_MAX_N,), F32)
        ops.colsum_bf16(dYr, db)
    out, c0 = [], 0
    for n, (w, b) in zip(widths, need):
        out.append((dW[c0:c0 + n].reshape(n, Cin, 1, 1) if w else None, db[c0:c0 + n] if b else None))
        c0 += n
    return out


class Conv1x1Thin(_ConvLayer):
    """nn.Conv2d(Cin, Cout, 1) with Cout <= 16 -- its parameters, names, initialisation and state dict -- on the thin streaming kernels
    (epilogues 10 / 11 of cs_gemm_nt) when the tensors live on a backend with THIN_HEADS and Cin % 64 == 0; F.conv2d otherwise.  The RPN's
    rpn_cls / rpn_reg and the mask head's conv_logits.  The weight and bias gradients are epilogue 12 (HipOps.thin_wgrad: dY and X read in
    place, one launch) where thin_wgrad_direct(ops) holds; otherwise cs_gemm_wgrad_tn on dY rows padded to 16 columns and cs_colsum_bf16.

    fused: True = the kernels or NotImplementedError, False = F.conv2d, None = FUSED_THIN_DEFAULT where the kernels can run.
    forward(x): x [N, Cin, H, W] fp32 or bf16 of any strides (a channel-last map is read in place) -> contiguous NCHW fp32
    [N, Cout, H, W] on the kernel route, whatever x's dtype: what det_losses.rpn_loss and det_proposals.rpn_proposals take without a copy."""
    FLAG, COUT_MULTIPLE = "THIN_HEADS", 1                  # any Cout <= THIN_MAX_N
    COVERAGE = "Cin % 64 == 0, fp32 parameters, fp32 / bf16 input"

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=True, ops=None, fused=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        assert self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0) and self.dilation == (1, 1) \
            and self.groups == 1, "Conv1x1Thin is Conv2d(kernel_size=1, stride=1, padding=0) and nothing else"
        assert out_channels <= THIN_MAX_N, f"Conv1x1Thin has at most {THIN_MAX_N} output channels, got {out_channels} (wider: Conv1x1)"
        self.ops = ops
        self.fused = fused

    def fused_default(self):
        return FUSED_THIN_DEFAULT

    def forward(self, x):
        k = self.kernel_backend(x)
        if k is None:
            return F.conv2d(x, self.weight, self.bias)
        return _thin_apply(x, (self,), k)[0]

    # ------------------------------------------------------------------------------------------ operands
    def gemm_weights(self):
        """(W bf16 [Cout, Cin], bias fp32 [Cout] | None), rebuilt when the parameters' version counters (or their storage) change."""
        return _thin_packed((self,))


def thin_heads(x, convs):
    """[conv(x) for conv in convs] for Conv1x1Thin modules that read one input.  Two modules whose widths sum to <= 16 and whose backend
    serves x run as ONE forward launch (the planes form of epilogue 10 with the split at the first module's width: two contiguous NCHW
    fp32 tensors in one allocation) and ONE input-gradient launch; a missing output gradient counts as zeros.  Anything else -- a module on
    the torch route, more than two modules, widths past 16 -- runs module by module, each by its own dispatch."""
    convs = tuple(convs)
    ks = [c.kernel_backend(x) for c in convs]
    together = (len(convs) == 2 and all(k is not None and k is ks[0] for k in ks) and sum(c.out_channels for c in convs) <= THIN_MAX_N
                and len({c.in_channels for c in convs}) == 1)
    if not together:
        return tuple(c(x) for c in convs)
    return _thin_apply(x, convs, ks[0])


def _thin_apply(x, convs, ops):
    params = []
    for c in convs:
        params += [c.weight, c.bias]
    return _ThinFn.apply(x, convs, ops, *params)


class _ThinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, convs, ops, *params):
        B, Cin, H, W = x.shape
        M, R = B * H * W, H * W
        widths = [c.out_channels for c in convs]
        Wp, bias = _thin_packed(convs)
        X = _thin_rows(ops, x)
        out = ops.empty((M * sum(widths),), F32)
        ops.thin_fwd(X, Wp, bias, out, R=R, split=widths[0] if len(convs) == 2 else None)
        ctx.convs, ctx.ops, ctx.geom, ctx.x_dtype, ctx.widths = convs, ops, (B, H, W), x.dtype, widths
        if any(ctx.needs_input_grad[3:]):
            ctx.save_for_backward(X)
        ys, o0 = [], 0
        for n in widths:
            ys.append(out[o0:o0 + M * n].view(B, n, H, W))
            o0 += M * n
        return tuple(ys)

    @staticmethod
    def backward(ctx, *d_outs):
        convs, ops, widths = ctx.convs, ctx.ops, ctx.widths
        B, H, W = ctx.geom
        M, R, Cin = B * H * W, H * W, convs[0].in_channels
        grads = []
        for d, n in zip(d_outs, widths):
            if d is None:
                d = ops.zeros((B, n, H, W), F32)
            grads.append(d.to(F32).contiguous())
        dx = None
        if ctx.needs_input_grad[0]:
            Wp, _ = _thin_packed(convs)
            dX = ops.empty((M, Cin), ctx.x_dtype)
            ops.thin_dgrad(grads[0], Wp, dX, R=R, dY2=grads[1] if len(grads) == 2 else None)
            dx = rows_to_map(dX, B, H, W)
        need = [(ctx.needs_input_grad[3 + 2 * i], ctx.needs_input_grad[4 + 2 * i] and c.bias is not None) for i, c in enumerate(convs)]
        out = [None] * (2 * len(convs))
        if any(w or b for w, b in need):
            (X,) = ctx.saved_tensors
            if thin_wgrad_direct(ops):                                 # the planes as they are, X as it was saved: one launch
                res = thin_param_grads(ops, convs[0], grads[0], X, widths, need, R=R, dY2=grads[1] if len(grads) == 2 else None)
                for i, (dw, db) in enumerate(res):
                    out[2 * i], out[2 * i + 1] = dw, db
                return (dx, None, None, *out)
            dYr = dy_rows16(ops, grads, M)
            if X.dtype != BF16 and any(w for w, _ in need):            # an fp32 map read in place: the weight gradient's operand is bf16
                Xc = X if X.is_contiguous() else X.contiguous()
                Xb = ops.empty((M, Cin), BF16)
                ops.cast_f32_bf16(Xc, Xb)
            else:
                Xb = X
            for i, (dw, db) in enumerate(thin_param_grads(ops, convs[0], dYr, Xb, widths, need)):
                out[2 * i], out[2 * i + 1] = dw, db
        return (dx, None, None, *out)
