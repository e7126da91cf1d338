"""What a kernel-backed detector layer is: the rule that picks its backend, the cache of its packed operands and the
helpers that bring maps to channel-last rows and back -- each stated once, for conv, linear, norm_act, fpn, neck and mask_head.

  layer_ops     det_backend.kernel_ops plus the one clause the layers need and the functional modules do not: a host backend serves host
                tensors, which is how the CPU tests run a layer's whole forward and backward on their reference ops;
  KernelLayer   the mixin beside nn.Conv2d / nn.Linear / nn.BatchNorm2d that turns a flag, a default and covered(x) into kernel_backend(x);
  packed        the packed operands of a module's parameters, rebuilt when a parameter's version counter or storage moves or a torch
                optimizer that owns it has stepped (the fused ones move neither);
  rows helpers  maps [N, C, H, W] as rows [N*H*W, C] and back, the chunking under CHUNK_BYTES, the padding to the GEMM's K tile, the weight
                gradient dY^T . X.

The epilogue numbers of cs_gemm_nt come from hip.py, the one place that defines them.  Importing hip.py loads no library: it defines
constants, signature tables and classes, and load_library() runs when the first HipOps is built.
"""
from __future__ import annotations

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from .det_backend import kernel_ops
from .hip import EPI_BF16, EPI_F32, EPI_RELU_BF16  # noqa: F401  (EPI_RELU_BF16 for linear and mask_head)

BF16, F32 = torch.bfloat16, torch.float32
CHUNK_BYTES = 512 << 20                       # upper bound of an intermediate rows buffer (Y, dY, im2col columns); larger ones are cut into chunks


# ------------------------------------------------------------------------------------------------ dispatch
def backend_device(ops):
    """The device of a backend's tensors, learned from one allocation per backend object and kept on it."""
    dev = getattr(ops, "_layer_device", None)
    if dev is None:
        dev = ops._layer_device = ops.empty((1,), F32).device
    return dev


def layer_ops(x, flag, ops, fused, default):
    """The backend whose `flag` kernels serve tensor x, or None (-> the torch route), by det_backend.kernel_ops' rule -- fused=False never,
    fused=True the kernels or NotImplementedError, fused=None where the backend has them and `default` is true -- with one clause in
    front: a backend handed in as `ops`, with `flag`, whose tensors live on x's (non-CUDA) device serves x."""
    if fused is not False and ops is not None and not x.is_cuda and getattr(ops, flag, False) and backend_device(ops) == x.device:
        return ops if fused or default else None                      # a host backend (the tests' reference ops) serves host tensors
    return kernel_ops(x, flag, ops, fused, default)


def uncovered(fused, what, coverage):
    """The answer for a case the backend could serve but the kernels do not cover: None (-> torch), NotImplementedError under fused=True."""
    if fused:
        raise NotImplementedError(f"fused=True: {what} is outside the kernels' coverage ({coverage})")
    return None


class KernelLayer:
    """The dispatch of a kernel-backed nn.Module.  The subclass sets `ops` and `fused` in its constructor and states
        FLAG              the backend attribute that announces its kernels,
        COVERAGE          the sentence that describes covered(x), for the refusal,
        fused_default()   its module's FUSED_*_DEFAULT, read when called (tests and benchmarks set the global),
        covered(x)        whether the kernels take x,
        describe()        the layer as the refusal names it.
    fused: True = the kernels or NotImplementedError, False = torch, None = fused_default() where the kernels can run.  The refusals come
    in this order: fused=False, the device, the flag, the coverage."""
    FLAG = COVERAGE = None

    def kernel_backend(self, x):
        """The backend whose kernels serve forward(x), or None (-> torch); NotImplementedError where fused=True cannot be met."""
        k = layer_ops(x, self.FLAG, self.ops, self.fused, self.fused_default())
        if k is not None and not self.covered(x):
            return uncovered(self.fused, f"{self.describe()} on {x.dtype} {tuple(x.shape)}", self.COVERAGE)
        return k


def conv_covered(conv, x, cout_multiple=1) -> bool:
    """What the convolutions' GEMMs cover: fp32 parameters, a 4-D fp32 / bf16 input on their device, Cin % 64 == 0 and Cout a multiple of
    `cout_multiple` (8 for rows that cs_gemm_nt writes, nothing for the thin forms)."""
    return (conv.in_channels % 64 == 0 and conv.out_channels % cout_multiple == 0 and conv.weight.dtype == F32 and x.dim() == 4
            and x.dtype in (F32, BF16) and x.shape[1] == conv.in_channels and x.numel() > 0 and x.device == conv.weight.device)


# ------------------------------------------------------------------------------------------------ packed operands
def version(t):
    try:
        return t._version
    except RuntimeError:                       # inference tensors carry no version counter
        return -1


def params_key(weight, bias):
    """What identifies a weight and bias as packed: storage, version counter (-1 for inference tensors) and device, so that the key moves
    with an optimizer step, a load_state_dict, a .to() and a `.data =`."""
    return (weight.data_ptr(), version(weight), weight.device, None if bias is None else (bias.data_ptr(), version(bias)))


def _optimizer_stepped(optimizer, args, kwargs):
    for group in optimizer.param_groups:
        for p in group["params"]:
            p.__dict__["_cs_steps"] = p.__dict__.get("_cs_steps", 0) + 1


register_optimizer_step_post_hook(_optimizer_stepped)      # every torch.optim.Optimizer of the process, whenever it was built


def param_steps(t):
    """How many steps torch optimizers that own tensor t have taken (0 for None, a buffer, a frozen module's parameter).  torch's fused
    optimizers (AdamW / Adam / SGD with fused=True) write the parameters through one multi-tensor kernel that leaves every `_version`
    and every storage where it was, so params_key alone cannot see their step; a cache of packed parameters keys on this count as well.
    The count is kept on the parameter itself by a process-wide optimizer-step hook: a step costs one dictionary write per parameter the
    optimizer owns, and a module that no optimizer owns is never repacked."""
    return 0 if t is None else t.__dict__.get("_cs_steps", 0)


def packed(mod, build, key=None, slot="_wcache"):
    """The tuple build() makes of mod's parameters (under no_grad), kept in mod.__dict__[slot] -- no buffer, no parameter: state_dict() does
    not see it -- and rebuilt when `key` (default: params_key of mod.weight and mod.bias) has moved or an optimizer that owns mod.weight
    or mod.bias has stepped since (param_steps: a step that params_key cannot see; after a step it can see the operands are rebuilt
    anyway).  A caller with a key of its own over other modules' parameters puts their param_steps into it."""
    if key is None:
        key = params_key(mod.weight, mod.bias)
    key = (key, param_steps(mod.weight), param_steps(getattr(mod, "bias", None)))
    _wcache = mod.__dict__.get(slot)
    if _wcache is None or _wcache[0] != key:
        with torch.no_grad():
            _wcache = mod.__dict__[slot] = (key, tuple(build()))
    return _wcache[1]


def bias_f32(bias):
    return None if bias is None else bias.detach().to(F32).contiguous()


# ------------------------------------------------------------------------------------------------ rows
def epi_for(dtype):
    """cs_gemm_nt's plain epilogue for an output type: C = acc + bias in fp32, or rounded to bf16."""
    return EPI_F32 if dtype == F32 else EPI_BF16


def kernel_grad(d_out):
    """An output gradient as the kernels read it: fp32 and bf16 as they are, anything else as fp32."""
    return d_out if d_out.dtype in (F32, BF16) else d_out.to(F32)


def row_chunks(M, row_bytes):
    """[(row0, rows)] covering M rows (or images, with an image's bytes as row_bytes) in chunks of at most CHUNK_BYTES, one row at least."""
    n = max(1, min(M, CHUNK_BYTES // max(1, row_bytes)))
    return [(r0, min(n, M - r0)) for r0 in range(0, M, n)]


def pad_cols(ops, t, multiple=64):
    """t [rows, K] with zero columns up to a multiple of `multiple` (cs_gemm_nt's K tile); t itself where K is one already.  The copy comes
    from ops.zeros, or beside t where ops is None."""
    K = t.shape[1]
    Kp = (K + multiple - 1) // multiple * multiple
    if Kp == K:
        return t
    out = t.new_zeros((t.shape[0], Kp)) if ops is None else ops.zeros((t.shape[0], Kp), t.dtype)
    out[:, :K] = t
    return out


def is_channel_last(t):
    """True when t [N, C, H, W] is dense in (n, y, x, c) order, so that its rows [N*H*W, C] are a view."""
    return t.permute(0, 2, 3, 1).is_contiguous()


def rows_to_map(rows, N, H, W):
    """rows [N*H*W, C] -> the map [N, C, H, W] with channel-last strides, a view."""
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def channel_last_rows(t):
    """t [N, C, H, W] -> (its rows [N*H*W, C] as a view of a channel-last tensor, made channel-last by torch where it is not)."""
    if not is_channel_last(t):
        t = t.contiguous(memory_format=torch.channels_last)
        if not is_channel_last(t):                                    # torch keeps ambiguous strides (C == 1 or H == W == 1) as they are
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    N, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(N * H * W, C)


def rows_bf16(ops, t):
    """t [N, C, H, W] fp32 / bf16 of any strides -> bf16 rows [N*H*W, C].  A channel-last bf16 tensor is returned as a view; a channel-last
    fp32 one goes through the cast kernel; a contiguous NCHW one through nchw_to_rows (cast and permutation in one pass)."""
    N, C, H, W = t.shape
    if not is_channel_last(t) and not t.is_contiguous():
        t = t.contiguous(memory_format=torch.channels_last)
    if is_channel_last(t):
        rows = t.permute(0, 2, 3, 1).reshape(N * H * W, C)
        if t.dtype == BF16:
            return rows
        out = ops.empty((N * H * W, C), BF16)
        ops.cast_f32_bf16(rows, out)
        return out
    out = ops.empty((N * H * W, C), BF16)
    ops.nchw_to_rows(t, N, H, W, C, 1, 0, out)
    return out


def rows2d(ops, x, width):
    """x [..., width] fp32 / bf16 -> bf16 rows [rows, width] with 16-byte aligned rows: a view where x allows it, one cast kernel for fp32."""
    X = x.reshape(-1, width)
    if X.dtype == BF16:
        if X.stride(1) != 1 or X.stride(0) % 8 or X.data_ptr() % 16:
            X = X.contiguous()
        return X
    out = ops.empty(tuple(X.shape), BF16)
    ops.cast_f32_bf16(X.contiguous(), out)
    return out


def wgrad(ops, mod, dY, X, dW):
    """dW[N, K] += dY^T . X from the token-major operands; shapes cs_gemm_wgrad_tn does not cover go through explicit transposes and the NT
    split-K kernel (as TowerEngine._wgrad).  The workspace is mod's own grow-only buffer."""
    M, N = dY.shape
    K = X.shape[1]
    ws = mod.__dict__.get("_wgrad_ws")
    need = ops.gemm_wgrad_tn_workspace(N, K, M)
    tn = need > 0
    if not tn:
        Mp = (M + 63) // 64 * 64
        need = ops.gemm_wgrad_workspace(N, K, Mp)
    if ws is None or ws.numel() < need or ws.device != dY.device:
        ws = mod.__dict__["_wgrad_ws"] = ops.empty((need,), torch.uint8)
    if tn:
        ops.gemm_wgrad_tn(dY, X, dW, ws)
        return
    Xt, dYt = ops.empty((K, Mp), BF16), ops.empty((N, Mp), BF16)
    ops.transpose_bf16(X, Xt)
    ops.transpose_bf16(dY, dYt)
    ops.gemm_wgrad(dYt, Xt, dW, ws)
