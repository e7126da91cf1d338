"""ctypes binding of the C-ABI kernel library (include/clipself_hip.h) + a thin tensor-level wrapper.

PyTorch is used here only as plumbing: device allocation (`torch.empty(device='cuda')`), the current HIP stream
and `torch.distributed`.  Every op below is one call into libclipself_hip.so with raw device pointers.

There is NO fallback: if the library is missing or a tensor is not on the GPU the call raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import torch

_CSRC = Path(__file__).resolve().parent / "csrc"
_LIB_PATH = Path(os.environ["CLIPSELF_HIP_LIB"]) if os.environ.get("CLIPSELF_HIP_LIB") else _CSRC / "libclipself_hip.so"   # override: A/B of two builds

EPI_BF16, EPI_F32, EPI_RESID_F32, EPI_SWIGLU_BF16, EPI_ATOMIC_F32, EPI_PATCH_F32, EPI_RESID_LN_F32, EPI_GELU_BF16, EPI_QGELU_BF16 = range(9)
EPI_RELU_BF16 = 9                       # bf16 = ReLU(acc + bias): the detector box head's Linear + ReLU (linear.LinearAct)
EPI_THIN_FWD, EPI_THIN_DGRAD = 10, 11   # the thin forms, N <= 16: 1 x 1 convolutions of the RPN and mask heads and their input gradient (conv.Conv1x1Thin)
THIN_MAX_N = 16
EPI_THIN_WGRAD = 12                     # their weight and bias gradient: dW[N, K] = dY^T . X over the rows, db = column sums of dY (HipOps.thin_wgrad)
# epilogue 12's grid and workspace rule (include/clipself_hip.h), restated by thin_wgrad_workspace: a wave takes 32 rows per step, a workgroup
# 128, at most 2 workgroups per compute unit; every workgroup leaves one partial of N * K + 16 floats behind the 16 floats of db
THIN_WGRAD_STEP_ROWS, THIN_WGRAD_WG_ROWS, THIN_WGRAD_BLOCKS_PER_CU, THIN_WGRAD_HEAD = 32, 128, 2, 16
SPLITK_MAX, SPLITK_MIN_KTILES = 8, 16   # cs_gemm_nt's choice of `splits` for epilogues 0 / 9 (include/clipself_hip.h), restated by gemm_nt_splits
DX_BF16, DX_F32_ASSIGN, DX_F32_ACCUM = range(3)
ADAMW_GUARD_HEAD, ADAMW_GUARD_SPAN = 8, 16384

_vp, _i, _l, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t
_F32, _F32_BF16 = (torch.float32,), (torch.float32, torch.bfloat16)

# name -> (restype, argtypes), one table per public header; the Python constant beside a table restates a macro of that header (MACROS)
# include/clipself_hip.h: the engines
SIGNATURES = {
    "cs_last_error": (ctypes.c_char_p, []),
    "cs_gemm_nt": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_crop_resize_workspace": (_sz, [_i, _i, _i]),
    "cs_crop_resize_u8": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cs_quant_rows_fp8": (_i, [_vp, _l, _vp, _l, _vp, _i, _i, _vp]),
    "cs_gemm_nt_f8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_resize_bilinear_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "cs_gemm_wgrad_workspace": (_sz, [_i, _i, _i]),
    "cs_gemm_wgrad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_gemm_wgrad_tn_workspace": (_sz, [_i, _i, _i]),
    "cs_gemm_wgrad_tn": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_gemm_nt_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_gemm_nt_ln_split": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_ln_stats_finalize": (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "cs_attn_fwd_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "cs_layernorm_fwd": (_i, [_vp, _i, _l, _vp, _vp, _vp, _l, _vp, _vp, _i, _i, _f, _vp]),
    "cs_layernorm_fwd_q8": (_i, [_vp, _i, _l, _vp, _vp, _vp, _l, _vp, _vp, _vp, _l, _vp, _i, _i, _f, _vp]),
    "cs_layernorm_fwd_f32": (_i, [_vp, _l, _vp, _vp, _vp, _l, _vp, _vp, _i, _i, _f, _vp]),
    "cs_layernorm_bwd_workspace": (_sz, [_i, _i]),
    "cs_layernorm_bwd": (_i, [_vp, _l, _vp, _i, _l, _vp, _vp, _vp, _vp, _i, _l, _vp, _vp, _i, _vp, _vp, _l, _vp, _i, _i, _vp]),
    "cs_layernorm_bwd_q8": (_i, [_vp, _l, _vp, _i, _l, _vp, _vp, _vp, _vp, _i, _l, _vp, _vp, _i, _vp, _vp, _l, _vp, _vp, _l, _vp, _i, _i, _vp]),
    "cs_l2norm_fwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp]),
    "cs_l2norm_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "cs_attn_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "cs_attn_cls_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "cs_attn_query_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "cs_attn_bwd_workspace": (_sz, [_i, _i, _i, _i]),
    "cs_attn_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "cs_swiglu_fwd": (_i, [_vp, _l, _vp, _l, _i, _i, _vp]),
    "cs_swiglu_bwd": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _vp]),
    "cs_swiglu_bwd_colsum": (_i, [_vp, _l, _vp, _l, _vp, _l, _vp, _vp, _i, _i, _vp]),
    "cs_swiglu_bwd_q8": (_i, [_vp, _l, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _vp]),
    "cs_gelu_fwd": (_i, [_vp, _l, _vp, _l, _i, _i, _i, _vp]),
    "cs_gelu_bwd": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _vp]),
    "cs_cast_f32_bf16": (_i, [_vp, _vp, _l, _vp]),
    "cs_transpose_bf16": (_i, [_vp, _l, _vp, _l, _i, _i, _i, _i, _vp]),
    "cs_transpose_bf16_batched": (_i, [_vp, _i, _i, _vp]),
    "cs_colsum_workspace": (_sz, [_i, _i]),
    "cs_colsum_bf16": (_i, [_vp, _l, _vp, _vp, _i, _i, _vp]),
    "cs_im2row": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "cs_cls_row": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "cs_roialign_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _i, _f, _vp, _l, _vp, _vp, _l, _vp]),
    "cs_roialign_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cs_cosine_loss_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "cs_cosine_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _vp, _vp]),
    "cs_fed_bce_fwd": (_i, [_vp, _l, _vp, _vp, _vp, _i, _i, _f, _f, _vp]),
    "cs_fed_bce_bwd": (_i, [_vp, _l, _vp, _vp, _l, _i, _i, _f, _f, _vp, _vp]),
    "cs_num_compute_units": (_i, []),
    "cs_stream_create_cu_mask": (_i, [_i, _i, ctypes.POINTER(_vp)]),
    "cs_stream_destroy": (_i, [_vp]),
    "cs_adamw_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _f, _f, _f, _f, _f, _i, _f, _f, _i, _vp, _vp]),
}


class AttnExtra(ctypes.Structure):
    """include/clipself_hip.h: cs_attn_extra, the extra query rows of a cs_attn_bwd launch."""
    _fields_ = [("q", _vp), ("o", _vp), ("dout", _vp), ("lse", _vp), ("allow", _vp), ("dq", _vp), ("Q", _i), ("ldq", _i), ("ldo", _i), ("lddq", _i)]


# include/clipself_det.h: detector post-processing
DET_SIGNATURES = {
    "csd_nms_workspace": (_sz, [_i, _i, _i, _i]),
    "csd_nms": (_i, [_vp, _l, _vp, _l, _i, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csd_delta2bbox": (_i, [_vp, _l, _vp, _l, _vp, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _f, _vp, _vp, _vp, _l, _vp]),
}
DET_MAX_BOXES, DET_MAX_NUM = 16384, 4096                 # Kmax, max_num


class RoiLevel(ctypes.Structure):
    """include/clipself_roi.h: csr_level, one level of the RoI extractor's maps."""
    _fields_ = [("map", _vp), ("ld", _l), ("h", _i), ("w", _i), ("spatial_scale", _f)]


# include/clipself_roi.h: the detector's multi-level RoIAlign, forward and backward
ROI_SIGNATURES = {
    "csr_roi_extract_workspace": (_sz, [_i]),
    "csr_roi_extract_fwd": (_i, [ctypes.POINTER(RoiLevel), _i, _i, _i, _vp, _i, _i, _i, _f, _vp, _l, _vp]),
    "csr_roi_extract_bwd": (_i, [_vp, _l, _vp, _i, _i, _i, _f, ctypes.POINTER(RoiLevel), _i, _i, _i, _vp, _vp]),
}
ROI_MAX_LEVELS, ROI_MAX_SIDE, ROI_MAX_P, ROI_MAX_SR = 4, 512, 14, 8


# include/clipself_assign.h: the detector's training targets (IoU assignment, sampling, box deltas)
_f4 = ctypes.POINTER(_f)
ASSIGN_SIGNATURES = {
    "csa_workspace": (_sz, [_i, _i, _i, _i]),
    "csa_assign": (_i, [_vp, _l, _vp, _i, _vp, _l, _vp, _i, _vp, _i, _i, _i, _f, _f, _f, _f, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "csa_sample": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "csa_targets": (_i, [_vp, _l, _vp, _i, _vp, _l, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f4, _f4, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
}
ASSIGN_MAX_ROWS, ASSIGN_MAX_GT, ASSIGN_MAX_NUM = 1 << 20, 1024, 4096       # Nmax, Gmax, num


class LossLevel(ctypes.Structure):
    """include/clipself_loss.h: csl_level, one level of the RPN's predictions and their gradients."""
    _fields_ = [("cls", _vp), ("reg", _vp), ("dcls", _vp), ("dreg", _vp), ("h", _i), ("w", _i)]


# include/clipself_loss.h: the detector's losses with their gradients (RPN and box head)
LOSS_SIGNATURES = {
    "csl_workspace": (_sz, [ctypes.POINTER(LossLevel), _i, _i, _i, _i]),
    "csl_rpn_loss": (_i, [ctypes.POINTER(LossLevel), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csl_bbox_head_loss": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
}
LOSS_MAX_LEVELS, LOSS_MAX_ANCHORS, LOSS_MAX_SIDE, LOSS_MAX_ROWS, LOSS_MAX_CLASSES = 8, 16, 512, 1 << 20, 4096


# include/clipself_mask.h: the detector's mask branch (mask targets, mask loss with gradient, mask paste)
MASK_SIGNATURES = {
    "csm_workspace": (_sz, [_i]),
    "csm_mask_target": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _l, _l, _i, _i, _vp, _vp]),
    "csm_mask_loss": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "csm_paste_masks": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
}
MASK_MAX_ROWS, MASK_MAX_GT, MASK_MAX_SIDE, MASK_MAX_MASK, MASK_MAX_CLASSES, MASK_MAX_IMAGE = 1 << 20, 1 << 24, 2048, 64, 4096, 16384


class RpnLevel(ctypes.Structure):
    """include/clipself_rpn.h: csp_level, one level of the RPN head's maps."""
    _fields_ = [("cls", _vp), ("reg", _vp), ("h", _i), ("w", _i)]


# include/clipself_rpn.h: RPN proposals (per-level top-k, decode, min-size filter)
RPN_SIGNATURES = {
    "csp_workspace": (_sz, [ctypes.POINTER(RpnLevel), _i, _i, _i, _i]),
    "csp_select": (_i, [ctypes.POINTER(RpnLevel), _i, _i, _i, _vp, _l, _i, _f4, _f4, _f, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
RPN_MAX_LEVELS, RPN_MAX_ANCHORS, RPN_MAX_SIDE, RPN_MAX_PRE, RPN_MAX_ROWS = 8, 16, 512, 4096, 16384


# include/clipself_conv.h: the detector heads' 3 x 3 convolutions (implicit GEMM, explicit matrix)
CONV_SIGNATURES = {
    "csc_conv3x3": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _vp]),
    "csc_im2col3x3": (_i, [_vp, _l, _vp, _l, _l, _l, _i, _i, _i, _i, _vp]),
}
CONV_MAX_ROWS = (1 << 31) - 512                          # N * H * W


# include/clipself_bn.h: batch norm (+ ReLU) on channel-last maps, forward and backward
BN_SIGNATURES = {
    "csb_row_parts": (_i, [_l, _i]),
    "csb_workspace": (_sz, [_l, _i]),
    "csb_stats": (_i, [_vp, _l, _i, _l, _i, _vp, _vp, _vp]),
    "csb_finalize": (_i, [_vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp]),
    "csb_apply": (_i, [_vp, _l, _i, _vp, _i, _vp, _l, _i, _l, _i, _vp]),
    "csb_bwd_reduce": (_i, [_vp, _l, _i, _vp, _l, _i, _vp, _i, _vp, _vp, _l, _i, _vp]),
    "csb_bwd_apply": (_i, [_vp, _l, _i, _vp, _l, _i, _vp, _i, _vp, _vp, _vp, _l, _i, _l, _i, _vp]),
}
BN_MAX_ROWS, BN_MAX_C, BN_MAX_RECORDS, BN_REC_EXTRA, BN_ST_EXTRA = (1 << 31) - 512, 65536, 4096, 4, 4


# The whole C ABI, one entry per public header: load_library binds these tables and tests/test_cabi_symbols.py holds every one of them,
# the structs and the macros against the header's text and the built library.  A new header is one more entry here, the include of
# that header in its source file, and nothing else.
ABI = {
    "clipself_hip.h": SIGNATURES, "clipself_det.h": DET_SIGNATURES, "clipself_roi.h": ROI_SIGNATURES, "clipself_assign.h": ASSIGN_SIGNATURES,
    "clipself_loss.h": LOSS_SIGNATURES, "clipself_mask.h": MASK_SIGNATURES, "clipself_rpn.h": RPN_SIGNATURES, "clipself_conv.h": CONV_SIGNATURES,
    "clipself_bn.h": BN_SIGNATURES,
}
STRUCTS = {"cs_attn_extra": AttnExtra, "csr_level": RoiLevel, "csl_level": LossLevel, "csp_level": RpnLevel}
MACROS = {
    "CS_ADAMW_GUARD_HEAD": ADAMW_GUARD_HEAD, "CS_ADAMW_GUARD_SPAN": ADAMW_GUARD_SPAN,
    "CSD_MAX_BOXES": DET_MAX_BOXES, "CSD_MAX_NUM": DET_MAX_NUM,
    "CSR_MAX_LEVELS": ROI_MAX_LEVELS, "CSR_MAX_SIDE": ROI_MAX_SIDE, "CSR_MAX_P": ROI_MAX_P, "CSR_MAX_SR": ROI_MAX_SR,
    "CSA_MAX_ROWS": ASSIGN_MAX_ROWS, "CSA_MAX_GT": ASSIGN_MAX_GT, "CSA_MAX_NUM": ASSIGN_MAX_NUM,
    "CSL_MAX_LEVELS": LOSS_MAX_LEVELS, "CSL_MAX_ANCHORS": LOSS_MAX_ANCHORS, "CSL_MAX_SIDE": LOSS_MAX_SIDE, "CSL_MAX_ROWS": LOSS_MAX_ROWS,
    "CSL_MAX_CLASSES": LOSS_MAX_CLASSES,
    "CSM_MAX_ROWS": MASK_MAX_ROWS, "CSM_MAX_GT": MASK_MAX_GT, "CSM_MAX_SIDE": MASK_MAX_SIDE, "CSM_MAX_MASK": MASK_MAX_MASK,
    "CSM_MAX_CLASSES": MASK_MAX_CLASSES, "CSM_MAX_IMAGE": MASK_MAX_IMAGE,
    "CSP_MAX_LEVELS": RPN_MAX_LEVELS, "CSP_MAX_ANCHORS": RPN_MAX_ANCHORS, "CSP_MAX_SIDE": RPN_MAX_SIDE, "CSP_MAX_PRE": RPN_MAX_PRE,
    "CSP_MAX_ROWS": RPN_MAX_ROWS,
    "CSC_MAX_ROWS": CONV_MAX_ROWS,
    "CSB_MAX_ROWS": BN_MAX_ROWS, "CSB_MAX_C": BN_MAX_C, "CSB_MAX_RECORDS": BN_MAX_RECORDS, "CSB_REC_EXTRA": BN_REC_EXTRA, "CSB_ST_EXTRA": BN_ST_EXTRA,
}


def library_path() -> Path:
    return _LIB_PATH


def build_library(force: bool = False) -> Path:
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        for o in _CSRC.glob("_obj_*.o"):
            o.unlink()
    subprocess.run(["bash", str(_CSRC / "build.sh")], check=True)
    return _LIB_PATH


_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise RuntimeError(
                f"{_LIB_PATH} is missing: build it with clipself_amd/csrc/build.sh (or __graft_entry__.build()). "
                "There is no CPU fallback for the CLIPSelf hot path.")
        lib = ctypes.CDLL(str(_LIB_PATH))
        for table in ABI.values():
            for name, (res, args) in table.items():
                fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
                fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(t) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise TypeError(f"unsupported dtype {t.dtype}")


def _readable(t, n) -> bool:
    """True when n elements from t's first one lie inside its storage (a kernel may fetch that many in whole vectors)."""
    return t is None or t.untyped_storage().nbytes() - t.storage_offset() * t.element_size() >= n * t.element_size()


class HipOps:
    """Tensor-level face of the C ABI.  Tensors are 2-D (rows, cols) views whose last stride is 1; row strides
    become the `ld*` arguments.  Outputs are written in place into caller-allocated tensors."""

    name = "hip"
    ATTN_EXTRA_QUERIES = True           # attn_query_fwd(lse=) / attn_bwd(extra=): mask-attention pooling is differentiable on this backend
    ATTN_CAUSAL = True                  # attn_query_fwd(allow=None): causal self-attention, what the text tower (encode_text) runs on
    ADAMW_GUARD = True                  # adamw_step(max_norm=, skip_nonfinite=, guard=): gradient norm, clipping and the non-finite-step skip on the device
    ATTN_NO_ROPE = True                 # attn_fwd / attn_fwd_stats / attn_cls_fwd / attn_bwd(cos=None, sin=None): no rotary embedding, any Ntok > 1
    TOKEN_TAPS = True                   # tokens_to_nchw: the residual stream after a block as a [B, C, h, w] map (encode_dense(taps=), the detector backbone)
    DECONV_ROWS = True                  # rows_to_nchw / nchw_to_rows: 2x2 transposed convolutions as GEMMs on token rows (neck.Deconv2x2)
    DET_POST = True                     # nms / delta2bbox: box decoding, class-aware NMS and the per-image cut on the device (det_post)
    ROI_EXTRACT = True                  # roi_extract_fwd / roi_extract_bwd: multi-level RoIAlign on channel-last maps, atomic-free backward (roi_extractor)
    ASSIGN = True                       # assign / sample / bbox_targets: IoU assignment, random sampling and box-delta targets on the device (det_targets)
    LOSS = True                         # rpn_loss / bbox_head_loss: the RPN's and the box head's losses with their gradients, one call per head (det_losses)
    MASK = True                         # mask_target / mask_loss / paste_masks: the mask branch's targets, loss with gradient and paste (det_masks)
    RPN = True                          # rpn_select: per-level top-k of the RPN maps, decode and min-size filter, the input of nms' group form (det_proposals)
    CONV3X3 = True                      # conv3x3 / im2col3x3: Conv2d(Cin, Cout, 3, padding=1) on channel-last rows as an implicit GEMM (conv.Conv3x3)
    BATCHNORM = True                    # bn_stats / bn_finalize / bn_apply / bn_bwd_reduce / bn_bwd_apply: batch norm (+ ReLU) on channel-last rows (norm_act.BatchNormAct2d)
    LINEAR_ACT = True                   # gemm_nt(epi=EPI_RELU_BF16, splits=, extra=workspace): Linear + ReLU with deterministic split-K (linear.LinearAct)
    FPN_TOPDOWN = True                  # upsample2x_add / pool2x: the FPN's top-down add and its adjoint on channel-last rows; Conv1x1 on gemm_nt (fpn.FPN)
    THIN_HEADS = True                   # thin_fwd / thin_dgrad: 1 x 1 convolutions with Cout <= 16 as streaming kernels, rows or NCHW planes out (conv.Conv1x1Thin, thin_heads)
    THIN_WGRAD = True                   # thin_wgrad: weight and bias gradient of the thin forms in one streaming launch, dY fp32 rows / planes and X read in place
    BOX_SCORES = True              # box_scores / roialign_fwd(box_scale=): pixel boxes pooled and scored against class embeddings in one launch (ov_head)

    def __init__(self):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("HipOps needs a ROCm device (torch.cuda.is_available() is False); no CPU fallback exists")
        # OR-ed into the flags of every GEMM call: bits 20-27 = compute units the persistent GEMM kernels leave free.  Two callers
        # withhold CUs: training/distributed.py (a few for RCCL's reduction kernels while gradient buckets are in flight) and the
        # single-GPU tower partition of training/clipself.py (the frozen teacher's prefetched pass leaves `share` CUs to the student,
        # whose own persistent GEMMs are capped at `cap` workgroups meanwhile).
        self.gemm_flags = 0
        self._rccl_reserve = 0          # reserve_compute_units()
        self._share = 0                 # share_compute_units(): CUs given to the other tower, added to the RCCL reserve
        self._cap = 0                   # cap_compute_units(): upper bound of a persistent grid (0 = none)
        self.num_cus = int(self.lib.cs_num_compute_units())

    def _update_flags(self):
        n = self._rccl_reserve + self._share
        if self._cap:
            n = max(n, self.num_cus - self._cap)
        # a ValueError, not an assert (python -O), and at the call that asked for it: the field of the GEMM flags has 8 bits, and a
        # persistent grid keeps at least 8 workgroups (one per XCD)
        if not (0 <= n <= self.num_cus - 8 and n < 256):
            raise ValueError(f"persistent GEMM grids keep at least 8 workgroups and can leave at most 255 compute units free "
                             f"(asked to leave {n} of {self.num_cus} CUs: RCCL reserve {self._rccl_reserve}, tower share {self._share}, cap {self._cap})")
        self.gemm_flags = (self.gemm_flags & ~(255 << 20)) | (int(n) << 20)

    def reserve_compute_units(self, n: int):
        """Persistent GEMM grids leave n compute units free from now on (0 = none): room for RCCL's kernels in data-parallel runs."""
        self._rccl_reserve = int(n)
        self._update_flags()

    def share_compute_units(self, n: int):
        """... and n more for the other tower of the step (the frozen teacher's side of the single-GPU partition)."""
        self._share = int(n)
        self._update_flags()

    def cap_compute_units(self, n: int):
        """Persistent GEMM grids use at most n workgroups (0 = no cap): the student's side of the partition."""
        self._cap = int(n)
        self._update_flags()

    def persistent_grid(self) -> int:
        """Workgroups a persistent GEMM launches under the current reservation (diagnostics, tests)."""
        return self.num_cus - ((self.gemm_flags >> 20) & 255)

    def num_compute_units(self) -> int:
        return self.num_cus

    def stream_create_cu_mask(self, first_cu: int, n_cus: int):
        """torch stream whose kernels run on compute units [first_cu, first_cu + n_cus) only (cs_stream_create_cu_mask)."""
        h = ctypes.c_void_p()
        self._ok(self.lib.cs_stream_create_cu_mask(int(first_cu), int(n_cus), ctypes.byref(h)), "cs_stream_create_cu_mask")
        s = torch.cuda.ExternalStream(h.value)
        s._cs_handle = h.value
        return s

    def stream_destroy(self, stream):
        torch.cuda.synchronize()
        self._ok(self.lib.cs_stream_destroy(ctypes.c_void_p(stream._cs_handle)), "cs_stream_destroy")

    # -- helpers ---------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _ok(self, rc, who):
        if rc != 0:
            raise RuntimeError(f"{who} failed ({rc}): {self.lib.cs_last_error().decode()}")

    @staticmethod
    def _chk(*ts):
        for t in ts:
            if t is not None and not t.is_cuda:
                raise RuntimeError("HipOps received a non-GPU tensor; the hot path has no CPU fallback")

    # The two layouts the detector headers state, and their workspaces.  ValueError, not assert: these are user-facing limits.
    @staticmethod
    def _dense(t, dtype, shape, who):
        """A dense tensor of this dtype and shape on the device."""
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{who} must be a contiguous {dtype} device tensor {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

    @staticmethod
    def _rows(t, dtypes, M, C, who, k=None, a=1):
        """Rows [M, C] (None: any) of one of `dtypes` with last stride 1 -> the row stride: the tensor's, or at least C where M <= 1 leaves
        it free.  k: the stride must be a multiple of k that holds C (an int, or one per dtype); k=None: the library's to refuse.
        a: bytes the base is aligned to."""
        sh, st = t.shape, t.stride()
        if len(sh) != 2 or t.dtype not in dtypes or (M is not None and sh[0] != M) or (C is not None and sh[1] != C) or (sh[0] and st[1] != 1):
            raise ValueError(f"{who} must be {' / '.join(str(d) for d in dtypes)} rows [{M}, {C}] with last stride 1, "
                             f"got {t.dtype} {tuple(sh)} strides {st}")
        m, c = sh
        ld = st[0] if m > 1 else max(st[0], c)
        if k is not None:
            if k.__class__ is not int:
                k = k[dtypes.index(t.dtype)]
            if ld < c or ld % k:
                raise ValueError(f"{who}: row stride {ld} must be a multiple of {k} that holds {c} columns")
        if a > 1 and t.data_ptr() % a:
            raise ValueError(f"{who}: the base must be {a}-byte aligned")
        return ld

    def _workspace(self, header, need, device, workspace, who):
        """`need` bytes of 16-byte aligned workspace for an entry point of `header`: the caller's `workspace`, or this object's one
        grow-only buffer per (header, device) -- so calls that share it must share a stream.  The size is checked either way;
        need == 0 is the library's answer for shapes outside the header's limits."""
        if need <= 0:
            raise ValueError(f"{who}: the shapes are outside the limits of include/{header}")
        own = workspace is None
        if own:
            try:
                workspace = self._ws[header, device]
            except (AttributeError, KeyError):
                pass
        have = 0 if workspace is None else workspace.numel() * workspace.element_size()
        if own and have < need:
            workspace = self.__dict__.setdefault("_ws", {})[header, device] = torch.empty(need, dtype=torch.uint8, device=device)
            have = need
        if have < need or workspace.data_ptr() % 16:
            raise ValueError(f"{who}: workspace holds {have} bytes, {need} (16-byte aligned) are needed")
        return workspace

    def _size(self, fn, *args):
        """fn(*args) bytes, remembered: the library's size functions are pure, and a ctypes call costs as much as a wrapper's other checks
        together (these wrappers run several times per layer and step).  A few thousand integers at the most."""
        try:
            return self._sizes[fn, args]
        except (AttributeError, KeyError):
            sizes = self.__dict__.setdefault("_sizes", {})
            if len(sizes) >= 4096:
                sizes.clear()
            need = sizes[fn, args] = int(getattr(self.lib, fn)(*args))
            return need

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device="cuda")

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    # -- ops -------------------------------------------------------------------------------------
    def gemm_nt(self, A, B, C, bias=None, extra=None, epi=EPI_BF16, splits=1, group=0, flags=0):
        self._chk(A, B, C, bias, extra)
        M, K = A.shape
        N = B.shape[0]
        assert B.shape[1] == K and A.stride(1) == 1 and B.stride(1) == 1 and C.stride(-1) == 1
        if extra is not None and epi in (EPI_RESID_F32, EPI_PATCH_F32):
            assert extra.stride(0) == C.stride(0), "extra must share C's row stride"
        if epi in (EPI_BF16, EPI_RELU_BF16) and splits != 1 and extra is not None:
            # split-K through partials: `extra` is the fp32 workspace.  Its size is checked here (the library sees a pointer); a missing or
            # misaligned one is the library's to refuse
            s = splits if splits > 0 else self.gemm_nt_splits(M, N, K)
            if s > 1 and (extra.dtype != torch.float32 or not extra.is_contiguous() or extra.numel() < s * M * N):
                raise ValueError(f"gemm_nt: split-K with {s} slices needs a contiguous fp32 workspace of {s} * {M} * {N} = {s * M * N} "
                                 f"floats in `extra`, got {extra.dtype} with {extra.numel()} elements")
        self._ok(self.lib.cs_gemm_nt(_p(A), _p(B), _p(C), _p(bias), _p(extra), M, N, K, A.stride(0), B.stride(0),
                                     C.stride(0), epi, splits, group, flags | self.gemm_flags, self._stream()), "cs_gemm_nt")

    @staticmethod
    def _thin_form(krows, W, thin, thin2, R, split):
        """Checks shared by thin_fwd / thin_dgrad / thin_wgrad -> (M, N, K, the `group`, the stride-or-split argument, flags) of cs_gemm_nt's
        thin forms (include/clipself_hip.h).  krows: the K-wide rows (X / dX); W: the bf16 weights [N, K], or the int N where the form has
        none (thin_wgrad); thin: the N-wide side -- rows [M, N] for R == 0, else the first plane block, contiguous with M * split elements;
        thin2: the second block (M * (N - split) elements) or None."""
        assert krows.dim() == 2 and krows.stride(1) == 1 and krows.dtype in (torch.float32, torch.bfloat16)
        assert thin.dtype == torch.float32
        M, K = krows.shape
        if isinstance(W, int):
            N = W
        else:
            assert W.dim() == 2 and W.stride(1) == 1 and W.dtype == torch.bfloat16 and W.shape[1] == K
            N = W.shape[0]
        assert 1 <= N <= THIN_MAX_N and K % 64 == 0 and M >= 1 and krows.stride(0) >= K
        flags = 1 if krows.dtype == torch.float32 else 0
        if R == 0:
            assert split is None and thin2 is None, "rows form: one [M, N] tensor, no split"
            assert thin.dim() == 2 and tuple(thin.shape) == (M, N) and thin.stride(1) == 1 and (thin.stride(0) >= N or M == 1)
            return M, N, K, 0, max(thin.stride(0), N), flags
        s = N if split is None else int(split)
        assert R >= 1 and M % R == 0 and 1 <= s <= N
        assert thin.is_contiguous() and thin.numel() == M * s, "planes form: the first block is [M / R, s, R], contiguous"
        if thin2 is None:
            assert s == N, "planes form: a split below N needs the second block"
        else:
            assert s < N and thin2.dtype == torch.float32 and thin2.is_contiguous() and thin2.numel() == M * (N - s)
        return M, N, K, int(R), s, flags

    def thin_fwd(self, X, W, bias, out, R=0, split=None):
        """Epilogue 10 of cs_gemm_nt: Y[m, n] = bias[n] + sum_k bf16(X[m, k]) * W[n, k], N <= 16, fp32 out.  X bf16 / fp32 rows [M, K] (row
        stride >= K), W bf16 [N, K], bias fp32 [N] or None.  R == 0: out is rows [M, N] (row stride >= N).  R >= 1 (pixels per image, M % R
        == 0): out is ONE contiguous fp32 allocation of M * N elements, the NCHW tensors [M / R, split, R] and [M / R, N - split, R] one
        behind the other (split None = N: one tensor)."""
        self._chk(X, W, bias, out)
        if R == 0:
            M, N, K, group, ldc, flags = self._thin_form(X, W, out, None, 0, split)
        else:
            assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == X.shape[0] * W.shape[0]
            s = W.shape[0] if split is None else int(split)
            flat = out.reshape(-1)
            M, N, K, group, ldc, flags = self._thin_form(X, W, flat[:X.shape[0] * s], flat[X.shape[0] * s:] if s < W.shape[0] else None, R, s)
        assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N)
        self._ok(self.lib.cs_gemm_nt(_p(X), _p(W), _p(out), _p(bias), None, M, N, K, X.stride(0), W.stride(0), ldc, EPI_THIN_FWD, 1, group,
                                     flags, self._stream()), "cs_gemm_nt")

    def thin_dgrad(self, dY, W, dX, R=0, dY2=None, gate=None):
        """Epilogue 11: dX[m, k] = gate(m, k) * sum_n bf16(dY[m, n]) * W[n, k].  dY fp32: rows [M, N] (R == 0), or contiguous planes
        [M / R, s, R] with the second block dY2 [M / R, N - s, R] (s = dY.numel() / M; None: s == N).  dX bf16 / fp32 rows [M, K] (row stride >=
        K), written whole.  gate: bf16 rows [M, K] with dX's row stride; where gate <= 0, dX = 0 (a NaN gate passes)."""
        self._chk(dY, W, dX, dY2, gate)
        split = None if R == 0 else dY.numel() // dX.shape[0]
        M, N, K, group, lda, flags = self._thin_form(dX, W, dY, dY2, R, split)
        if gate is not None:
            assert gate.dtype == torch.bfloat16 and tuple(gate.shape) == (M, K) and gate.stride(1) == 1 and (gate.stride(0) == dX.stride(0) or M == 1), \
                "the gate is bf16 rows [M, K] with dX's row stride"
        self._ok(self.lib.cs_gemm_nt(_p(dY), _p(W), _p(dX), _p(dY2), _p(gate), M, N, K, lda, W.stride(0), dX.stride(0), EPI_THIN_DGRAD, 1, group,
                                     flags, self._stream()), "cs_gemm_nt")

    def thin_wgrad_partials(self, M) -> int:
        """Workgroups along the rows of epilogue 12 (each leaves one partial): min(ceil(M / 128), 2 * compute units)."""
        return min((M + THIN_WGRAD_WG_ROWS - 1) // THIN_WGRAD_WG_ROWS, THIN_WGRAD_BLOCKS_PER_CU * self.num_cus)

    def thin_wgrad_workspace(self, M, N, K) -> int:
        """Floats of epilogue 12's workspace (the rule of include/clipself_hip.h): 16 + P * (N * K + 16), P = thin_wgrad_partials(M)."""
        return THIN_WGRAD_HEAD + self.thin_wgrad_partials(M) * (N * K + THIN_WGRAD_HEAD)

    def thin_wgrad(self, dY, X, dW, db=None, R=0, dY2=None, workspace=None):
        """Epilogue 12: dW[n, k] = sum_m bf16(dY[m, n]) * bf16(X[m, k]) (overwritten, fp32 [N, K], row stride >= K) and db[n] = sum_m
        bf16(dY[m, n]).  dY fp32 as in thin_dgrad: rows [M, N] (R == 0) or contiguous planes [M / R, s, R] with the second block dY2.  X bf16
        / fp32 rows [M, K], read in place.  workspace: fp32, contiguous, at least thin_wgrad_workspace(M, N, K) floats (allocated when None;
        ValueError when too small); on return workspace[:N] holds db, which is copied into `db` when one is given.  -> the workspace."""
        self._chk(dY, X, dW, db, dY2, workspace)
        M, K = X.shape
        N = dY.shape[1] if R == 0 else (dY.numel() + (0 if dY2 is None else dY2.numel())) // M
        assert dW.dim() == 2 and dW.dtype == torch.float32 and dW.stride(1) == 1 and dW.shape[1] >= K and dW.shape[0] >= N, \
            "dW is fp32 [>= N, >= K] with unit column stride"
        split = None if R == 0 else dY.numel() // M
        M, N, K, group, lda, flags = self._thin_form(X, int(N), dY, dY2, R, split)
        need = self.thin_wgrad_workspace(M, N, K)
        if workspace is None:
            workspace = self.empty((need,), torch.float32)
        elif workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() < need:
            raise ValueError(f"thin_wgrad: M={M}, N={N}, K={K} needs a contiguous fp32 workspace of {need} floats, got {workspace.dtype} with "
                             f"{workspace.numel()} elements")
        self._ok(self.lib.cs_gemm_nt(_p(dY), _p(X), _p(dW), _p(dY2), _p(workspace), M, N, K, lda, X.stride(0), dW.stride(0), EPI_THIN_WGRAD, 1,
                                     group, flags, self._stream()), "cs_gemm_nt")
        if db is not None:
            assert db.dtype == torch.float32 and db.numel() == N
            db.view(-1).copy_(workspace[:N])
        return workspace

    def gemm_nt_splits(self, M, N, K) -> int:
        """The slice count cs_gemm_nt chooses for splits <= 0 on epilogues 0 / 9 (the rule of include/clipself_hip.h): what a caller sizes the
        workspace with.  1 = the plain call, no workspace."""
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        s = 1
        while s < SPLITK_MAX and tiles * 2 * s <= self.num_cus and (K // 64) // (2 * s) >= SPLITK_MIN_KTILES:
            s *= 2
        return s

    def gemm_nt_ln(self, A, B, C, bias=None, extra=None, ln_mean=None, ln_rstd=None, ln_colsum=None, stats_part=None, xb_out=None,
                   epi=EPI_RESID_LN_F32, group=0, flags=0):
        self._chk(A, B, C, bias, extra, ln_mean, ln_rstd, ln_colsum, stats_part, xb_out)
        M, K = A.shape
        N = B.shape[0]
        assert B.shape[1] == K and A.stride(1) == 1 and B.stride(1) == 1 and C.stride(-1) == 1
        if extra is not None and epi in (EPI_RESID_F32, EPI_RESID_LN_F32):
            assert extra.stride(0) == C.stride(0), "extra must share C's row stride"
        if stats_part is not None:
            slices = 4 * ((group + 127) // 128) if epi == EPI_SWIGLU_BF16 else (N + 63) // 64
            assert stats_part.is_contiguous() and stats_part.shape[0] >= slices and stats_part.shape[1] == M
        if xb_out is not None:
            assert xb_out.dtype == torch.bfloat16 and xb_out.stride(1) == 1 and xb_out.shape[0] == M
        self._ok(self.lib.cs_gemm_nt_ln(_p(A), _p(B), _p(C), _p(bias), _p(extra), _p(ln_mean), _p(ln_rstd), _p(ln_colsum), _p(stats_part),
                                        _p(xb_out), xb_out.stride(0) if xb_out is not None else 0, M, N, K, A.stride(0), B.stride(0),
                                        C.stride(0), epi, 1, group, flags | self.gemm_flags, self._stream()), "cs_gemm_nt_ln")

    def gemm_nt_ln_split(self, A, B, hi, lo, bias, ln_mean, ln_rstd, ln_colsum, x_in=None, x_out=None, stats_part=None, flags=0):
        """Folded-LayerNorm residual GEMM on the split stream (cs_gemm_nt_ln_split): x += rstd * (A.B^T - mean * colsum) + bias with x held as
        the 16-bit planes hi (bf16 view of x, the next folded GEMM's operand) and lo (int16) -- or read from x_in / written to x_out (fp32)
        at the two ends of the tower."""
        self._chk(A, B, hi, lo, bias, ln_mean, ln_rstd, ln_colsum, x_in, x_out, stats_part)
        M, K = A.shape
        N = B.shape[0]
        assert hi.dtype == torch.bfloat16 and lo.dtype == torch.int16 and hi.shape == (M, N) and lo.shape == (M, N)
        assert hi.stride(1) == 1 and lo.stride(1) == 1 and hi.stride(0) == lo.stride(0) and hi.stride(0) % 8 == 0
        assert x_out is None or stats_part is None, "fp32 out: hi / lo are only read, no statistics epilogue"
        x = x_in if x_in is not None else x_out
        assert x is None or (x.dtype == torch.float32 and x.shape == (M, N) and x.stride(1) == 1)
        self._ok(self.lib.cs_gemm_nt_ln_split(_p(A), _p(B), _p(bias), _p(ln_mean), _p(ln_rstd), _p(ln_colsum), _p(x_in), _p(x_out), _p(hi), _p(lo),
                                              hi.stride(0), _p(stats_part), M, N, K, A.stride(0), B.stride(0), x.stride(0) if x is not None else N,
                                              flags | self.gemm_flags, self._stream()), "cs_gemm_nt_ln_split")

    def quant_rows_fp8(self, x, q, scale):
        """bf16 [M,K] -> e4m3 bytes q [M,Kp] (uint8 / float8 storage, Kp = K rounded up to 128, padding zeroed) + fp32 row scales [M]."""
        self._chk(x, q, scale)
        M, K = x.shape
        assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and q.element_size() == 1 and q.stride(1) == 1 and q.shape[1] == (K + 127) // 128 * 128
        self._ok(self.lib.cs_quant_rows_fp8(_p(x), x.stride(0), _p(q), q.stride(0), _p(scale), M, K, self._stream()), "cs_quant_rows_fp8")

    def gemm_nt_f8(self, A8, B8, C, row_scale, col_scale, bias=None, extra=None, epi=EPI_BF16, flags=0):
        """C = row_scale[m] * col_scale[n] * (A8 . B8^T) + bias (+ extra): e4m3 operands [M,Kp] / [N,Kp] from quant_rows_fp8."""
        self._chk(A8, B8, C, row_scale, col_scale, bias, extra)
        M, K8 = A8.shape
        N = B8.shape[0]
        assert B8.shape[1] == K8 and A8.element_size() == 1 and B8.element_size() == 1 and C.stride(-1) == 1
        if extra is not None:
            assert extra.stride(0) == C.stride(0), "extra must share C's row stride"
        self._ok(self.lib.cs_gemm_nt_f8(_p(A8), _p(B8), _p(C), _p(bias), _p(extra), _p(row_scale), _p(col_scale), M, N, K8, A8.stride(0), B8.stride(0),
                                        C.stride(0), epi, flags | self.gemm_flags, self._stream()), "cs_gemm_nt_f8")

    def crop_resize(self, image_u8, boxes, size, pad_center=True, mean=(0.48145466, 0.4578275, 0.40821073),
                    std=(0.26862954, 0.26130258, 0.27577711), out=None):
        """image_u8 [H,W,3] uint8 on the GPU, boxes [K,4] f32 pixel xyxy -> [K,3,size,size] f32: crop, Pillow-exact bicubic resize of
        the longest side to `size`, zero pad (centred or right/bottom), /255, normalise (defaults: the OpenAI CLIP statistics)."""
        self._chk(image_u8, boxes, out)
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[2] == 3 and image_u8.is_contiguous()
        boxes = boxes.to(torch.float32).contiguous()
        H, W, K = image_u8.shape[0], image_u8.shape[1], boxes.shape[0]
        if out is None:
            out = torch.empty((K, 3, size, size), dtype=torch.float32, device=image_u8.device)
        need = max(int(self.lib.cs_crop_resize_workspace(H, K, size)), 16)           # K == 0 needs none and is no error
        ws = self._workspace("clipself_hip.h", need, image_u8.device, None, "crop_resize")
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        self._ok(self.lib.cs_crop_resize_u8(_p(image_u8), H, W, _p(boxes), K, size, int(bool(pad_center)), m3, s3, _p(out), _p(ws),
                                            self._stream()), "cs_crop_resize_u8")
        return out

    def resize_bilinear(self, x, size):
        """x fp32 [B,C,H,W] -> [B,C,size,size], torch's bilinear / align_corners=False arithmetic (the --multiscale resize)."""
        self._chk(x)
        assert x.dtype == torch.float32 and x.dim() == 4
        x = x.contiguous()
        B, C, H, W = x.shape
        out = torch.empty((B, C, size, size), dtype=torch.float32, device=x.device)
        self._ok(self.lib.cs_resize_bilinear_f32(_p(x), _p(out), B * C, H, W, size, size, self._stream()), "cs_resize_bilinear_f32")
        return out

    def gemm_wgrad_workspace(self, M, N, K) -> int:
        return int(self.lib.cs_gemm_wgrad_workspace(M, N, K))

    def gemm_wgrad(self, A, B, dW, workspace):
        """dW[M,N] += A[M,K] . B[N,K]^T (split-K through `workspace`, a uint8/any buffer of >= gemm_wgrad_workspace bytes)."""
        self._chk(A, B, dW, workspace)
        M, K = A.shape
        N = B.shape[0]
        assert B.shape[1] == K and A.stride(1) == 1 and B.stride(1) == 1 and dW.stride(1) == 1 and dW.dtype == torch.float32
        assert workspace.numel() * workspace.element_size() >= self.gemm_wgrad_workspace(M, N, K)
        self._ok(self.lib.cs_gemm_wgrad(_p(A), _p(B), _p(dW), _p(workspace), M, N, K, A.stride(0), B.stride(0), dW.stride(0),
                                        self._stream()), "cs_gemm_wgrad")

    def gemm_wgrad_tn_workspace(self, N, K, tokens) -> int:
        """Bytes of workspace for gemm_wgrad_tn, 0 when the shape is outside its coverage (take the transposing path then)."""
        return int(self.lib.cs_gemm_wgrad_tn_workspace(N, K, tokens))

    def gemm_wgrad_tn(self, dY, X, dW, workspace):
        """dW[N,K] += dY[tokens,N]^T . X[tokens,K] from the token-major operands (no transposed copies)."""
        self._chk(dY, X, dW, workspace)
        T, N = dY.shape
        K = X.shape[1]
        assert X.shape[0] == T and dY.stride(1) == 1 and X.stride(1) == 1 and dW.stride(1) == 1 and dW.dtype == torch.float32
        assert workspace.numel() * workspace.element_size() >= self.gemm_wgrad_tn_workspace(N, K, T) > 0
        rc = self.lib.cs_gemm_wgrad_tn(_p(dY), _p(X), _p(dW), _p(workspace), N, K, T, dY.stride(0), X.stride(0), dW.stride(0), self._stream())
        if rc == 1:
            raise RuntimeError("cs_gemm_wgrad_tn: shape outside the kernel's coverage (check gemm_wgrad_tn_workspace first)")
        self._ok(rc, "cs_gemm_wgrad_tn")

    def ln_stats_finalize(self, part, npp, C, mean, rstd, eps=1e-6):
        self._chk(part, mean, rstd)
        P, M = part.shape[0], part.shape[1]
        assert part.is_contiguous() and part.shape[2] == 2
        self._ok(self.lib.cs_ln_stats_finalize(_p(part), P, npp, C, M, eps, _p(mean), _p(rstd), self._stream()), "cs_ln_stats_finalize")

    def _check_rope_tables(self, cos, sin, Ntok):
        """The rotary tables must have the layout rope.py:118-142 builds (one `freqs` tensor, repeated for the pair, broadcast over rows and
        columns): for a g x g grid, dims [0, 32) of token (r, c) depend on r only, dims [32, 64) on c only (the forward kernels read the tables
        separably), the row part of grid row i equals the column part of grid column i, and the two dims of a rotation pair share their entry.
        The C ABI documents this as a precondition (include/clipself_hip.h); this wrapper checks it once per table tensor (a few reductions
        and one host read-back) and raises instead of letting a kernel return wrong numbers."""
        def ver(t):
            try:
                return t._version
            except RuntimeError:               # inference tensors carry no version counter
                return -1
        key = (cos.data_ptr(), sin.data_ptr(), ver(cos), ver(sin), Ntok)
        seen = self.__dict__.setdefault("_rope_ok", set())
        if key in seen:
            return
        g = int(round((Ntok - 1) ** 0.5))
        if g * g != Ntok - 1 or tuple(cos.shape) != (Ntok - 1, 64) or tuple(sin.shape) != (Ntok - 1, 64):
            raise ValueError(f"rotary tables must be [g*g, 64] for a square token grid, got {tuple(cos.shape)} for {Ntok} tokens")
        for t in (cos, sin):
            v = t.view(g, g, 64)
            ok = (torch.equal(v[:, :, :32], v[:, :1, :32].expand(g, g, 32)) and torch.equal(v[:, :, 32:], v[:1, :, 32:].expand(g, g, 32))
                  and torch.equal(v[:, 0, :32], v[0, :, 32:]) and torch.equal(v[..., 0::2], v[..., 1::2]))
            if not ok:
                raise ValueError("rotary tables are not in the layout of rope.py:118-142 (separable, row part == column part, one entry per "
                                 "rotation pair): the attention kernels cannot read them")
        if len(seen) > 64:
            seen.clear()
        seen.add(key)

    @staticmethod
    def _no_rope(cos, sin, who) -> bool:
        """True for cos is None and sin is None: the form without rotary embedding (NULL tables in the C ABI; the outputs equal those of
        identity tables by value).  One table without the other is an error here, before any launch."""
        if (cos is None) != (sin is None):
            raise ValueError(f"{who}: cos and sin are given together, or both None (no rotary embedding)")
        return cos is None

    def attn_fwd_stats(self, qkv, cos, sin, out, lse, stats_part, B, Ntok, H, scale):
        self._chk(qkv, cos, sin, out, lse, stats_part)
        if not self._no_rope(cos, sin, "attn_fwd_stats"):
            self._check_rope_tables(cos, sin, Ntok)
        assert stats_part.is_contiguous() and tuple(stats_part.shape) == (H, B * Ntok, 2)
        self._ok(self.lib.cs_attn_fwd_stats(_p(qkv), _p(cos), _p(sin), _p(out), _p(lse), _p(stats_part), B, Ntok, H, qkv.stride(0),
                                            out.stride(0), scale, self._stream()), "cs_attn_fwd_stats")

    @staticmethod
    def _ln_pad(C, *params):
        """C % 4 != 0 (padded rows): the kernels fetch gamma / beta in 16-byte pieces, so these must be readable up to the next multiple of 4
        (include/clipself_hip.h, cs_layernorm_fwd); what the extra elements hold is ignored."""
        if C % 4:
            assert all(_readable(t, (C + 3) // 4 * 4) for t in params), "LayerNorm with C % 4 != 0: gamma / beta must be readable up to roundup4(C)"

    def layernorm_fwd(self, x, gamma, beta, y, mean=None, rstd=None, eps=1e-6, q8=None, q_scale=None):
        if q8 is not None:
            return self.layernorm_fwd_q8(x, gamma, beta, y, q8, q_scale, mean, rstd, eps)
        self._chk(x, gamma, beta, y, mean, rstd)
        M, C = x.shape
        self._ln_pad(C, gamma, beta)
        self._ok(self.lib.cs_layernorm_fwd(_p(x), _dt(x), x.stride(0), _p(gamma), _p(beta), _p(y), y.stride(0) if y is not None else 0,
                                           _p(mean), _p(rstd), M, C, eps, self._stream()), "cs_layernorm_fwd")

    def layernorm_fwd_q8(self, x, gamma, beta, y, q8, q_scale, mean=None, rstd=None, eps=1e-6):
        """LayerNorm forward that also writes the e4m3 copy of y for the fp8 GEMM: q8 [M, Kp] (1-byte elements, Kp >= C rounded up to 128,
        padding zero) + q_scale [M]; bit-identical to quant_rows_fp8(y)."""
        self._chk(x, gamma, beta, y, mean, rstd, q8, q_scale)
        M, C = x.shape
        assert q8.element_size() == 1 and q8.stride(1) == 1 and q8.shape[1] >= (C + 127) // 128 * 128 and q_scale is not None and y is not None
        self._ln_pad(C, gamma, beta)
        self._ok(self.lib.cs_layernorm_fwd_q8(_p(x), _dt(x), x.stride(0), _p(gamma), _p(beta), _p(y), y.stride(0), _p(mean), _p(rstd),
                                              _p(q8), q8.stride(0), _p(q_scale), M, C, eps, self._stream()), "cs_layernorm_fwd_q8")

    def layernorm_fwd_f32(self, x, gamma, beta, y, mean=None, rstd=None, eps=1e-5):
        """fp32 rows -> fp32 rows (ln_pre of the OpenAI-CLIP ViT: its output is the residual stream)."""
        self._chk(x, gamma, beta, y, mean, rstd)
        M, C = x.shape
        assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.stride(1) == 1 and y.stride(1) == 1
        assert x.data_ptr() != y.data_ptr(), "layernorm_fwd_f32 is out of place"
        self._ok(self.lib.cs_layernorm_fwd_f32(_p(x), x.stride(0), _p(gamma), _p(beta), _p(y), y.stride(0), _p(mean), _p(rstd), M, C, eps,
                                               self._stream()), "cs_layernorm_fwd_f32")

    def layernorm_bwd_workspace(self, M, C) -> int:
        return int(self.lib.cs_layernorm_bwd_workspace(M, C))

    def layernorm_bwd_q8(self, dy, x, gamma, mean, rstd, dx, dx_mode, dgamma, dbeta, accumulate, workspace, dx_copy, copy_colsum, q8, q_scale):
        """layernorm_bwd whose bf16 copy also leaves as e4m3 bytes q8 [M, >= C rounded up to 128] + fp32 row scales (= quant_rows_fp8(dx_copy))."""
        self._chk(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, dx_copy, copy_colsum, q8, q_scale)
        M, C = x.shape
        assert dx_copy is not None and dx_copy.dtype == torch.bfloat16 and dx_copy.shape == (M, C) and dx_copy.stride(1) == 1
        self._ln_pad(C, gamma)
        assert q8.element_size() == 1 and q8.stride(1) == 1 and q8.shape[1] >= (C + 127) // 128 * 128 and q_scale is not None
        self._ok(self.lib.cs_layernorm_bwd_q8(_p(dy), dy.stride(0), _p(x), _dt(x), x.stride(0), _p(gamma), _p(mean), _p(rstd),
                                              _p(dx), dx_mode, dx.stride(0), _p(dgamma), _p(dbeta), int(accumulate),
                                              _p(workspace), _p(dx_copy), dx_copy.stride(0), _p(copy_colsum), _p(q8), q8.stride(0), _p(q_scale),
                                              M, C, self._stream()), "cs_layernorm_bwd_q8")

    def layernorm_bwd(self, dy, x, gamma, mean, rstd, dx, dx_mode, dgamma=None, dbeta=None, accumulate=False, workspace=None,
                      dx_copy=None, copy_colsum=None, q8=None, q_scale=None):
        """dx_copy (fp32 dx modes): bf16 copy of the updated dx rows; copy_colsum [C]: (+)= its column sums (a bias gradient);
        q8 / q_scale: the e4m3 copy of dx_copy as well (layernorm_bwd_q8)."""
        if q8 is not None:
            return self.layernorm_bwd_q8(dy, x, gamma, mean, rstd, dx, dx_mode, dgamma, dbeta, accumulate, workspace, dx_copy, copy_colsum,
                                         q8, q_scale)
        self._chk(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, dx_copy, copy_colsum)
        M, C = x.shape
        self._ln_pad(C, gamma)
        if dx_copy is not None:
            assert dx_copy.dtype == torch.bfloat16 and dx_copy.shape == (M, C) and dx_copy.stride(1) == 1
        self._ok(self.lib.cs_layernorm_bwd(_p(dy), dy.stride(0), _p(x), _dt(x), x.stride(0), _p(gamma), _p(mean), _p(rstd),
                                           _p(dx), dx_mode, dx.stride(0), _p(dgamma), _p(dbeta), int(accumulate),
                                           _p(workspace), _p(dx_copy), dx_copy.stride(0) if dx_copy is not None else 0, _p(copy_colsum),
                                           M, C, self._stream()), "cs_layernorm_bwd")

    def l2norm_fwd(self, x, y, inv_norm, eps=1e-12):
        self._chk(x, y, inv_norm)
        M, C = x.shape
        assert x.is_contiguous() and y.is_contiguous()
        self._ok(self.lib.cs_l2norm_fwd(_p(x), _p(y), _p(inv_norm), M, C, eps, self._stream()), "cs_l2norm_fwd")

    def l2norm_bwd(self, dy, y, inv_norm, dx):
        self._chk(dy, y, inv_norm, dx)
        M, C = y.shape
        assert dy.is_contiguous() and y.is_contiguous() and dx.is_contiguous()
        self._ok(self.lib.cs_l2norm_bwd(_p(dy), _p(y), _p(inv_norm), _p(dx), M, C, self._stream()), "cs_l2norm_bwd")

    def attn_fwd(self, qkv, cos, sin, out, lse, B, Ntok, H, scale):
        self._chk(qkv, cos, sin, out, lse)
        if not self._no_rope(cos, sin, "attn_fwd"):
            self._check_rope_tables(cos, sin, Ntok)
        self._ok(self.lib.cs_attn_fwd(_p(qkv), _p(cos), _p(sin), _p(out), _p(lse), B, Ntok, H, qkv.stride(0), out.stride(0),
                                      scale, self._stream()), "cs_attn_fwd")

    def attn_cls_fwd(self, q, kv, cos, sin, out, B, Ntok, H, scale):
        self._chk(q, kv, cos, sin, out)
        self._no_rope(cos, sin, "attn_cls_fwd")
        self._ok(self.lib.cs_attn_cls_fwd(_p(q), _p(kv), _p(cos), _p(sin), _p(out), B, Ntok, H, q.stride(0), kv.stride(0),
                                          out.stride(0), scale, self._stream()), "cs_attn_cls_fwd")

    def attn_query_fwd(self, q, kv, allow, out, B, Q, Ntok, H, scale, lse=None):
        """Q extra query rows per image against the image's keys / values; allow [B*Q, Ntok] uint8 (1 = may attend).  lse [B*H, Q] f32
        (optional): the rows' log-sum-exp over their allowed keys, what attn_bwd(extra=) needs.
        allow=None: causal self-attention of B sequences of Ntok <= 128 tokens (the text tower; Q == Ntok, no lse)."""
        self._chk(q, kv, allow, out, lse)
        if allow is None:
            assert Q == Ntok and lse is None and Ntok <= 128, "attn_query_fwd(allow=None) is causal self-attention: Q == Ntok <= 128, no lse"
            assert q.stride(1) == 1 and kv.stride(1) == 1 and out.stride(1) == 1 and q.shape[0] == B * Ntok == kv.shape[0] == out.shape[0]
            self._ok(self.lib.cs_attn_query_fwd(_p(q), _p(kv), None, _p(out), None, B, Q, Ntok, H, q.stride(0), kv.stride(0), out.stride(0),
                                                scale, self._stream()), "cs_attn_query_fwd")
            return
        assert allow.dtype == torch.uint8 and allow.is_contiguous() and tuple(allow.shape) == (B * Q, Ntok)
        assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * Q)
        self._ok(self.lib.cs_attn_query_fwd(_p(q), _p(kv), _p(allow), _p(out), _p(lse), B, Q, Ntok, H, q.stride(0), kv.stride(0), out.stride(0),
                                            scale, self._stream()), "cs_attn_query_fwd")

    def attn_bwd_workspace(self, B, Ntok, H, Q=0) -> int:
        return int(self.lib.cs_attn_bwd_workspace(B, Ntok, H, Q))

    def _check_identity_tables(self, cos, sin):
        """Extra query rows exist in the family without rotary embedding only: cos = 1, sin = 0 (checked once per table tensor)."""
        key = ("ident", cos.data_ptr(), sin.data_ptr(), tuple(cos.shape))
        seen = self.__dict__.setdefault("_rope_ok", set())
        if key in seen:
            return
        if not (bool((cos == 1).all()) and bool((sin == 0).all())):
            raise ValueError("attn_bwd(extra=...): extra query rows are not rotated, so the rotary tables must be the identity (cos 1, sin 0)")
        seen.add(key)

    def attn_bwd(self, qkv, o, dout, lse, cos, sin, dqkv, workspace, B, Ntok, H, scale, extra=None):
        """extra: dict(q, o, dout, lse, allow, dq, Q) -- the extra query rows of the launch (cs_attn_extra); o / dout / lse may then be None.
        cos = sin = None: no rotary embedding (with extra rows the tables must be the identity or None, which mean the same)."""
        self._chk(qkv, o, dout, lse, cos, sin, dqkv, workspace)
        no_rope = self._no_rope(cos, sin, "attn_bwd")
        assert qkv.stride(0) == dqkv.stride(0)
        if extra is None:
            assert o.stride(0) == dout.stride(0)
            self._ok(self.lib.cs_attn_bwd(_p(qkv), _p(o), _p(dout), _p(lse), _p(cos), _p(sin), _p(dqkv), _p(workspace), B, Ntok, H,
                                          qkv.stride(0), o.stride(0), scale, None, self._stream()), "cs_attn_bwd")
            return
        q, eo, edo, elz, allow, dq, Q = (extra[k] for k in ("q", "o", "dout", "lse", "allow", "dq", "Q"))
        self._chk(q, eo, edo, elz, allow, dq)
        if not no_rope:
            self._check_identity_tables(cos, sin)
        assert (o is None) == (dout is None) == (lse is None), "image rows: o, dout and lse together or not at all"
        assert o is None or o.stride(0) == dout.stride(0)
        assert eo.stride(0) == edo.stride(0) and all(t.stride(1) == 1 for t in (q, eo, edo, dq))
        assert q.shape[0] == B * Q and eo.shape[0] == B * Q and dq.shape[0] == B * Q
        assert allow.dtype == torch.uint8 and allow.is_contiguous() and tuple(allow.shape) == (B * Q, Ntok)
        assert elz.dtype == torch.float32 and elz.is_contiguous() and elz.numel() == B * H * Q
        assert workspace.numel() * workspace.element_size() >= self.attn_bwd_workspace(B, Ntok, H, Q)
        ex = AttnExtra(_p(q), _p(eo), _p(edo), _p(elz), _p(allow), _p(dq), Q, q.stride(0), eo.stride(0), dq.stride(0))
        self._ok(self.lib.cs_attn_bwd(_p(qkv), _p(o), _p(dout), _p(lse), _p(cos), _p(sin), _p(dqkv), _p(workspace), B, Ntok, H,
                                      qkv.stride(0), o.stride(0) if o is not None else H * 64, scale, ctypes.byref(ex), self._stream()), "cs_attn_bwd")

    def swiglu_fwd(self, x12, h):
        self._chk(x12, h)
        M, Hd = h.shape
        self._ok(self.lib.cs_swiglu_fwd(_p(x12), x12.stride(0), _p(h), h.stride(0), M, Hd, self._stream()), "cs_swiglu_fwd")

    def swiglu_bwd_q8(self, dh, x12, dx12, q8, q_scale):
        """swiglu_bwd + the e4m3 copy of dx12 (bytes [M, 2*Hd rounded up to 128] + fp32 row scales) for an fp8 dgrad; = quant_rows_fp8(dx12)."""
        self._chk(dh, x12, dx12, q8, q_scale)
        M, Hd = dh.shape
        assert q_scale is not None and q8.element_size() == 1 and q8.stride(1) == 1 and q8.shape[1] >= (2 * Hd + 127) // 128 * 128
        self._ok(self.lib.cs_swiglu_bwd_q8(_p(dh), dh.stride(0), _p(x12), x12.stride(0), _p(dx12), dx12.stride(0), _p(q8), q8.stride(0),
                                           _p(q_scale), M, Hd, self._stream()), "cs_swiglu_bwd_q8")

    def swiglu_bwd_colsum(self, dh, x12, dx12, colsum, workspace):
        """swiglu_bwd + colsum[2*Hd] += column sums of dx12 (the w1 | w2 bias gradients) in the same pass; = swiglu_bwd, colsum_bf16(dx12)."""
        self._chk(dh, x12, dx12, colsum, workspace)
        M, Hd = dh.shape
        assert colsum.dtype == torch.float32 and colsum.numel() >= 2 * Hd and colsum.is_contiguous()
        assert workspace.numel() * workspace.element_size() >= self.colsum_workspace(M, 2 * Hd)
        self._ok(self.lib.cs_swiglu_bwd_colsum(_p(dh), dh.stride(0), _p(x12), x12.stride(0), _p(dx12), dx12.stride(0), _p(colsum), _p(workspace),
                                               M, Hd, self._stream()), "cs_swiglu_bwd_colsum")

    def swiglu_bwd(self, dh, x12, dx12, q8=None, q_scale=None):
        if q8 is not None:
            return self.swiglu_bwd_q8(dh, x12, dx12, q8, q_scale)
        self._chk(dh, x12, dx12)
        M, Hd = dh.shape
        self._ok(self.lib.cs_swiglu_bwd(_p(dh), dh.stride(0), _p(x12), x12.stride(0), _p(dx12), dx12.stride(0), M, Hd,
                                        self._stream()), "cs_swiglu_bwd")

    def gelu_fwd(self, x, y, quick=False):
        self._chk(x, y)
        M, N = x.shape
        self._ok(self.lib.cs_gelu_fwd(_p(x), x.stride(0), _p(y), y.stride(0), M, N, int(bool(quick)), self._stream()), "cs_gelu_fwd")

    def gelu_bwd(self, dy, x, dx, quick=False):
        self._chk(dy, x, dx)
        M, N = x.shape
        self._ok(self.lib.cs_gelu_bwd(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(dx), dx.stride(0), M, N, int(bool(quick)),
                                      self._stream()), "cs_gelu_bwd")

    def cast_f32_bf16(self, x, y):
        self._chk(x, y)
        assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
        self._ok(self.lib.cs_cast_f32_bf16(_p(x), _p(y), x.numel(), self._stream()), "cs_cast_f32_bf16")

    def transpose_bf16(self, inp, out):
        """out[c, r] = inp[r, c]; out is [Cc, ld_out >= R] and columns R.. are zero-filled."""
        self._chk(inp, out)
        R, Cc = inp.shape
        assert out.shape[0] == Cc and out.is_contiguous()
        self._ok(self.lib.cs_transpose_bf16(_p(inp), inp.stride(0), _p(out), out.shape[1], R, Cc, 0, 1, self._stream()), "cs_transpose_bf16")

    def tokens_to_nchw(self, x, B, N, C, out):
        """x fp32 [B*N, >= C] (row stride ldx), token-major, each image's CLS row first -> out [B, C, h, w] contiguous, fp32 or bf16 (RNE):
        out[b, c, p] = x[b*N + 1 + p, c] -- forms 1 / 2 of cs_transpose_bf16 (evaclip_vit.py:117-122 `_expand_x`)."""
        self._chk(x, out)
        assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B * N and x.shape[1] >= C and N >= 2
        assert out.is_contiguous() and out.dim() == 4 and out.shape[0] == B and out.shape[1] == C and out.shape[2] * out.shape[3] == N - 1
        self._ok(self.lib.cs_transpose_bf16(_p(x), x.stride(0), _p(out), N - 1, N - 1, C, 1 + _dt(out), B, self._stream()), "cs_transpose_bf16")

    @staticmethod
    def _deconv_form(form, rows, nchw, B, h, w, C, s, off):
        """Checks shared by rows_to_nchw / nchw_to_rows -> the packed `form` of cs_transpose_bf16 (include/clipself_hip.h)."""
        assert s in (1, 2) and off in (0, 1) and min(B, h, w, C) >= 1 and w < (1 << 19)
        assert rows.dim() == 2 and rows.stride(1) == 1 and rows.shape[0] == B * (h * w + off) and rows.shape[1] >= s * s * C <= rows.stride(0)
        assert nchw.is_contiguous() and tuple(nchw.shape) == (B, C, s * h, s * w)
        return form | (s - 1) << 8 | off << 9 | _dt(rows) << 10 | _dt(nchw) << 11 | w << 12

    def rows_to_nchw(self, rows, B, h, w, C, s, off, out):
        """rows fp32 / bf16 [B*(h*w + off), >= s*s*C] (row stride ld) -> out [B, C, s*h, s*w] contiguous, fp32 or bf16 (RNE):
        out[b, c, s*i + di, s*j + dj] = rows[b*(h*w + off) + off + i*w + j, (di*s + dj)*C + c] -- form 4 of cs_transpose_bf16: the output
        permutation of a transposed convolution with kernel == stride == s run as a GEMM on token rows (s = 1: rows back to a map)."""
        self._chk(rows, out)
        form = self._deconv_form(4, rows, out, B, h, w, C, s, off)
        self._ok(self.lib.cs_transpose_bf16(_p(rows), rows.stride(0), _p(out), 0, h * w, C, form, B, self._stream()), "cs_transpose_bf16")

    def nchw_to_rows(self, x, B, h, w, C, s, off, rows):
        """The inverse, form 5: x fp32 / bf16 [B, C, s*h, s*w] contiguous -> rows bf16 (RNE) [B*(h*w + off), >= s*s*C]; with off = 1 each
        image's CLS row gets s*s*C zeros.  Columns past s*s*C are left alone."""
        self._chk(x, rows)
        assert rows.dtype == torch.bfloat16
        form = self._deconv_form(5, rows, x, B, h, w, C, s, off)
        self._ok(self.lib.cs_transpose_bf16(_p(x), 0, _p(rows), rows.stride(0), h * w, C, form, B, self._stream()), "cs_transpose_bf16")

    @staticmethod
    def _topdown_form(form, coarse, fine, B, h, w, C, accumulate):
        """Checks shared by upsample2x_add / pool2x -> the packed `form` of cs_transpose_bf16 (include/clipself_hip.h)."""
        assert min(B, h, w, C) >= 1 and w < (1 << 20) and B * h * w * C < (1 << 31)
        assert coarse.dim() == 2 and coarse.stride(1) == 1 and coarse.shape[0] == B * h * w and coarse.shape[1] == C <= coarse.stride(0)
        assert fine.dim() == 2 and fine.stride(1) == 1 and fine.shape[0] == 4 * B * h * w and fine.shape[1] == C <= fine.stride(0)
        return form | 1 << 8 | int(bool(accumulate)) << 9 | _dt(coarse) << 10 | _dt(fine) << 11 | w << 12

    def upsample2x_add(self, coarse, fine, B, h, w, C, accumulate=True):
        """coarse fp32 / bf16 rows [B*h*w, C], fine fp32 / bf16 rows [B*2h*2w, C] (each with its own row stride >= C), in place:
        fine[b, 2i+di, 2j+dj, c] = rnd((fine[b, 2i+di, 2j+dj, c] if accumulate else 0) + coarse[b, i, j, c]) -- form 7 of cs_transpose_bf16:
        the FPN's laterals[i - 1] += F.interpolate(laterals[i], scale_factor=2, mode='nearest') on channel-last maps.  One rounding."""
        self._chk(coarse, fine)
        form = self._topdown_form(7, coarse, fine, B, h, w, C, accumulate)
        self._ok(self.lib.cs_transpose_bf16(_p(coarse), coarse.stride(0), _p(fine), fine.stride(0), h * w, C, form, B, self._stream()),
                 "cs_transpose_bf16")

    def pool2x(self, fine, coarse, B, h, w, C, accumulate=False):
        """Its adjoint, form 8: coarse[b, i, j, c] = rnd((coarse[b, i, j, c] if accumulate else 0) + s) with
        s = ((fine[b, 2i, 2j, c] + fine[b, 2i, 2j+1, c]) + fine[b, 2i+1, 2j, c]) + fine[b, 2i+1, 2j+1, c] in fp32."""
        self._chk(fine, coarse)
        form = self._topdown_form(8, coarse, fine, B, h, w, C, accumulate)
        self._ok(self.lib.cs_transpose_bf16(_p(fine), fine.stride(0), _p(coarse), coarse.stride(0), h * w, C, form, B, self._stream()),
                 "cs_transpose_bf16")

    def transpose_bf16_batched(self, pairs):
        """[(inp [R, C], out [C, ld_out >= R]), ...] -> every out = inp^T (zero padded) in ONE launch.  The device descriptor table is
        cached per list of buffers (the weight shadows and their transposes keep their addresses for the life of the engine)."""
        import numpy as np
        key = tuple((a.data_ptr(), b.data_ptr(), a.shape, b.shape, a.stride(0)) for a, b in pairs)
        tables = self.__dict__.setdefault("_tr_desc_tables", {})      # a few lists at most: every trainable block / a subset after a re-lock
        cache = tables.get(key)
        if cache is None:
            if len(tables) >= 8:
                tables.clear()
            rec = np.zeros((len(pairs), 6), dtype=np.int64)
            tile0 = 0
            for i, (a, b) in enumerate(pairs):
                self._chk(a, b)
                R, Cc = a.shape
                assert b.shape[0] == Cc and b.is_contiguous() and b.shape[1] >= R and a.stride(1) == 1
                tiles_x, tiles_y = (Cc + 63) // 64, (b.shape[1] + 63) // 64
                rec[i] = (a.data_ptr(), b.data_ptr(), a.stride(0), b.shape[1], R | (Cc << 32), tile0 | (tiles_x << 32))
                tile0 += tiles_x * tiles_y
            cache = tables[key] = (key, torch.from_numpy(rec).cuda(), tile0)
        _, desc, total = cache
        self._ok(self.lib.cs_transpose_bf16_batched(_p(desc), len(pairs), total, self._stream()), "cs_transpose_bf16_batched")

    def colsum_workspace(self, M, N) -> int:
        return int(self.lib.cs_colsum_workspace(M, N))

    def colsum_bf16(self, x, out, workspace=None):
        """out[n] += sum_m x[m, n] in a fixed order (row-block partials through `workspace`, >= colsum_workspace(M, N) bytes; allocated
        here when not given)."""
        self._chk(x, out, workspace)
        M, N = x.shape
        need = self.colsum_workspace(M, N)
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
        self._ok(self.lib.cs_colsum_bf16(_p(x), x.stride(0), _p(out), _p(workspace), M, N, self._stream()), "cs_colsum_bf16")

    def im2row(self, img, out, p):
        self._chk(img, out)
        B, _, S, _ = img.shape
        assert img.is_contiguous()
        assert out.stride(1) == 1 and out.stride(0) == out.shape[1], "im2row writes whole rows (zeros in [3*p*p, ldo)): out must be contiguous"
        self._ok(self.lib.cs_im2row(_p(img), _dt(img), _p(out), B, S, p, out.stride(0), self._stream()), "cs_im2row")

    def cls_row(self, x, cls, pos):
        self._chk(x, cls, pos)
        B, Ntok, C = x.shape
        self._ok(self.lib.cs_cls_row(_p(x), _p(cls), _p(pos), B, Ntok, C, self._stream()), "cs_cls_row")

    @staticmethod
    def _token_map(feat, grid_h, grid_w, tok_off):
        """-> (B, Ntok, E) of a token-major fp32 map: [B, Ntok, E], or its grid as a [B, h, w, E] view with strides (Ntok*E, w*E, E, 1)."""
        E = feat.shape[-1]
        assert feat.dtype == torch.float32 and feat.stride(-1) == 1 and E % 4 == 0 and feat.stride(0) % E == 0 and feat.data_ptr() % 16 == 0
        if feat.dim() == 4:
            assert tuple(feat.shape[1:3]) == (grid_h, grid_w) and feat.stride(2) == E and feat.stride(1) == grid_w * E, \
                "a [B, h, w, E] map must be a view of the token-major layout"
        else:
            assert feat.dim() == 3 and feat.stride(1) == E
        Ntok = feat.stride(0) // E if feat.shape[0] > 1 else max(feat.stride(0) // E, tok_off + grid_h * grid_w)
        return feat.shape[0], Ntok, E

    def roialign_fwd(self, feat, rois, pooled, grid_h, grid_w, tok_off, *, box_scale=0.0):
        """box_scale = 0: boxes normalised to [0, 1], unchecked (the distillation path).  box_scale = 1 / featmap_stride: pixel boxes,
        torchvision's scaling; image indices outside the map and boxes wider than twice the grid pool to 0 (include/clipself_hip.h)."""
        self._chk(feat, rois, pooled)
        B, Ntok, E = self._token_map(feat, grid_h, grid_w, tok_off)
        assert rois.is_contiguous() and rois.dtype == torch.float32 and pooled.is_contiguous() and pooled.dtype == torch.float32
        self._ok(self.lib.cs_roialign_fwd(_p(feat), _p(rois), _p(pooled), rois.shape[0], Ntok, grid_h, grid_w, E, tok_off, float(box_scale),
                                          B if box_scale else 0, None, 0, 0.0, None, 0, None, None, 0, self._stream()), "cs_roialign_fwd")

    def box_scores(self, feat, rois, class_embed, scores, grid_h, grid_w, tok_off, box_scale, vlm_temp, det_logits=None, expo=None, pooled=None):
        """Open-vocabulary box scores in one launch (cs_roialign_fwd's scoring form): pool every pixel box of rois [K, 5] from the
        token-major map, normalise, take logits against class_embed [C, E] (fp32, contiguous) times vlm_temp, softmax, and blend with
        softmax(det_logits [K, C]) by the per-class exponents expo [C]:  scores = det^(1-expo) * vlm^expo, evaluated in the log domain;
        det_logits None -> the VLM softmax alone.  pooled [K, E] (optional) receives the pooled features, not normalised."""
        self._chk(feat, rois, class_embed, scores, det_logits, expo, pooled)
        B, Ntok, E = self._token_map(feat, grid_h, grid_w, tok_off)
        K, C = rois.shape[0], class_embed.shape[0]
        f32 = torch.float32
        assert rois.is_contiguous() and rois.dtype == f32 and tuple(rois.shape) == (K, 5)
        assert class_embed.is_contiguous() and class_embed.dtype == f32 and class_embed.shape[1] == E and class_embed.data_ptr() % 16 == 0
        assert scores.dtype == f32 and tuple(scores.shape) == (K, C) and scores.stride(1) == 1
        assert det_logits is None or (det_logits.dtype == f32 and tuple(det_logits.shape) == (K, C) and det_logits.stride(1) == 1)
        assert det_logits is None or (expo is not None and expo.dtype == f32 and expo.is_contiguous() and expo.numel() == C), \
            "det_logits needs the per-class exponents"
        assert pooled is None or (pooled.is_contiguous() and pooled.dtype == f32 and tuple(pooled.shape) == (K, E))
        self._ok(self.lib.cs_roialign_fwd(_p(feat), _p(rois), _p(pooled), K, Ntok, grid_h, grid_w, E, tok_off, float(box_scale), B,
                                          _p(class_embed), C, float(vlm_temp), _p(det_logits), det_logits.stride(0) if det_logits is not None else 0,
                                          _p(expo) if det_logits is not None else None, _p(scores), scores.stride(0), self._stream()),
                 "cs_roialign_fwd")

    # -- detector post-processing (include/clipself_det.h) ------------------------------------------
    def nms_workspace(self, B, Kmax, C_or_G, max_num) -> int:
        return self._size("csd_nms_workspace", int(B), int(Kmax), int(C_or_G), int(max_num))

    def nms(self, boxes, scores, starts, Kmax, score_thr, iou_thr, max_num, group=None, G=0, out=None, workspace=None):
        """Score threshold, per-list greedy NMS and the per-image cut (csd_nms): boxes [K, 4], scores [K, C] (foreground columns), starts
        [B + 1] int32 on the device, group [K] int32 with G groups for the RPN form (C == 1).  -> (dets [B, max_num, 5], labels, inds
        [B, max_num] int32, counts [B] int32): fixed shapes, nothing is read back.  The workspace is this header's one buffer per device,
        grown to the largest call so far (pass workspace= to own it): once it is large enough the call allocates only its outputs (pass
        out= to own those too) and never synchronises, which is what stream capture needs (the tests do not capture); calls that share
        the buffer must share a stream."""
        self._chk(boxes, scores, starts, group, workspace)
        f32, i32 = torch.float32, torch.int32
        lds = self._rows(scores, _F32, None, None, "nms: scores")
        K, C = scores.shape
        ldb = self._rows(boxes, _F32, K, 4, "nms: boxes")
        B = starts.numel() - 1
        assert starts.dtype == i32 and starts.is_contiguous() and B >= 1
        assert group is None or (group.dtype == i32 and group.is_contiguous() and group.numel() == K)
        L = int(G) if group is not None else C
        if out is None:
            dev = boxes.device
            out = (torch.empty(B, max_num, 5, dtype=f32, device=dev), torch.empty(B, max_num, dtype=i32, device=dev),
                   torch.empty(B, max_num, dtype=i32, device=dev), torch.empty(B, dtype=i32, device=dev))
        dets, labels, inds, counts = out
        assert all(t.is_contiguous() for t in out) and dets.dtype == f32 and labels.dtype == i32 and inds.dtype == i32 and counts.dtype == i32
        assert dets.numel() == B * max_num * 5 and labels.numel() == B * max_num and inds.numel() == B * max_num and counts.numel() == B
        workspace = self._workspace("clipself_det.h", self.nms_workspace(B, Kmax, L, max_num), boxes.device, workspace, "nms")
        self._ok(self.lib.csd_nms(_p(boxes), ldb, _p(scores), lds, C, _p(starts), _p(group), int(G), K, B, int(Kmax), float(score_thr),
                                  float(iou_thr), int(max_num), _p(dets), _p(labels), _p(inds), _p(counts), _p(workspace), self._stream()),
                 "csd_nms")
        return dets, labels, inds, counts

    def delta2bbox(self, rois, deltas, out, means=(0.0, 0.0, 0.0, 0.0), stds=(1.0, 1.0, 1.0, 1.0), wh_ratio_clip=16 / 1000, starts=None,
                   max_shape=None, scale=None):
        """mmdet's DeltaXYWHBBoxCoder.decode and the rescale (csd_delta2bbox): rois [K, 4] columns x0, y0, x1, y1 (a view rois[:, 1:] of
        [K, 5] rois is fine), deltas [K, 4] -> out [K, 4].  max_shape [B, 2] = (h, w) and scale [B, 4] (the scale factors the boxes are
        divided by) are device tensors per image and need starts [B + 1]."""
        self._chk(rois, deltas, out, starts, max_shape, scale)
        f32 = torch.float32
        K = rois.shape[0]
        ldr = self._rows(rois, _F32, K, 4, "delta2bbox: rois")
        ldd = self._rows(deltas, _F32, K, 4, "delta2bbox: deltas")
        ldo = self._rows(out, _F32, K, 4, "delta2bbox: out")
        B = 0
        if max_shape is not None or scale is not None:
            assert starts is not None and starts.dtype == torch.int32 and starts.is_contiguous()
            B = starts.numel() - 1
            assert max_shape is None or (max_shape.dtype == f32 and max_shape.is_contiguous() and tuple(max_shape.shape) == (B, 2))
            assert scale is None or (scale.dtype == f32 and scale.is_contiguous() and tuple(scale.shape) == (B, 4))
        m4, s4 = (_f * 4)(*[float(v) for v in means]), (_f * 4)(*[float(v) for v in stds])
        self._ok(self.lib.csd_delta2bbox(_p(rois), ldr, _p(deltas), ldd, _p(starts), B, K, m4, s4, float(wh_ratio_clip),
                                         _p(max_shape), _p(scale), _p(out), ldo, self._stream()), "csd_delta2bbox")
        return out

    # -- detector training targets (include/clipself_assign.h) -----------------------------------------
    def assign_workspace(self, B, Nmax, Gmax, num=1) -> int:
        return self._size("csa_workspace", int(B), int(Nmax), int(Gmax), int(num))

    def _assign_layout(self, boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax):
        """The checks the three csa_ wrappers share -> (K, ldb, Gtot, ldg)."""
        f32, i32 = torch.float32, torch.int32
        ldb, ldg = self._rows(boxes, _F32, None, 4, "boxes"), self._rows(gt_boxes, _F32, None, 4, "gt_boxes")
        if gt_starts.dtype != i32 or not gt_starts.is_contiguous() or gt_starts.numel() != B + 1:
            raise ValueError(f"gt_starts must be contiguous int32 [B + 1] = [{B + 1}], got {gt_starts.dtype} {tuple(gt_starts.shape)}")
        if starts is not None and (starts.dtype != i32 or not starts.is_contiguous() or starts.numel() != B + 1):
            raise ValueError(f"starts must be None (shared rows) or contiguous int32 [B + 1] = [{B + 1}], got {starts.dtype} {tuple(starts.shape)}")
        if not (1 <= B <= 65535 and 0 <= Nmax <= ASSIGN_MAX_ROWS and 0 <= Gmax <= ASSIGN_MAX_GT):
            raise ValueError(f"limits: 1 <= B <= 65535, 0 <= Nmax <= {ASSIGN_MAX_ROWS}, 0 <= Gmax <= {ASSIGN_MAX_GT} (B = {B}, Nmax = {Nmax}, Gmax = {Gmax})")
        return boxes.shape[0], ldb, gt_boxes.shape[0], ldg

    def assign(self, boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True,
               gt_max_assign_all=True, gt_prefix=False, valid=None, out=None, workspace=None):
        """MaxIoUAssigner.assign for B images in one call (csa_assign): boxes [K, 4] grouped by starts [B + 1] int32 (None: all images share
        the K rows), gt_boxes [Gtot, 4] grouped by gt_starts, valid [K] uint8 or None; neg_iou_thr a float or (lo, hi).
        -> (gt_inds [B, Nmax] int32, max_overlaps [B, Nmax] fp32); nothing is read back.  The workspace is this header's one
        buffer per device (pass workspace= to own it); calls that share it must share a stream."""
        self._chk(boxes, starts, gt_boxes, gt_starts, valid, workspace)
        B, Nmax, Gmax = int(B), int(Nmax), int(Gmax)
        K, ldb, Gtot, ldg = self._assign_layout(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax)
        if valid is not None and (valid.dtype != torch.uint8 or not valid.is_contiguous() or valid.numel() != K):
            raise ValueError(f"valid must be contiguous uint8 [K] = [{K}], got {valid.dtype} {tuple(valid.shape)}")
        lo, hi = (neg_iou_thr if isinstance(neg_iou_thr, (tuple, list)) else (0.0, neg_iou_thr))
        if out is None:
            out = (torch.empty(B, Nmax, dtype=torch.int32, device=boxes.device), torch.empty(B, Nmax, dtype=torch.float32, device=boxes.device))
        gt_inds, max_overlaps = out
        if not (gt_inds.dtype == torch.int32 and max_overlaps.dtype == torch.float32 and gt_inds.is_contiguous() and max_overlaps.is_contiguous()
                and gt_inds.numel() == B * Nmax and max_overlaps.numel() == B * Nmax):
            raise ValueError("out must be (int32 [B, Nmax], fp32 [B, Nmax]), contiguous")
        workspace = self._workspace("clipself_assign.h", self.assign_workspace(B, Nmax, Gmax), boxes.device, workspace, "assign")
        self._ok(self.lib.csa_assign(_p(boxes), ldb, _p(starts), K, _p(gt_boxes), ldg, _p(gt_starts), Gtot, _p(valid), B, Nmax, Gmax,
                                     float(pos_iou_thr), float(lo), float(hi), float(min_pos_iou), int(bool(match_low_quality)),
                                     int(bool(gt_max_assign_all)), int(bool(gt_prefix)), _p(gt_inds), _p(max_overlaps), _p(workspace),
                                     self._stream()), "csa_assign")
        return gt_inds, max_overlaps

    def sample(self, gt_inds, keys, starts, K, gt_starts, Gtot, Gmax, num, expected_pos, neg_pos_ub=-1.0, out=None):
        """RandomSampler.sample for B images (csa_sample): gt_inds [B, Nmax] int32, keys [B, Nmax] uint32 bits (int32 or uint32 tensor).
        -> (flags [B, Nmax] uint8, sel [B, num] int32, counts [B, 2] int32); nothing is read back."""
        self._chk(gt_inds, keys, starts, gt_starts)
        if gt_inds.dim() != 2 or gt_inds.dtype != torch.int32 or not gt_inds.is_contiguous():
            raise ValueError(f"gt_inds must be contiguous int32 [B, Nmax], got {gt_inds.dtype} {tuple(gt_inds.shape)}")
        B, Nmax = gt_inds.shape
        if keys.element_size() != 4 or keys.is_floating_point() or not keys.is_contiguous() or tuple(keys.shape) != (B, Nmax):
            raise ValueError(f"keys must be contiguous 32-bit integers [B, Nmax] = [{B}, {Nmax}], got {keys.dtype} {tuple(keys.shape)}")
        num, expected_pos, Gmax = int(num), int(expected_pos), int(Gmax)
        if not (1 <= B <= 65535 and 0 <= Nmax <= ASSIGN_MAX_ROWS and 0 <= Gmax <= ASSIGN_MAX_GT and 1 <= num <= ASSIGN_MAX_NUM and 0 <= expected_pos <= num):
            raise ValueError(f"limits: 1 <= B <= 65535, Nmax <= {ASSIGN_MAX_ROWS}, Gmax <= {ASSIGN_MAX_GT}, 1 <= num <= {ASSIGN_MAX_NUM}, "
                             f"0 <= expected_pos <= num (B = {B}, Nmax = {Nmax}, Gmax = {Gmax}, num = {num}, expected_pos = {expected_pos})")
        for t, who in ((starts, "starts"), (gt_starts, "gt_starts")):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != B + 1):
                raise ValueError(f"{who} must be contiguous int32 [B + 1] = [{B + 1}]")
        if gt_starts is None:
            raise ValueError("gt_starts is needed (gt_inds is checked against each image's ground-truth count)")
        if out is None:
            dev = gt_inds.device
            out = (torch.empty(B, Nmax, dtype=torch.uint8, device=dev), torch.empty(B, num, dtype=torch.int32, device=dev),
                   torch.empty(B, 2, dtype=torch.int32, device=dev))
        flags, sel, counts = out
        if not (flags.dtype == torch.uint8 and sel.dtype == torch.int32 and counts.dtype == torch.int32 and all(t.is_contiguous() for t in out)
                and flags.numel() == B * Nmax and sel.numel() == B * num and counts.numel() == 2 * B):
            raise ValueError("out must be (uint8 [B, Nmax], int32 [B, num], int32 [B, 2]), contiguous")
        self._ok(self.lib.csa_sample(_p(gt_inds), _p(keys), _p(starts), int(K), _p(gt_starts), int(Gtot), B, Nmax, Gmax, num, expected_pos,
                                     float(neg_pos_ub), _p(flags), _p(sel), _p(counts), self._stream()), "csa_sample")
        return flags, sel, counts

    def bbox_targets(self, boxes, starts, gt_boxes, gt_labels, gt_starts, Gmax, gt_inds, flags=None, sel=None, means=(0.0, 0.0, 0.0, 0.0),
                     stds=(1.0, 1.0, 1.0, 1.0), bg_label=1, pos_weight=-1.0, out=None):
        """Labels, weights and bbox2delta targets (csa_targets).  out: the outputs, in the order returned, to own them.  sel None: the dense form of the anchor head, from flags [B, Nmax] ->
        (labels [B, Nmax], label_weights [B, Nmax], bbox_targets [B, Nmax, 4], bbox_weights [B, Nmax, 4]).  sel [B, num]: the compact form
        of the box head -> (rois [B, num, 5], labels [B, num], label_weights [B, num], bbox_targets [B, num, 4], bbox_weights [B, num, 4])."""
        self._chk(boxes, starts, gt_boxes, gt_labels, gt_starts, gt_inds, flags, sel)
        if gt_inds.dim() != 2 or gt_inds.dtype != torch.int32 or not gt_inds.is_contiguous():
            raise ValueError(f"gt_inds must be contiguous int32 [B, Nmax], got {gt_inds.dtype} {tuple(gt_inds.shape)}")
        B, Nmax = gt_inds.shape
        Gmax = int(Gmax)
        K, ldb, Gtot, ldg = self._assign_layout(boxes, starts, gt_boxes, gt_starts, B, Nmax, Gmax)
        if gt_labels is not None and (gt_labels.dtype != torch.int32 or not gt_labels.is_contiguous() or gt_labels.numel() != Gtot):
            raise ValueError(f"gt_labels must be contiguous int32 [Gtot] = [{Gtot}], got {gt_labels.dtype} {tuple(gt_labels.shape)}")
        if pos_weight > 0:
            raise ValueError(f"pos_weight = {pos_weight} is not supported (only pos_weight <= 0)")
        dev, f32, i32 = boxes.device, torch.float32, torch.int32
        num, rois = 1, None
        if sel is None:
            if flags is None or flags.dtype != torch.uint8 or not flags.is_contiguous() or tuple(flags.shape) != (B, Nmax):
                raise ValueError(f"the dense form needs flags: contiguous uint8 [B, Nmax] = [{B}, {Nmax}]")
            S = Nmax
        else:
            if sel.dtype != i32 or sel.dim() != 2 or not sel.is_contiguous() or sel.shape[0] != B or not 1 <= sel.shape[1] <= ASSIGN_MAX_NUM:
                raise ValueError(f"sel must be contiguous int32 [B, num] with 1 <= num <= {ASSIGN_MAX_NUM}, got {sel.dtype} {tuple(sel.shape)}")
            S = num = sel.shape[1]
        if out is None:
            out = (torch.empty(B, S, dtype=i32, device=dev), torch.empty(B, S, dtype=f32, device=dev),
                   torch.empty(B, S, 4, dtype=f32, device=dev), torch.empty(B, S, 4, dtype=f32, device=dev))
            if sel is not None:
                out = (torch.empty(B, S, 5, dtype=f32, device=dev),) + out
        if len(out) != (4 if sel is None else 5):
            raise ValueError("out must hold (labels, label_weights, bbox_targets, bbox_weights), with rois in front in the compact form")
        if sel is not None:
            rois = out[0]
        labels, label_weights, bt, bw = out[-4:]
        want = [(labels, i32, B * S), (label_weights, f32, B * S), (bt, f32, B * S * 4), (bw, f32, B * S * 4)] + ([(rois, f32, B * S * 5)] if sel is not None else [])
        for t, dt, n in want:
            if t.dtype != dt or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
                raise ValueError(f"out: expected a contiguous {dt} device tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")
        m4, s4 = (_f * 4)(*[float(v) for v in means]), (_f * 4)(*[float(v) for v in stds])
        self._ok(self.lib.csa_targets(_p(boxes), ldb, _p(starts), K, _p(gt_boxes), ldg, _p(gt_labels), _p(gt_starts), Gtot, B, Nmax, Gmax,
                                      _p(gt_inds), _p(flags), _p(sel), num, m4, s4, int(bg_label), float(pos_weight), _p(rois), _p(labels),
                                      _p(label_weights), _p(bt), _p(bw), self._stream()), "csa_targets")
        return (labels, label_weights, bt, bw) if sel is None else (rois, labels, label_weights, bt, bw)

    # -- detector losses (include/clipself_loss.h) ------------------------------------------------------
    def _loss_levels(self, cls_scores, bbox_preds, dcls=None, dreg=None):
        L = len(cls_scores)
        if not (1 <= L <= LOSS_MAX_LEVELS and len(bbox_preds) == L):
            raise ValueError(f"rpn_loss: {L} cls maps and {len(bbox_preds)} reg maps (1 <= L <= {LOSS_MAX_LEVELS})")
        B, A = cls_scores[0].shape[0], cls_scores[0].shape[1]
        arr, N = (LossLevel * L)(), 0
        for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
            if c.dim() != 4:
                raise ValueError(f"rpn_loss: level {l}: cls must be [B, A, h, w], got {tuple(c.shape)}")
            h, w = c.shape[2], c.shape[3]
            self._dense(c, torch.float32, (B, A, h, w), f"rpn_loss: level {l}: cls")
            self._dense(r, torch.float32, (B, 4 * A, h, w), f"rpn_loss: level {l}: reg")
            if dcls is not None:
                self._dense(dcls[l], torch.float32, (B, A, h, w), f"rpn_loss: level {l}: dcls")
                self._dense(dreg[l], torch.float32, (B, 4 * A, h, w), f"rpn_loss: level {l}: dreg")
            arr[l] = LossLevel(c.data_ptr(), r.data_ptr(), None if dcls is None else dcls[l].data_ptr(), None if dreg is None else dreg[l].data_ptr(),
                               int(h), int(w))
            N += h * w * A
        return arr, L, B, A, N

    def loss_workspace(self, cls_scores=None, bbox_preds=None, R=0) -> int:
        """Bytes of workspace (csl_workspace) for rpn_loss on these maps and / or bbox_head_loss on R rows; 0 outside the limits."""
        if cls_scores is None:
            return int(self.lib.csl_workspace(None, 0, 1, 1, int(R)))
        arr, L, B, A, _ = self._loss_levels(cls_scores, bbox_preds)
        return int(self.lib.csl_workspace(arr, L, B, A, int(R)))

    def rpn_loss(self, cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor, grad=True, out=None, workspace=None):
        """RPNHead.loss for all levels and images in one call (csl_rpn_loss).  cls_scores[l] [B, A, h, w], bbox_preds[l] [B, 4A, h, w];
        the dense targets [B, N] / [B, N, 4] as bbox_targets' dense form returns them; avg_factor a device fp32 scalar.
        -> (losses [L, 2], dcls list, dreg list), the gradient lists None with grad=False.  out: the same triple, to own the outputs.
        The workspace is cached per device (pass workspace= to own it); calls that share it must share a stream."""
        self._chk(labels, label_weights, bbox_targets, bbox_weights, avg_factor, *cls_scores, *bbox_preds)
        dev = labels.device
        if out is None:
            losses = torch.empty(len(cls_scores), 2, dtype=torch.float32, device=dev)
            dcls = [torch.empty_like(c) for c in cls_scores] if grad else None
            dreg = [torch.empty_like(r) for r in bbox_preds] if grad else None
        else:
            losses, dcls, dreg = out
        if (dcls is None) != (dreg is None):
            raise ValueError("rpn_loss: dcls and dreg are given together or both None")
        arr, L, B, A, N = self._loss_levels(cls_scores, bbox_preds, dcls, dreg)
        self._dense(labels, torch.int32, (B, N), "rpn_loss: labels")
        self._dense(label_weights, torch.float32, (B, N), "rpn_loss: label_weights")
        self._dense(bbox_targets, torch.float32, (B, N, 4), "rpn_loss: bbox_targets")
        self._dense(bbox_weights, torch.float32, (B, N, 4), "rpn_loss: bbox_weights")
        self._dense(losses, torch.float32, (L, 2), "rpn_loss: losses")
        if avg_factor.dtype != torch.float32 or avg_factor.numel() != 1:
            raise ValueError(f"rpn_loss: avg_factor must be a device fp32 scalar, got {avg_factor.dtype} {tuple(avg_factor.shape)}")
        ws = self._workspace("clipself_loss.h", int(self.lib.csl_workspace(arr, L, B, A, 0)), dev, workspace, "rpn_loss")
        self._ok(self.lib.csl_rpn_loss(arr, L, B, A, _p(labels), _p(label_weights), _p(bbox_targets), _p(bbox_weights), _p(avg_factor), _p(losses),
                                       _p(ws), self._stream()), "csl_rpn_loss")
        return losses, dcls, dreg

    def bbox_head_loss(self, cls_score, labels, label_weights, bbox_pred, bbox_targets, bbox_weights, bg_label, class_weight=None, avg_factor=None,
                       grad=True, out=None, workspace=None):
        """BBoxHead.loss, class-agnostic boxes, CustomCrossEntropyLoss + L1Loss + accuracy in one call (csl_bbox_head_loss).  cls_score
        [R, C1] fp32 with last stride 1 (its row stride is ldc); class_weight [C1] or None; avg_factor a device fp32 scalar or None
        (None: max(count(label_weights > 0), 1) on the device).  -> (out4 = (loss_cls, acc, loss_bbox, avg) [4], dcls [R, C1] with
        cls_score's row stride, dbbox [R, 4]), the gradients None with grad=False.  out: the same triple, to own the outputs."""
        self._chk(cls_score, labels, label_weights, bbox_pred, bbox_targets, bbox_weights, class_weight, avg_factor)
        dev, f32 = cls_score.device, torch.float32
        ldc = self._rows(cls_score, _F32, None, None, "bbox_head_loss: cls_score")
        R, C1 = cls_score.shape
        self._dense(labels, torch.int32, (R,), "bbox_head_loss: labels")
        self._dense(label_weights, f32, (R,), "bbox_head_loss: label_weights")
        for t, who in ((bbox_pred, "bbox_pred"), (bbox_targets, "bbox_targets"), (bbox_weights, "bbox_weights")):
            self._dense(t, f32, (R, 4), "bbox_head_loss: " + who)
        if class_weight is not None:
            self._dense(class_weight, f32, (C1,), "bbox_head_loss: class_weight")
        if avg_factor is not None and (avg_factor.dtype != f32 or avg_factor.numel() != 1):
            raise ValueError(f"bbox_head_loss: avg_factor must be a device fp32 scalar or None, got {avg_factor.dtype} {tuple(avg_factor.shape)}")
        if out is None:
            out4 = torch.empty(4, dtype=f32, device=dev)
            dcls = torch.empty_strided((R, C1), (ldc, 1), dtype=f32, device=dev) if grad else None
            dbbox = torch.empty(R, 4, dtype=f32, device=dev) if grad else None
        else:
            out4, dcls, dbbox = out
        self._dense(out4, f32, (4,), "bbox_head_loss: out")
        if dcls is not None:
            if dcls.dtype != f32 or tuple(dcls.shape) != (R, C1) or not dcls.is_cuda or (R > 0 and dcls.stride(1) != 1) or (R > 1 and dcls.stride(0) != ldc):
                raise ValueError(f"bbox_head_loss: dcls must be fp32 [R, C1] with cls_score's strides ({ldc}, 1), got {tuple(dcls.shape)} {dcls.stride()}")
        if dbbox is not None:
            self._dense(dbbox, f32, (R, 4), "bbox_head_loss: dbbox")
        ws = self._workspace("clipself_loss.h", int(self.lib.csl_workspace(None, 0, 1, 1, R)), dev, workspace, "bbox_head_loss")
        self._ok(self.lib.csl_bbox_head_loss(_p(cls_score), ldc, _p(labels), _p(label_weights), _p(class_weight), _p(bbox_pred), _p(bbox_targets),
                                             _p(bbox_weights), R, C1, int(bg_label), _p(avg_factor), _p(out4), _p(dcls), _p(dbbox), _p(ws),
                                             self._stream()), "csl_bbox_head_loss")
        return out4, dcls, dbbox

    # -- RPN proposals (include/clipself_rpn.h) -----------------------------------------------------------
    def _rpn_levels(self, cls_scores, bbox_preds, nms_pre):
        """-> (csp_level array, L, B, A, N, Ktot); ValueError outside the limits of the header."""
        L = len(cls_scores)
        if not (1 <= L <= RPN_MAX_LEVELS and len(bbox_preds) == L):
            raise ValueError(f"rpn_select: {L} cls maps and {len(bbox_preds)} reg maps (1 <= L <= {RPN_MAX_LEVELS})")
        if cls_scores[0].dim() != 4:
            raise ValueError(f"rpn_select: level 0: cls must be [B, A, h, w], got {tuple(cls_scores[0].shape)}")
        B, A = cls_scores[0].shape[0], cls_scores[0].shape[1]
        nms_pre = int(nms_pre)
        if not (1 <= B <= 65535 and 1 <= A <= RPN_MAX_ANCHORS and 1 <= nms_pre <= RPN_MAX_PRE):
            raise ValueError(f"rpn_select: limits 1 <= B <= 65535, 1 <= A <= {RPN_MAX_ANCHORS}, 1 <= nms_pre <= {RPN_MAX_PRE} "
                             f"(B = {B}, A = {A}, nms_pre = {nms_pre})")
        arr, N, Ktot = (RpnLevel * L)(), 0, 0
        for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
            if c.dim() != 4:
                raise ValueError(f"rpn_select: level {l}: cls must be [B, A, h, w], got {tuple(c.shape)}")
            h, w = int(c.shape[2]), int(c.shape[3])
            if not (1 <= h <= RPN_MAX_SIDE and 1 <= w <= RPN_MAX_SIDE):
                raise ValueError(f"rpn_select: level {l}: h = {h}, w = {w} must be in [1, {RPN_MAX_SIDE}]")
            self._dense(c, torch.float32, (B, A, h, w), f"rpn_select: level {l}: cls")
            self._dense(r, torch.float32, (B, 4 * A, h, w), f"rpn_select: level {l}: reg")
            arr[l] = RpnLevel(c.data_ptr(), r.data_ptr(), h, w)
            N += h * w * A
            Ktot += min(nms_pre, h * w * A)
        if Ktot > RPN_MAX_ROWS:
            raise ValueError(f"rpn_select: Ktot = {Ktot} rows per image, at most {RPN_MAX_ROWS}")
        return arr, L, B, A, N, Ktot

    def rpn_select_workspace(self, cls_scores, bbox_preds, nms_pre) -> int:
        """Bytes of workspace (csp_workspace) for rpn_select on these maps."""
        arr, L, B, A, _, _ = self._rpn_levels(cls_scores, bbox_preds, nms_pre)
        return int(self.lib.csp_workspace(arr, L, B, A, int(nms_pre)))

    def rpn_select(self, cls_scores, bbox_preds, anchors, nms_pre, means=(0.0, 0.0, 0.0, 0.0), stds=(1.0, 1.0, 1.0, 1.0), wh_ratio_clip=16 / 1000,
                   max_shape=None, min_bbox_size=0.0, out=None, workspace=None):
        """The nms_pre best anchors of every (image, level), decoded and filtered, in one call (csp_select).  cls_scores[l] [B, A, h, w],
        bbox_preds[l] [B, 4A, h, w] fp32; anchors [N, 4] fp32 with last stride 1 (its row stride is lda), all levels one after another;
        max_shape [B, 2] = (h, w) fp32 on the device or None.
        -> (boxes [B * Ktot, 4], scores [B * Ktot], group [B * Ktot] int32, anchor_inds [B * Ktot] int32, starts [B + 1] int32): what nms'
        group form takes; nothing is read back.  out: the same five, to own the outputs.  The workspace is cached per device (pass
        workspace= to own it); calls that share it must share a stream."""
        self._chk(anchors, max_shape, workspace, *cls_scores, *bbox_preds)
        arr, L, B, A, N, Ktot = self._rpn_levels(cls_scores, bbox_preds, nms_pre)
        f32, i32, dev = torch.float32, torch.int32, anchors.device
        if anchors.dtype != f32 or anchors.dim() != 2 or anchors.shape[0] != N or anchors.shape[1] < 4 or anchors.stride(1) != 1:
            raise ValueError(f"rpn_select: anchors must be fp32 [N = {N}, >= 4] with last stride 1, got {anchors.dtype} {tuple(anchors.shape)}")
        lda = anchors.stride(0) if N > 1 else max(anchors.stride(0), 4)
        if lda < 4:
            raise ValueError(f"rpn_select: the row stride of anchors is {lda}, at least 4 is needed")
        if max_shape is not None:
            self._dense(max_shape, f32, (B, 2), "rpn_select: max_shape")
        if out is None:
            out = (torch.empty(B * Ktot, 4, dtype=f32, device=dev), torch.empty(B * Ktot, dtype=f32, device=dev),
                   torch.empty(B * Ktot, dtype=i32, device=dev), torch.empty(B * Ktot, dtype=i32, device=dev),
                   torch.empty(B + 1, dtype=i32, device=dev))
        boxes, scores, group, anchor_inds, starts = out
        self._dense(boxes, f32, (B * Ktot, 4), "rpn_select: boxes")
        self._dense(scores, f32, (B * Ktot,), "rpn_select: scores")
        self._dense(group, i32, (B * Ktot,), "rpn_select: group")
        if anchor_inds is not None:
            self._dense(anchor_inds, i32, (B * Ktot,), "rpn_select: anchor_inds")
        self._dense(starts, i32, (B + 1,), "rpn_select: starts")
        workspace = self._workspace("clipself_rpn.h", int(self.lib.csp_workspace(arr, L, B, A, int(nms_pre))), dev, workspace, "rpn_select")
        m4, s4 = (_f * 4)(*[float(v) for v in means]), (_f * 4)(*[float(v) for v in stds])
        self._ok(self.lib.csp_select(arr, L, B, A, _p(anchors), lda, int(nms_pre), m4, s4, float(wh_ratio_clip), _p(max_shape),
                                     float(min_bbox_size), _p(boxes), _p(scores), _p(group), _p(anchor_inds), _p(starts), _p(workspace),
                                     self._stream()), "csp_select")
        return boxes, scores, group, anchor_inds, starts

    # -- 3 x 3 convolutions of the detector heads (include/clipself_conv.h) ---------------------------------
    def conv3x3(self, x, Wg, y, bias, N, H, W):
        """y[p, co] = bias[co] + sum_{t, ci} x[p shifted by tap t, ci] * Wg[co, t*Cin + ci] (csc_conv3x3): Conv2d(Cin, Cout, 3, padding=1)
        on channel-last rows.  x bf16 [N*H*W, Cin] (row stride % 8 == 0), Wg bf16 [Cout, 9*Cin], bias fp32 [Cout] or None, y fp32 or bf16
        [N*H*W, Cout] (row stride % 4 == 0).  Cin % 64 == 0 and Cout % 8 == 0, else ValueError."""
        self._chk(x, Wg, y, bias)
        N, H, W = int(N), int(H), int(W)
        if min(N, H, W) < 1 or N * H * W > CONV_MAX_ROWS:
            raise ValueError(f"conv3x3: 1 <= N*H*W <= {CONV_MAX_ROWS} (N = {N}, H = {H}, W = {W})")
        ldx = self._rows(x, (torch.bfloat16,), N * H * W, None, "conv3x3: x", 8, 16)
        Cin = x.shape[1]
        if Wg.dtype != torch.bfloat16 or Wg.dim() != 2 or Wg.shape[1] != 9 * Cin or Wg.stride(1) != 1 or Wg.stride(0) % 8 or Wg.data_ptr() % 16:
            raise ValueError(f"conv3x3: Wg must be bf16 [Cout, 9*Cin = {9 * Cin}] with 16-byte aligned rows, got {Wg.dtype} {tuple(Wg.shape)}")
        Cout = Wg.shape[0]
        if Cin % 64 or Cout % 8:
            raise ValueError(f"conv3x3: outside the kernel's coverage (Cin % 64 == 0, Cout % 8 == 0): Cin = {Cin}, Cout = {Cout}")
        ldy = self._rows(y, _F32_BF16, N * H * W, Cout, "conv3x3: y", 4, 16)
        if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (Cout,) or not bias.is_contiguous() or bias.data_ptr() % 16):
            raise ValueError(f"conv3x3: bias must be contiguous fp32 [{Cout}], 16-byte aligned")
        rc = self.lib.csc_conv3x3(_p(x), ldx, _p(Wg), max(Wg.stride(0), 9 * Cin), _p(bias), _p(y), ldy, _dt(y), N, H, W, Cin, Cout, self._stream())
        if rc == 1:
            raise ValueError("csc_conv3x3: shape outside the kernel's coverage")
        self._ok(rc, "csc_conv3x3")

    def im2col3x3(self, x, cols, N, H, W, row0=0):
        """cols[r, t*Cin + ci] = x[(row0 + r) shifted by tap t, ci], zero where the tap leaves the image (csc_im2col3x3): rows
        [row0, row0 + cols.shape[0]) of the explicit matrix.  x bf16 [N*H*W, Cin], cols bf16 [rows, 9*Cin] (row strides % 8 == 0; columns
        past 9*Cin of a wider row are left alone).  Cin % 8 == 0, else ValueError."""
        self._chk(x, cols)
        N, H, W, row0 = int(N), int(H), int(W), int(row0)
        if min(N, H, W) < 1 or N * H * W > CONV_MAX_ROWS:
            raise ValueError(f"im2col3x3: 1 <= N*H*W <= {CONV_MAX_ROWS} (N = {N}, H = {H}, W = {W})")
        ldx = self._rows(x, (torch.bfloat16,), N * H * W, None, "im2col3x3: x", 8, 16)
        Cin = x.shape[1]
        if Cin % 8:
            raise ValueError(f"im2col3x3: outside the kernel's coverage (Cin % 8 == 0): Cin = {Cin}")
        ldc = self._rows(cols, (torch.bfloat16,), None, 9 * Cin, "im2col3x3: cols", 8, 16)
        rows = cols.shape[0]
        if not (0 <= row0 and row0 + rows <= N * H * W):
            raise ValueError(f"im2col3x3: rows [{row0}, {row0 + rows}) outside the map's {N * H * W} rows")
        rc = self.lib.csc_im2col3x3(_p(x), ldx, _p(cols), ldc, row0, rows, N, H, W, Cin, self._stream())
        if rc == 1:
            raise ValueError("csc_im2col3x3: shape outside the kernel's coverage")
        self._ok(rc, "csc_im2col3x3")

    # -- batch norm (+ ReLU) on channel-last maps (include/clipself_bn.h) --------------------------------
    @staticmethod
    def _bn_shape(x, who):
        if x.dim() != 2:
            raise ValueError(f"{who}: a map is 2-D rows [M, C], got {tuple(x.shape)}")
        M, C = x.shape
        if not (1 <= M <= BN_MAX_ROWS and 1 <= C <= BN_MAX_C):
            raise ValueError(f"{who}: 1 <= M <= {BN_MAX_ROWS}, 1 <= C <= {BN_MAX_C} (M = {M}, C = {C})")
        if C % 8:
            raise ValueError(f"{who}: outside the kernels' coverage (C % 8 == 0): C = {C}")
        return M, C

    @staticmethod
    def _bn_vec(t, n, who, optional=False):
        if t is None and optional:
            return
        if t is None or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{who} must be contiguous fp32 with {n} elements, 16-byte aligned")

    @staticmethod
    def _bn_stream(t):
        """The current stream of t's device as a raw handle.  These wrappers run five times per layer and step, where
        torch.cuda.current_stream() (a Python object per call) is a tenth of the host time; the raw getter is what torch's own
        compiled code paths use."""
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        return raw(t.device.index) if raw is not None else torch.cuda.current_stream(t.device).cuda_stream

    def _bn_rc(self, rc, who):
        if rc == 1:
            raise ValueError(f"{who}: shape outside the kernels' coverage")
        self._ok(rc, who)

    def bn_workspace(self, M, C) -> int:
        """Bytes of per-part partial sums (csb_workspace) that bn_stats and bn_bwd_reduce need for a map of M rows and C channels."""
        return self._size("csb_workspace", int(M), int(C))

    def bn_stats(self, x, rec, ws=None):
        """This rank's record of the map x [M, C] (csb_stats): rec fp32 [2*C + 4] = mean | M2 = sum (x - mean)^2 | the row count as int32 bits."""
        self._chk(x, rec, ws)
        M, C = self._bn_shape(x, "bn_stats")
        ldx = self._rows(x, _F32_BF16, M, C, "bn_stats: x", (4, 8), 16)
        self._bn_vec(rec, 2 * C + BN_REC_EXTRA, "bn_stats: rec")
        ws = self._workspace("clipself_bn.h", self._size("csb_workspace", M, C), x.device, ws, "bn_stats")
        self._bn_rc(self.lib.csb_stats(_p(x), ldx, _dt(x), M, C, _p(rec), _p(ws), self._bn_stream(x)), "csb_stats")

    def bn_finalize(self, recs, C, gamma, beta, eps, momentum, running_mean, running_var, st):
        """The state st fp32 [4*C + 4] = mean | rstd | scale | shift | 1/N (csb_finalize) from recs fp32 [R, 2*C + 4] merged in ascending order
        by count (training; running_mean / running_var updated in place where given) or, with recs=None, from the running statistics."""
        self._chk(recs, gamma, beta, running_mean, running_var, st)
        C = int(C)
        if not 1 <= C <= BN_MAX_C:
            raise ValueError(f"bn_finalize: 1 <= C <= {BN_MAX_C} (C = {C})")
        if C % 8:
            raise ValueError(f"bn_finalize: outside the kernels' coverage (C % 8 == 0): C = {C}")
        R = 0
        if recs is not None:
            if recs.dim() == 1:
                recs = recs.view(1, -1)
            R = recs.shape[0]
            if not 1 <= R <= BN_MAX_RECORDS:
                raise ValueError(f"bn_finalize: 1 <= R <= {BN_MAX_RECORDS} records (R = {R})")
            self._bn_vec(recs, R * (2 * C + BN_REC_EXTRA), "bn_finalize: recs")
        elif running_mean is None or running_var is None:
            raise ValueError("bn_finalize: recs=None (evaluation mode) needs running_mean and running_var")
        if not float(eps) >= 0.0:
            raise ValueError(f"bn_finalize: eps >= 0 (eps = {eps})")
        for t, who in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
            self._bn_vec(t, C, f"bn_finalize: {who}", optional=True)
        self._bn_vec(st, 4 * C + BN_ST_EXTRA, "bn_finalize: st")
        self._bn_rc(self.lib.csb_finalize(_p(recs), R, C, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var),
                                          _p(st), self._bn_stream(st)), "csb_finalize")

    @staticmethod
    def _bn_act(act):
        if act not in (0, 1):
            raise ValueError(f"act is 0 (none) or 1 (ReLU), got {act!r}")
        return int(act)

    def bn_apply(self, x, st, act, y):
        """y = act(fmaf(x, scale[c], shift[c])) (csb_apply): x, y fp32 / bf16 [M, C], st from bn_finalize, act 0 = none, 1 = ReLU."""
        self._chk(x, st, y)
        M, C = self._bn_shape(x, "bn_apply")
        ldx = self._rows(x, _F32_BF16, M, C, "bn_apply: x", (4, 8), 16)
        ldy = self._rows(y, _F32_BF16, M, C, "bn_apply: y", (4, 8), 16)
        self._bn_vec(st, 4 * C + BN_ST_EXTRA, "bn_apply: st")
        self._bn_rc(self.lib.csb_apply(_p(x), ldx, _dt(x), _p(st), self._bn_act(act), _p(y), ldy, _dt(y), M, C, self._bn_stream(x)), "csb_apply")

    def bn_bwd_reduce(self, dy, x, st, act, sums, ws=None):
        """sums fp32 [2*C] = sum g | sum g * xhat over the rows (csb_bwd_reduce), g = dy under the ReLU mask recomputed from x and st."""
        self._chk(dy, x, st, sums, ws)
        M, C = self._bn_shape(x, "bn_bwd_reduce")
        lddy = self._rows(dy, _F32_BF16, M, C, "bn_bwd_reduce: dy", (4, 8), 16)
        ldx = self._rows(x, _F32_BF16, M, C, "bn_bwd_reduce: x", (4, 8), 16)
        self._bn_vec(st, 4 * C + BN_ST_EXTRA, "bn_bwd_reduce: st")
        self._bn_vec(sums, 2 * C, "bn_bwd_reduce: sums")
        ws = self._workspace("clipself_bn.h", self._size("csb_workspace", M, C), x.device, ws, "bn_bwd_reduce")
        self._bn_rc(self.lib.csb_bwd_reduce(_p(dy), lddy, _dt(dy), _p(x), ldx, _dt(x), _p(st), self._bn_act(act), _p(sums), _p(ws), M, C,
                                            self._bn_stream(x)), "csb_bwd_reduce")

    def bn_bwd_apply(self, dy, x, st, act, sums, gamma, dx):
        """dx = gamma * rstd * (g - sum g / N - xhat * sum g xhat / N) (csb_bwd_apply); without the last two terms when st is an
        evaluation-mode state.  gamma fp32 [C] or None."""
        self._chk(dy, x, st, sums, gamma, dx)
        M, C = self._bn_shape(x, "bn_bwd_apply")
        lddy = self._rows(dy, _F32_BF16, M, C, "bn_bwd_apply: dy", (4, 8), 16)
        ldx = self._rows(x, _F32_BF16, M, C, "bn_bwd_apply: x", (4, 8), 16)
        lddx = self._rows(dx, _F32_BF16, M, C, "bn_bwd_apply: dx", (4, 8), 16)
        self._bn_vec(st, 4 * C + BN_ST_EXTRA, "bn_bwd_apply: st")
        self._bn_vec(sums, 2 * C, "bn_bwd_apply: sums")
        self._bn_vec(gamma, C, "bn_bwd_apply: gamma", optional=True)
        self._bn_rc(self.lib.csb_bwd_apply(_p(dy), lddy, _dt(dy), _p(x), ldx, _dt(x), _p(st), self._bn_act(act), _p(sums), _p(gamma), _p(dx), lddx,
                                           _dt(dx), M, C, self._bn_stream(x)), "csb_bwd_apply")

    # -- detector mask branch (include/clipself_mask.h) --------------------------------------------------
    def mask_workspace(self, R) -> int:
        """Bytes of workspace (csm_workspace) for mask_loss on R rows; 0 outside the limits."""
        return self._size("csm_workspace", int(R))

    def mask_target(self, rois, gt_rows, masks, M, soft=False, out=None):
        """mask_target / BitmapMasks.crop_and_resize (csm_mask_target).  rois [R, 5] fp32 contiguous (image, x0, y0, x1, y1), gt_rows [R]
        int32 (rows outside [0, Gtot) give zero targets), masks [Gtot, H, W] uint8 with last stride 1 (its row and plane strides are
        passed on).  -> targets [R, M, M], uint8 (t >= 0.5) or, with soft=True, fp32.  Nothing is read back."""
        self._chk(rois, gt_rows, masks)
        R, M = rois.shape[0], int(M)
        self._dense(rois, torch.float32, (R, 5), "mask_target: rois")
        self._dense(gt_rows, torch.int32, (R,), "mask_target: gt_rows")
        if masks.dtype != torch.uint8 or masks.dim() != 3 or (masks.numel() and masks.stride(2) != 1):
            raise ValueError(f"mask_target: masks must be uint8 [Gtot, H, W] with last stride 1, got {masks.dtype} {tuple(masks.shape)}")
        Gtot, H, W = masks.shape
        ldm = max(masks.stride(1), W) if H > 1 else W
        plane = max(masks.stride(0), H * ldm) if Gtot > 1 else H * ldm
        if not (1 <= M <= MASK_MAX_MASK and 1 <= H <= MASK_MAX_SIDE and 1 <= W <= MASK_MAX_SIDE and 0 <= R <= MASK_MAX_ROWS):
            raise ValueError(f"mask_target: limits 1 <= M <= {MASK_MAX_MASK}, 1 <= H, W <= {MASK_MAX_SIDE}, R <= {MASK_MAX_ROWS} "
                             f"(M = {M}, H = {H}, W = {W}, R = {R})")
        dt = torch.float32 if soft else torch.uint8
        if out is None:
            out = torch.empty(R, M, M, dtype=dt, device=rois.device)
        self._dense(out, dt, (R, M, M), "mask_target: out")
        self._ok(self.lib.csm_mask_target(_p(rois), _p(gt_rows), R, _p(masks), Gtot, H, W, ldm, plane, M, int(bool(soft)), _p(out),
                                          self._stream()), "csm_mask_target")
        return out

    def mask_loss(self, pred, labels, targets, row_weights, grad=True, out=None, workspace=None):
        """FCNMaskHead.loss / mask_cross_entropy with its gradient in one call (csm_mask_loss).  pred [R, C, M, M] fp32 contiguous, labels
        [R] int32 or None (channel 0), targets [R, M, M] uint8 or fp32, row_weights [R] fp32.  -> (out2 = (loss, n) [2], dpred like pred),
        dpred None with grad=False.  out: the same pair, to own the outputs.  The workspace is cached per device (pass workspace= to own
        it); calls that share it must share a stream."""
        self._chk(pred, labels, targets, row_weights)
        if pred.dim() != 4 or pred.shape[2] != pred.shape[3]:
            raise ValueError(f"mask_loss: pred must be [R, C, M, M], got {tuple(pred.shape)}")
        R, C, M, _ = pred.shape
        f32 = torch.float32
        self._dense(pred, f32, (R, C, M, M), "mask_loss: pred")
        if labels is not None:
            self._dense(labels, torch.int32, (R,), "mask_loss: labels")
        if targets.dtype not in (torch.uint8, f32):
            raise ValueError(f"mask_loss: targets must be uint8 or fp32, got {targets.dtype}")
        self._dense(targets, targets.dtype, (R, M, M), "mask_loss: targets")
        self._dense(row_weights, f32, (R,), "mask_loss: row_weights")
        dev = pred.device
        if out is None:
            out2, dpred = torch.empty(2, dtype=f32, device=dev), (torch.empty_like(pred) if grad else None)
        else:
            out2, dpred = out
        self._dense(out2, f32, (2,), "mask_loss: out")
        if dpred is not None:
            self._dense(dpred, f32, (R, C, M, M), "mask_loss: dpred")
        ws = self._workspace("clipself_mask.h", self.mask_workspace(R) if R * C * M * M < 1 << 31 else 0, dev, workspace, "mask_loss")
        self._ok(self.lib.csm_mask_loss(_p(pred), _p(labels), _p(targets), int(targets.dtype == f32), _p(row_weights), R, C, M, _p(out2),
                                        _p(dpred), _p(ws), self._stream()), "csm_mask_loss")
        return out2, dpred

    def paste_masks(self, logits, labels, boxes, img_h, img_w, thr=0.5, out=None, soft=None):
        """FCNMaskHead.get_seg_masks / _do_paste_mask (csm_paste_masks).  logits [N, C, M, M] fp32 contiguous, labels [N] int32 or None
        (channel 0), boxes [N, 4] fp32 contiguous in output-image pixels.  -> out [N, img_h, img_w] uint8 = (v >= thr); soft: an fp32
        tensor of the same shape that receives v (a test aid).  Nothing is read back."""
        self._chk(logits, labels, boxes, out, soft)
        if logits.dim() != 4 or logits.shape[2] != logits.shape[3]:
            raise ValueError(f"paste_masks: logits must be [N, C, M, M], got {tuple(logits.shape)}")
        N, C, M, _ = logits.shape
        img_h, img_w = int(img_h), int(img_w)
        self._dense(logits, torch.float32, (N, C, M, M), "paste_masks: logits")
        if labels is not None:
            self._dense(labels, torch.int32, (N,), "paste_masks: labels")
        self._dense(boxes, torch.float32, (N, 4), "paste_masks: boxes")
        if out is None:
            out = torch.empty(N, img_h, img_w, dtype=torch.uint8, device=logits.device)
        self._dense(out, torch.uint8, (N, img_h, img_w), "paste_masks: out")
        if soft is not None:
            self._dense(soft, torch.float32, (N, img_h, img_w), "paste_masks: soft")
        self._ok(self.lib.csm_paste_masks(_p(logits), _p(labels), _p(boxes), N, C, M, img_h, img_w, float(thr), _p(out), _p(soft),
                                          self._stream()), "csm_paste_masks")
        return out

    # -- detector RoI extractor (include/clipself_roi.h) -------------------------------------------------
    def roi_extract_workspace(self, K) -> int:
        return self._size("csr_roi_extract_workspace", int(K))

    def _roi_levels(self, maps, grids, scales, B):
        """maps[l]: the level's channel-last map as a 2-D view [B * h_l * w_l, C] (row = one cell, last stride 1, its own row stride);
        grids[l] = (h_l, w_l); scales[l] = 1 / stride_l.  -> (csr_level array, L, C).  Limits are the library's to refuse."""
        L = len(maps)
        if not (len(grids) == L and len(scales) == L and L >= 1):
            raise ValueError(f"roi_extract: {L} maps, {len(grids)} grids and {len(scales)} scales")
        C = maps[0].shape[1]
        arr = (RoiLevel * L)()
        for l, (m, (h, w), s) in enumerate(zip(maps, grids, scales)):
            ld = self._rows(m, _F32, B * int(h) * int(w), C, f"roi_extract: level {l}")
            arr[l] = RoiLevel(m.data_ptr(), ld, int(h), int(w), float(s))      # 1.0 / stride in double; the c_float field rounds it once
        return arr, L, C

    def roi_extract_fwd(self, maps, grids, scales, rois, out, B, P, sampling_ratio=0, finest_scale=56.0):
        """Multi-level RoIAlign (csr_roi_extract_fwd): rois [K, 5] fp32 (image, x0, y0, x1, y1) -> out, the [K, P, P, C] bins as a 2-D
        view [K * P * P, C].  maps / grids / scales: see _roi_levels; scales[l] = (float)(1 / stride_l)."""
        self._chk(rois, out, *maps)
        K = rois.shape[0]
        self._dense(rois, torch.float32, (K, 5), "roi_extract: rois")
        arr, L, C = self._roi_levels(maps, grids, scales, B)
        ldo = self._rows(out, _F32, K * P * P, C, "roi_extract: out")
        self._ok(self.lib.csr_roi_extract_fwd(arr, L, int(B), C, _p(rois), K, int(P), int(sampling_ratio), float(finest_scale), _p(out), ldo,
                                              self._stream()), "csr_roi_extract_fwd")
        return out

    def roi_extract_bwd(self, dout, rois, dmaps, grids, scales, B, P, sampling_ratio=0, finest_scale=56.0, workspace=None):
        """dmaps[l] += the gradient of roi_extract_fwd's out with respect to level l, all levels in one call (csr_roi_extract_bwd): a
        gather in ascending box row, no floating-point atomics, equal bits from equal inputs.  The workspace is this header's one
        buffer per device (pass workspace= to own it); calls that share it must share a stream."""
        self._chk(rois, dout, workspace, *dmaps)
        K = rois.shape[0]
        self._dense(rois, torch.float32, (K, 5), "roi_extract: rois")
        arr, L, C = self._roi_levels(dmaps, grids, scales, B)
        ldo = self._rows(dout, _F32, K * P * P, C, "roi_extract: dout")
        workspace = self._workspace("clipself_roi.h", self.roi_extract_workspace(K), rois.device, workspace, "roi_extract_bwd")
        self._ok(self.lib.csr_roi_extract_bwd(_p(dout), ldo, _p(rois), K, int(P), int(sampling_ratio), float(finest_scale), arr, L, int(B), C,
                                              _p(workspace), self._stream()), "csr_roi_extract_bwd")
        return dmaps

    def roialign_bwd(self, dpooled, rois, dfeat, grid_h, grid_w, tok_off):
        self._chk(dpooled, rois, dfeat)
        B, Ntok, E = dfeat.shape
        self._ok(self.lib.cs_roialign_bwd(_p(dpooled), _p(rois), _p(dfeat), rois.shape[0], B, Ntok, grid_h, grid_w, E, tok_off,
                                          self._stream()), "cs_roialign_bwd")

    def cosine_loss_fwd(self, student, teacher, stats, loss, weight):
        self._chk(student, teacher, stats, loss)
        K, E = student.shape
        self._ok(self.lib.cs_cosine_loss_fwd(_p(student), _p(teacher), _p(stats), _p(loss), K, E, weight, self._stream()),
                 "cs_cosine_loss_fwd")

    def cosine_loss_bwd(self, student, teacher, stats, dstudent, weight, grad_scale=1.0, upstream=None):
        self._chk(student, teacher, stats, dstudent, upstream)
        K, E = student.shape
        self._ok(self.lib.cs_cosine_loss_bwd(_p(student), _p(teacher), _p(stats), _p(dstudent), K, E, weight, grad_scale,
                                             _p(upstream), self._stream()), "cs_cosine_loss_bwd")

    def fed_bce_fwd(self, logits, tgt, rowloss, loss, ns, temp, weight):
        self._chk(logits, tgt, rowloss, loss)
        assert tgt.dtype == torch.int32
        self._ok(self.lib.cs_fed_bce_fwd(_p(logits), logits.stride(0), _p(tgt), _p(rowloss), _p(loss), logits.shape[0], ns, temp, weight,
                                         self._stream()), "cs_fed_bce_fwd")

    def fed_bce_bwd(self, logits, tgt, dz, ns, temp, weight, upstream=None):
        self._chk(logits, tgt, dz, upstream)
        assert dz.stride(1) == 1 and dz.stride(0) == dz.shape[1], "fed_bce_bwd writes whole rows (zeros in [ns, ldd)): dz must be contiguous"
        self._ok(self.lib.cs_fed_bce_bwd(_p(logits), logits.stride(0), _p(tgt), _p(dz), dz.stride(0), logits.shape[0], ns, temp, weight,
                                         _p(upstream), self._stream()), "cs_fed_bce_bwd")

    @staticmethod
    def adamw_guard_numel(n: int) -> int:
        """Floats of the guard buffer of adamw_step for n parameters: the head + one partial sum of squares per span."""
        return ADAMW_GUARD_HEAD + (int(n) + ADAMW_GUARD_SPAN - 1) // ADAMW_GUARD_SPAN

    def adamw_step(self, p, g, m, v, shadow, flags, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False,
                   guard=None):
        """guard (fp32, adamw_guard_numel(n) floats, zeroed once by the caller): the step also leaves the gradient norm, the clip coefficient
        of max_norm (<= 0: no clipping), applied / skipped and the count of skipped steps in guard[0..3] -- include/clipself_hip.h."""
        self._chk(p, g, m, v, shadow, flags, guard)
        if guard is not None:
            assert guard.dtype == torch.float32 and guard.is_contiguous() and guard.numel() >= self.adamw_guard_numel(p.numel())
        self._ok(self.lib.cs_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(shadow), _p(flags), p.numel(), lr, beta1, beta2, eps, wd,
                                        step, grad_scale, max_norm, int(bool(skip_nonfinite)), _p(guard), self._stream()), "cs_adamw_step")
