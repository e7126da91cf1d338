"""mmdet's FCNMaskHead as the F-ViT configs build it: the mask branch between the RoI extractor and det_masks.

`convs` (num_convs ConvModules: conv.Conv3x3 + norm_act.BatchNormAct2d with the ReLU), `upsample` (ConvTranspose2d(k=2, s=2):
neck.Deconv2x2), ReLU, `conv_logits` (1 x 1 to 1 | num_classes channels).  The submodules carry mmdet's names (`convs.{i}.conv.*`,
`convs.{i}.bn.*`, `upsample.*`, `conv_logits.*`), so a reference checkpoint's mask-head keys load with strict=True.

With class_agnostic=True (the configs' form) the tail -- deconvolution, ReLU, logits -- runs on the RoI rows [K*196, C] without ever
laying the [K, C, 28, 28] map out:
    1. cs_gemm_nt epilogue 9 with Deconv2x2.gemm_weights(): bf16 [K*196, 4*C] = relu(X . Wg^T + bias), a row's four C-wide quarters being
       the four output pixels (2i + di, 2j + dj) of input pixel (i, j);
    2. that buffer as rows [4*K*196, C] through HipOps.thin_fwd (rows form, N = 1 | num_classes <= 16): the logits, 4 bytes per pixel;
    3. a torch permutation of the [K, 14, 14, 2, 2, N] logits to [K, N, 28, 28].
The backward is the inverse permutation, HipOps.thin_dgrad with the saved activation as the ReLU's gate, the deconvolution's own
pieces (det_layer.wgrad, colsum_bf16, gemm_nt with Wg^T) on those rows, and conv_logits' gradients as in conv.Conv1x1Thin: the rows form
of HipOps.thin_wgrad on the fp32 dL and the saved activation where conv.thin_wgrad_direct holds, the padded bf16 rows otherwise.

The initialisation follows mmdet's FCNMaskHead.init_weights (Kaiming normal, mode='fan_out', nonlinearity='relu', zero biases for
`upsample` and `conv_logits`).  mmdet is not installed beside this project, so that part is cited, not run: parity-unpinned.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .conv import THIN_MAX_N, Conv1x1, Conv1x1Thin, thin_param_grads, thin_wgrad_direct
from .det_layer import BF16, EPI_RELU_BF16, F32, epi_for, row_chunks, rows_bf16, rows_to_map, uncovered, wgrad
from .neck import Deconv2x2
from .norm_act import ConvModule, apply_norm_cfg


class FCNMaskHead(nn.Module):
    """FCNMaskHead(**the config's mask_head dict).  forward(x [K, in_channels, s, s]) -> mask logits [K, 1 | num_classes, 2s, 2s]; fp32
    on the kernel route.

    ops / fused are handed to every kernel-backed submodule (see det_layer.KernelLayer); the fused tail additionally needs
    conv_out_channels % 64 == 0 and a logits width <= 16."""

    def __init__(self, num_convs=4, in_channels=256, conv_out_channels=256, num_classes=80, class_agnostic=False, norm_cfg=None,
                 upsample_cfg=None, ops=None, fused=None,
                 # What belongs to other modules here and is accepted so that a config dict can be passed whole:
                 #   loss_mask                  -> det_masks.mask_loss
                 #   roi_feat_size, predictor_cfg, conv_kernel_size (3 is the only one built), type, init_cfg -> mmdet's
                 **other_modules):
        super().__init__()
        upsample_cfg = dict(type="deconv", scale_factor=2) if upsample_cfg is None else dict(upsample_cfg)
        if upsample_cfg.get("type") != "deconv" or upsample_cfg.get("scale_factor", 2) != 2:
            raise NotImplementedError(f"FCNMaskHead: upsample_cfg={upsample_cfg!r} is not built here (dict(type='deconv', scale_factor=2) only)")
        if other_modules.get("conv_kernel_size", 3) != 3:
            raise NotImplementedError(f"FCNMaskHead: conv_kernel_size={other_modules['conv_kernel_size']!r} is not built here (3 only)")
        self.num_convs, self.in_channels, self.conv_out_channels = num_convs, in_channels, conv_out_channels
        self.num_classes, self.class_agnostic = num_classes, class_agnostic
        self.ops, self.fused = ops, fused
        self.convs = nn.ModuleList(ConvModule(in_channels if i == 0 else conv_out_channels, conv_out_channels, norm=norm_cfg is not None,
                                              ops=ops, fused=fused) for i in range(num_convs))
        up_in = conv_out_channels if num_convs > 0 else in_channels
        self.upsample = Deconv2x2(up_in, conv_out_channels, ops=None if fused is False else ops)      # fused=False: torch throughout
        width = 1 if class_agnostic else num_classes
        if width <= THIN_MAX_N:
            self.conv_logits = Conv1x1Thin(conv_out_channels, width, ops=ops, fused=fused)
        else:
            self.conv_logits = Conv1x1(conv_out_channels, width, ops=ops, fused=fused)
        apply_norm_cfg(self, norm_cfg)
        self.init_weights()

    def init_weights(self):
        for m in (self.upsample, self.conv_logits):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            nn.init.zeros_(m.bias)

    def tail_backend(self, x):
        """The backend that runs deconvolution + ReLU + logits on the RoI rows for the map x in front of `upsample`, or None (-> the
        layers one by one); NotImplementedError where fused=True cannot be met."""
        lg, up = self.conv_logits, self.upsample
        if not isinstance(lg, Conv1x1Thin):
            return None
        k = lg.kernel_backend(x) if up.in_channels == lg.in_channels else None
        if k is None:
            return None
        ok = (getattr(k, "LINEAR_ACT", False) and up.in_channels % 64 == 0 and up.out_channels % 64 == 0 and up.weight.dtype == F32
              and up.weight.device == x.device and up.bias is not None)
        if not ok:
            return uncovered(self.fused, f"FCNMaskHead's tail ({up.in_channels} -> {up.out_channels} -> {lg.out_channels})",
                             "channels % 64 == 0, fp32 parameters, a backend with LINEAR_ACT")
        return k

    def forward(self, x):
        for conv in self.convs:
            x = conv(x)
        k = self.tail_backend(x)
        if k is None:
            return self.conv_logits(F.relu(self.upsample(x)))
        up, lg = self.upsample, self.conv_logits
        return _MaskTailFn.apply(x, up.weight, up.bias, lg.weight, lg.bias, self, k)


class _MaskTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, up_w, up_b, lg_w, lg_b, head, ops):
        up, lg = head.upsample, head.conv_logits
        K, Cin, h, w = x.shape
        Cout, Nl, M = up.out_channels, lg.out_channels, K * h * w
        Wg, _, bias4 = up.gemm_weights()
        Wl, bl = lg.gemm_weights()
        X = rows_bf16(ops, x)
        keep = any(ctx.needs_input_grad[:5])
        act = ops.empty((M, 4 * Cout), BF16) if keep else None              # relu(deconv) on the rows: the gate and conv_logits' operand
        L = ops.empty((4 * M, Nl), F32)
        buf = None
        for r0, n in row_chunks(M, 4 * Cout * 2):
            if keep:
                Y = act[r0:r0 + n]
            else:
                if buf is None or buf.shape[0] != n:
                    buf = ops.empty((n, 4 * Cout), BF16)
                Y = buf
            ops.gemm_nt(X[r0:r0 + n], Wg, Y, bias4, epi=EPI_RELU_BF16)
            ops.thin_fwd(Y.view(4 * n, Cout), Wl, bl, L[4 * r0:4 * (r0 + n)], R=0)
        ctx.head, ctx.ops, ctx.geom, ctx.x_dtype = head, ops, (K, h, w), x.dtype
        if keep:
            ctx.save_for_backward(X, act)
        return L.view(K, h, w, 2, 2, Nl).permute(0, 5, 1, 3, 2, 4).reshape(K, Nl, 2 * h, 2 * w)

    @staticmethod
    def backward(ctx, d_out):
        head, ops = ctx.head, ctx.ops
        up, lg = head.upsample, head.conv_logits
        K, h, w = ctx.geom
        Cin, Cout, Nl, M = up.in_channels, up.out_channels, lg.out_channels, K * h * w
        X, act = ctx.saved_tensors
        need_x, need_uw, need_ub, need_lw, need_lb = ctx.needs_input_grad[:5]
        _, WgT, _ = up.gemm_weights()
        Wl, _ = lg.gemm_weights()
        dL = d_out.to(F32).reshape(K, Nl, h, 2, w, 2).permute(0, 2, 4, 3, 5, 1).reshape(4 * M, Nl).contiguous()
        A4 = act.view(4 * M, Cout)
        dx = duw = dub = dlw = dlb = None
        if (need_lw or need_lb) and thin_wgrad_direct(ops):                  # the rows form of epilogue 12: dL and the activation in place
            ((dlw, dlb),) = thin_param_grads(ops, lg, dL, A4, [Nl], [(need_lw, need_lb)], R=0)
        elif need_lw or need_lb:
            dLr = ops.zeros((4 * M, THIN_MAX_N), BF16)
            dLr[:, :Nl] = dL
            ((dlw, dlb),) = thin_param_grads(ops, lg, dLr, A4, [Nl], [(need_lw, need_lb)])
        if need_x or need_uw or need_ub:
            dA = ops.empty((4 * M, Cout), BF16)
            ops.thin_dgrad(dL, Wl, dA, R=0, gate=A4)                          # through conv_logits and the ReLU in one pass
            dY = dA.view(M, 4 * Cout)
            if need_uw:
                dWg = ops.zeros((4 * Cout, Cin), F32)
                wgrad(ops, up, dY, X, dWg)
                duw = dWg.view(2, 2, Cout, Cin).permute(3, 2, 0, 1).contiguous()
            if need_ub:
                col = ops.zeros((4 * Cout,), F32)
                ops.colsum_bf16(dY, col)
                dub = col.view(4, Cout).sum(0)
            if need_x:
                dXr = ops.empty((M, Cin), ctx.x_dtype)
                ops.gemm_nt(dY, WgT, dXr, None, epi=epi_for(ctx.x_dtype))
                dx = rows_to_map(dXr, K, h, w)
        return dx, duw, dub, dlw, dlb, None, None
