"""The F-ViT detector's RPN head: F-ViT/models/custom_rpn_head.py `CustomRPNHead` on mmdet's `RPNHead`.

A shared stack of 3 x 3 convolutions (`rpn_conv`: norm_act.ConvModule, i.e. conv.Conv3x3 + norm_act.BatchNormAct2d carrying the ReLU) and
the two 1 x 1 heads `rpn_cls` (feat_channels -> A * cls_out_channels) and `rpn_reg` (feat_channels -> 4 A), A anchors per position.  The
heads are conv.Conv1x1Thin and run through conv.thin_heads: ONE pass over a level's 256-channel map writes both outputs as the contiguous
NCHW fp32 tensors that the loss and the proposal stage read without a copy.  The submodules carry mmdet's names (`rpn_conv.{i}.conv.*`,
`rpn_conv.{i}.bn.*`, `rpn_cls.*`, `rpn_reg.*`; `rpn_conv.*` itself for num_convs == 1), so a reference checkpoint's keys load with
strict=True.

The training step continues with the modules that exist already:

    cls_scores, bbox_preds = head(feats)                                       # two lists over the levels
    targets = det_targets.rpn_targets(anchors, valid, gt_boxes, ...)           # labels, label weights, box targets, box weights
    losses = det_losses.rpn_loss(cls_scores, bbox_preds, *targets)             # reads the NCHW fp32 maps as they are
    proposals = det_proposals.rpn_proposals(cls_scores, bbox_preds, anchors, img_shapes, ...)

The initialisation follows mmdet's init_cfg for RPNHead (dense_heads/rpn_head.py: Normal, layer='Conv2d', std=0.01, hence zero biases).
mmdet is not installed beside this project, so that part is cited, not run: parity-unpinned, for the initialisation only.
"""
from __future__ import annotations

import torch.nn.functional as F
from torch import nn

from .conv import Conv1x1Thin, Conv3x3, thin_heads
from .norm_act import ConvModule, apply_norm_cfg


class RPNHead(nn.Module):
    """RPNHead(**the config's rpn_head dict).  forward(feats) -> (cls_scores, bbox_preds): per level [B, A * cls_out_channels, h, w] and
    [B, 4 A, h, w]; contiguous NCHW fp32 on the kernel route.  mmdet's forward_single applies F.relu after rpn_conv; behind a ConvModule
    that ends in ReLU it is the identity and is skipped.

    ops / fused are handed to every kernel-backed submodule (see det_layer.KernelLayer)."""

    def __init__(self, in_channels, feat_channels=256, anchor_generator=None, num_convs=1, norm_cfg=None, ops=None, fused=None,
                 # What belongs to other modules here and is accepted so that a config dict can be passed whole:
                 #   bbox_coder                 -> det_post.delta2bbox / det_targets
                 #   loss_cls, loss_bbox        -> det_losses.rpn_loss (loss_cls.use_sigmoid also sets cls_out_channels here)
                 #   train_cfg, test_cfg        -> det_targets.rpn_targets / det_proposals.rpn_proposals
                 #   type, init_cfg             -> mmdet's registry and initialiser
                 **other_modules):
        super().__init__()
        if anchor_generator is None:
            anchor_generator = dict(scales=[8, 16, 32], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64])     # mmdet's AnchorHead default
        scales = anchor_generator.get("scales")
        if scales is None:                                                # AnchorGenerator: octave_base_scale * 2^(i / scales_per_octave)
            scales = range(anchor_generator["scales_per_octave"])
        self.num_base_priors = len(scales) * len(anchor_generator["ratios"])
        self.cls_out_channels = 1 if other_modules.get("loss_cls", dict(use_sigmoid=True)).get("use_sigmoid", False) else 2
        self.in_channels, self.feat_channels, self.num_convs = in_channels, feat_channels, num_convs
        self.ops, self.fused = ops, fused
        if num_convs > 1:
            self.rpn_conv = nn.Sequential(*(ConvModule(in_channels if i == 0 else feat_channels, feat_channels, norm=norm_cfg is not None,
                                                       ops=ops, fused=fused) for i in range(num_convs)))
        else:
            self.rpn_conv = Conv3x3(in_channels, feat_channels, ops=ops, fused=fused)
        self.rpn_cls = Conv1x1Thin(feat_channels, self.num_base_priors * self.cls_out_channels, ops=ops, fused=fused)
        self.rpn_reg = Conv1x1Thin(feat_channels, self.num_base_priors * 4, ops=ops, fused=fused)
        apply_norm_cfg(self, norm_cfg)
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward_single(self, x):
        x = self.rpn_conv(x)
        if self.num_convs == 1:
            x = F.relu(x)
        return thin_heads(x, (self.rpn_cls, self.rpn_reg))

    def forward(self, feats):
        cls_scores, bbox_preds = [], []
        for x in feats:
            c, r = self.forward_single(x)
            cls_scores.append(c)
            bbox_preds.append(r)
        return cls_scores, bbox_preds
