"""mmdet's ConvFCBBoxHead as the F-ViT configs build it: the box head's trunk in front of the open-vocabulary scores.

F-ViT/models/fvit_head.py:14 derives FViTBBoxHead from mmdet.models.roi_heads.ConvFCBBoxHead and its forward (:72-107) walks that
module's lists: `shared_convs` (ConvModules), `x.flatten(1)`, `shared_fcs`, then the class branch (`cls_convs`, `cls_fcs`) and the box
branch (`reg_convs`, `reg_fcs`, `fc_reg`), every FC followed by ReLU.  Here the ConvModules are norm_act.ConvModule (conv.Conv3x3 +
norm_act.BatchNormAct2d), the FCs are linear.LinearAct(act="relu") -- the first shared FC with `spatial`, so the flatten moves no data --
and `fc_reg` (512 -> 4, 16 MFLOP) is linear.LinearThin where its width is <= 16 and its input a multiple of 64 (class-agnostic
regression, every F-ViT config), nn.Linear otherwise.  `fc_reg` has a switch of its own, `fused_reg` (None = conv.FUSED_THIN_DEFAULT,
which is off: F.linear); the head's `fused` is not handed to it.  The submodules carry mmdet's names, so a reference checkpoint's
box-head keys load with strict=True.

Two lines compose the training branch with ov_head.OpenVocabBoxScores:

    x_cls, bbox_pred = head(roi_feats)
    cls_score = scores.class_logits(x_cls)

The initialisation follows mmdet's init_cfg for this module (bbox_head.py: Normal std 0.01 for fc_cls, 0.001 for fc_reg;
convfc_bbox_head.py: Xavier uniform for shared_fcs / cls_fcs / reg_fcs).  mmdet is not installed beside this project, so that part is
cited, not run: parity-unpinned, for the initialisation only.
"""
from __future__ import annotations

from torch import nn

from .linear import THIN_MAX_N, LinearAct, LinearThin
from .norm_act import ConvModule


class ConvFCBBoxHead(nn.Module):
    """ConvFCBBoxHead(**the config's bbox_head dict).  forward(x [K, in_channels, s, s]) -> (x_cls [K, fc_out_channels], bbox_pred [K, 4 |
    4 * num_classes]): fvit_head.py:72-107 up to the class branch's output, which goes to OpenVocabBoxScores.class_logits unchanged.

    ops / fused are handed to every kernel-backed submodule (see det_layer.KernelLayer) but fc_reg, which takes ops / fused_reg; on its
    kernel route bbox_pred is fp32 whatever the input's dtype."""

    def __init__(self, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_shared_convs=0, num_shared_fcs=0, num_cls_convs=0,
                 num_cls_fcs=0, num_reg_convs=0, num_reg_fcs=0, conv_out_channels=256, num_classes=80, reg_class_agnostic=False,
                 norm_cfg=None, ops=None, fused=None, fused_reg=None,
                 # What belongs to other modules here and is accepted so that a config dict can be passed whole:
                 #   bbox_coder                        -> det_post.delta2bbox / det_targets.bbox_targets
                 #   loss_cls, loss_bbox               -> det_losses.BBoxHeadLoss
                 #   fixed_temperature, learned_temperature, vlm_temperature, alpha, beta, learn_bg, class_embed, seen_classes,
                 #   all_classes                       -> ov_head.OpenVocabBoxScores
                 #   type, init_cfg                    -> mmdet's registry and initialiser
                 **other_modules):
        super().__init__()
        assert num_shared_convs + num_shared_fcs + num_cls_convs + num_cls_fcs + num_reg_convs + num_reg_fcs > 0
        if num_cls_convs > 0 or num_reg_convs > 0:
            assert num_shared_fcs == 0                                 # convfc_bbox_head.py:40-41
        self.in_channels, self.fc_out_channels, self.conv_out_channels = in_channels, fc_out_channels, conv_out_channels
        self.roi_feat_size = roi_feat_size if isinstance(roi_feat_size, int) else roi_feat_size[0]
        assert isinstance(roi_feat_size, int) or roi_feat_size[0] == roi_feat_size[1], "square RoI features"
        self.roi_feat_area = self.roi_feat_size ** 2
        self.num_shared_convs, self.num_shared_fcs = num_shared_convs, num_shared_fcs
        self.num_cls_convs, self.num_cls_fcs, self.num_reg_convs, self.num_reg_fcs = num_cls_convs, num_cls_fcs, num_reg_convs, num_reg_fcs
        self.num_classes, self.reg_class_agnostic = num_classes, reg_class_agnostic
        self.norm = norm_cfg is not None
        self.ops, self.fused, self.fused_reg = ops, fused, fused_reg

        self.shared_convs, self.shared_fcs, last, spatial = self._branch(num_shared_convs, num_shared_fcs, in_channels, True)
        self.shared_out_channels = last
        self.cls_convs, self.cls_fcs, self.cls_last_dim, _ = self._branch(num_cls_convs, num_cls_fcs, last, spatial)
        self.reg_convs, self.reg_fcs, self.reg_last_dim, _ = self._branch(num_reg_convs, num_reg_fcs, last, spatial)
        if num_shared_fcs == 0:                                        # convfc_bbox_head.py:71-75: a branch without FCs is flattened at its end
            if num_cls_fcs == 0:
                self.cls_last_dim *= self.roi_feat_area
            if num_reg_fcs == 0:
                self.reg_last_dim *= self.roi_feat_area
        # fc_cls is part of the state dict and unused by the forward, as in FViTBBoxHead (the class scores come from the embeddings)
        self.fc_cls = nn.Linear(self.cls_last_dim, num_classes + 1)
        reg_width = 4 if reg_class_agnostic else 4 * num_classes
        if reg_width <= THIN_MAX_N and self.reg_last_dim % 64 == 0:    # every F-ViT config: class-agnostic regression
            self.fc_reg = LinearThin(self.reg_last_dim, reg_width, ops=ops, fused=fused_reg)
        else:
            self.fc_reg = nn.Linear(self.reg_last_dim, reg_width)
        self.init_weights()

    def _branch(self, num_convs, num_fcs, in_channels, spatial):
        """convfc_bbox_head.py:96-126 (_add_conv_fc_branch): convs, then fcs; -> (convs, fcs, last width, whether the output is still a map).
        The FC that meets a map is the one built with `spatial`."""
        convs, fcs, last = nn.ModuleList(), nn.ModuleList(), in_channels
        for i in range(num_convs):
            convs.append(ConvModule(last, self.conv_out_channels, norm=self.norm, ops=self.ops, fused=self.fused))
            last = self.conv_out_channels
        for i in range(num_fcs):
            on_map = spatial and i == 0
            fcs.append(LinearAct(last * self.roi_feat_area if on_map else last, self.fc_out_channels, act="relu",
                                 spatial=(last, self.roi_feat_area) if on_map else None, ops=self.ops, fused=self.fused))
            last = self.fc_out_channels
        return convs, fcs, last, spatial and num_fcs == 0

    def init_weights(self):
        for fcs in (self.shared_fcs, self.cls_fcs, self.reg_fcs):
            for m in fcs:
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.zeros_(self.fc_cls.bias)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.zeros_(self.fc_reg.bias)

    @staticmethod
    def _run(x, convs, fcs):
        for conv in convs:
            x = conv(x)
        if x.dim() > 2 and (len(fcs) == 0 or fcs[0].spatial is None):
            x = x.flatten(1)
        for fc in fcs:
            x = fc(x)                                                  # Linear + ReLU: fvit_head.py:83, 96, 105
        return x

    def forward(self, x):
        for conv in self.shared_convs:
            x = conv(x)
        for fc in self.shared_fcs:                                     # the first one takes the map: fvit_head.py:80 without the copy
            x = fc(x)
        x_cls = self._run(x, self.cls_convs, self.cls_fcs)
        x_reg = self._run(x, self.reg_convs, self.reg_fcs)
        return x_cls, self.fc_reg(x_reg)
