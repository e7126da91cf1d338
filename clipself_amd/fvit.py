"""Detector backbone on the frozen HIP tower: `EvaCLIPViT`, shaped like the reference's F-ViT backbone
(F-ViT/models/evaclip_vit.py:13-122) so that a detector built on a CLIPSelf checkpoint can keep its configs.

The reference drives `visual.patch_embed`, `visual.blocks[i]`, `visual.norm` and `visual.head` module by module under no_grad and copies
the token stream out after four blocks (`_expand_x`).  Here the whole frozen pass is one call, EVAVisionTower.forward_intermediates ->
TowerEngine.encode_dense(taps=...): the blocks update the fp32 residual stream in place and the token-taps kernel (HipOps.tokens_to_nchw)
writes each tapped block's output as a [B, width, h, w] map before the next block overwrites it.  What trains -- the neck of transposed
convolutions, `interpolate1` .. `interpolate4` -- keeps the reference's parameter names; like any nn.Module it is built on the CPU and
placed by its owner (`.cuda()` / `.to(device)`: the tower already lives on the engine's device and stays there).  Its three transposed
convolutions are neck.Deconv2x2: nn.ConvTranspose2d by state dict and by default behaviour, and with `fused_neck` GEMMs on the token
stream (taps 0 and 1 then arrive as the tower's bf16 rows, not as maps); norm and GELU stay torch.

mmdet / mmcv are optional: when mmdet can be imported the class is registered with its BACKBONES registry under the reference's name,
otherwise it is an ordinary nn.Module.
"""
from __future__ import annotations

import logging

from torch import nn

from .neck import Deconv2x2
from .open_clip.factory import create_model

# What EvaCLIPViT(fused_neck=None) chooses on a backend that has the fused path.  On: forward + backward of the neck takes 0.72x / 0.72x the
# time of the faster torch variant (bf16 autocast) at the B/16 and L/14-336 detector shapes on the MI355X (profiles/neck_bench.md).
FUSED_NECK_DEFAULT = True


def build_norm(norm_cfg, channels: int) -> nn.Module:
    """The normalisation layers the shipped F-ViT configs ask mmcv's build_norm_layer for (`dict(type='SyncBN', requires_grad=True)`;
    'BN' for single-process runs), as torch layers; None / {} -> Identity (evaclip_vit.py:28)."""
    if not norm_cfg:
        return nn.Identity()
    cfg = dict(norm_cfg)
    kind = cfg.pop("type")
    requires_grad = cfg.pop("requires_grad", True)
    layers = {"BN": nn.BatchNorm2d, "BN2d": nn.BatchNorm2d, "SyncBN": nn.SyncBatchNorm}
    if kind not in layers:
        raise NotImplementedError(f"norm_cfg type {kind!r}: the F-ViT configs use 'SyncBN' (or 'BN'); got {norm_cfg!r}")
    cfg.setdefault("eps", 1e-5)
    layer = layers[kind](channels, **cfg)
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return layer


class EvaCLIPViT(nn.Module):
    """forward(images [B, 3, S, S]) -> (interpolate1(tap0), interpolate2(tap1), interpolate3(tap2), interpolate4(tap3), feature_map):
    strides patch/4, patch/2, patch, 2*patch of the four tapped blocks' outputs and, in evaluation mode, the L2-normalised dense map
    [B, embed_dim, h, w] (None while training) -- evaclip_vit.py:61-115."""

    def __init__(self, model_name, pretrained, out_indices=[3, 5, 7, 11], norm_cfg=None, ops=None, fused_neck=None):
        """fused_neck: True = the neck's transposed convolutions run as GEMMs on the token stream (NotImplementedError on a kernel backend
        without DECONV_ROWS), False = torch's convolutions, None = FUSED_NECK_DEFAULT where the backend has the path, else torch."""
        super().__init__()
        self.vit_layers = list(out_indices)
        self.model_name = model_name
        self.pretrained = pretrained                      # the checkpoint file (the reference passes it as cache_dir)
        self._ops = ops
        clip_model = create_model(model_name, pretrained="eva", cache_dir=pretrained, ops=ops, trainable=False)
        self.embed_dim = clip_model.embed_dim            # output dim
        self.width = width = clip_model.visual.embed_dim
        self.patch_size = clip_model.visual.cfg.patch_size
        self.interpolate1 = nn.Sequential(
            Deconv2x2(width, width, kernel_size=2, stride=2),
            build_norm(norm_cfg, width),
            nn.GELU(),
            Deconv2x2(width, width, kernel_size=2, stride=2),
        )
        self.interpolate2 = nn.Sequential(
            Deconv2x2(width, width, kernel_size=2, stride=2),
        )
        self.interpolate3 = nn.Identity()
        self.interpolate4 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.visual = clip_model.visual
        backend = self.visual.engine.ops
        has = bool(getattr(backend, "DECONV_ROWS", False))
        if fused_neck and not has:
            raise NotImplementedError(f"EvaCLIPViT(fused_neck=True) needs the rows <-> NCHW copies of the 2x2 deconvolution GEMMs, which the "
                                      f"kernel backend {getattr(backend, 'name', type(backend).__name__)!r} does not provide (no DECONV_ROWS)")
        self.fused_neck = bool(FUSED_NECK_DEFAULT and has) if fused_neck is None else bool(fused_neck)
        if self.fused_neck:
            for layer in (self.interpolate1[0], self.interpolate1[3], self.interpolate2[0]):
                layer.ops = backend
        for param in self.visual.parameters():
            param.requires_grad = False

    def init_weights(self):
        """evaclip_vit.py:41-48: (re)load the tower from the checkpoint and freeze it; the neck keeps torch's default initialisation."""
        clip_model = create_model(self.model_name, pretrained="eva", cache_dir=self.pretrained, ops=self._ops, trainable=False)
        logging.info("%s", self.visual.load_state_dict(clip_model.visual.state_dict(), strict=True))
        for param in self.visual.parameters():          # only freeze the CLIP model
            param.requires_grad = False

    def train(self, mode=True):
        """evaclip_vit.py:50-59: the tower is always in evaluation mode, the neck follows `mode`."""
        self.training = mode
        self.visual.train(False)
        for i in range(1, 5):
            getattr(self, f"interpolate{i}").train(mode)
        return self

    def forward(self, x):
        bs, _, h, w = x.shape
        if h != w:
            raise NotImplementedError(f"the tower runs square inputs (the F-ViT pipelines pad to 1024 x 1024 / 896 x 896), got {h} x {w}")
        assert len(self.vit_layers) == 4
        # fused neck: taps 0 and 1 feed a Deconv2x2 and travel as the tower's bf16 rows when the layer will take them (width, device)
        lead = (self.interpolate1[0], self.interpolate2[0])
        rows = tuple(i for i, layer in enumerate(lead) if self.fused_neck and layer.fused_rows())
        outs, feature_map = self.visual.forward_intermediates(x, self.vit_layers, final_map=not self.training, rows=rows)
        assert len(outs) == 4
        for idx, out in enumerate(outs):
            interpolate = getattr(self, f"interpolate{idx + 1}")
            outs[idx] = interpolate(out if idx in rows else out.detach())
        outs.append(feature_map)
        return tuple(outs)


try:                                                      # optional: the reference registers the class with mmdet (evaclip_vit.py:13)
    from mmdet.models.builder import BACKBONES
    BACKBONES.register_module(name="EvaCLIPViT")(EvaCLIPViT)
except ImportError:
    pass
