"""Open-vocabulary box scores: the scoring tail of the reference's F-ViT heads, usable without mmdet.

`OpenVocabBoxScores` restates what makes the detector open-vocabulary (F-ViT/models/fvit_head.py):

  :267-277  vlm_roi_extractor([vlm_feat], rois)[..., 0, 0] -- a 1x1 aligned, adaptive RoIAlign with featmap_strides=[16] on pixel boxes;
  :63-70, 108-119 (FViTBBoxHead)  normalise the pooled feature, multiply by the class embeddings and vlm_temperature, softmax, and blend
            with the detector's softmax as det^(1-alpha) * vlm^alpha on base classes and det^(1-beta) * vlm^beta on novel classes;
  :290-347 (FViTTransferBBoxHead)  the same with one exponent for all classes (seen_classes=None here).

The convolutions and linears in front of `cls_score` are bbox_head.ConvFCBBoxHead (mmdet's module of that name on this project's layers);
FPN and RPN are mmdet's and stay there: this module takes the
class branch's output and the backbone's dense map (fvit.EvaCLIPViT's fifth output) and returns the blended scores [K, C].  `get_bboxes`
(:123-164) turns them into detections through det_post (box decoding, class-aware NMS and the cut as HIP kernels, no mmcv / mmdet).

Two routes.  FUSED (a kernel backend with BOX_SCORES, HipOps): one launch per call (cs_roialign_fwd's scoring form) that
reads the tower's token-major map in place -- the NCHW tensor forward_intermediates returns is a permuted view of it, no copy is made --
pools in torchvision's arithmetic (pixel box * 1/stride in fp32), and evaluates the blend in the log domain,
exp((1-w) log_softmax(det) + w log_softmax(vlm)), which equals the reference's softmax() ** p product in exact arithmetic and has no
0 ** x corner when a probability underflows.  FALLBACK (RefOps, CPU, or fused=False): ops.roialign_fwd on boxes converted to the
normalised form, then torch.  The conversion computes (x / (w * stride)) * w where torchvision computes x * (1 / stride): equal bits when
the stride is a power of two and the map side is exactly representable, not bit-equal otherwise (a relative 2^-23 on a box coordinate).
"""
from __future__ import annotations

import json

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .det_layer import param_steps

# What OpenVocabBoxScores(fused=None) chooses on a backend that has the fused path.  Off: at 8 x 1000 boxes on a 64 x 64 map the one-launch
# route takes 1.29 / 1.49 / 1.46 x the time of the composition (roialign_fwd + torch) at (E, C) = (512, 66) / (512, 1204) / (768, 1204) on the
# MI355X -- its grouped pooling phase and its logits phase both lose (profiles/ov_scores_bench.md, tools/ov_scores_bench.py).
FUSED_SCORES_DEFAULT = False


def _names(classes):
    if classes is None:
        return None
    if isinstance(classes, (list, tuple)):
        return list(classes)
    with open(classes) as f:
        return list(json.load(f))


def _load_embed(class_embed, names):
    """-> fp32 [C, E] in the order of `names` (a .pt dict name -> vector, as the reference loads it) or in file order."""
    if isinstance(class_embed, torch.Tensor):
        e = class_embed.detach().float()
    elif str(class_embed).endswith(".npy"):
        e = torch.from_numpy(np.load(class_embed).astype(np.float32))
    else:
        d = torch.load(class_embed, map_location="cpu")
        if isinstance(d, dict):
            if names is None:
                raise ValueError("a name -> vector embedding file needs all_classes (the row order)")
            e = torch.stack([torch.as_tensor(d[n]).float() for n in names], dim=0)        # fvit_head.py:46-48
        else:
            e = torch.as_tensor(d).float()
    if e.dim() != 2:
        raise ValueError(f"class embeddings must be [C, E], got {tuple(e.shape)}")
    if names is not None and e.shape[0] != len(names):
        raise ValueError(f"{e.shape[0]} embedding rows for {len(names)} classes (all_classes + 'background')")
    return e


class OpenVocabBoxScores(nn.Module):
    """forward(cls_score [K, C] | None, vlm_feat [B, E, h, w], rois [K, 5] = (image index, x0, y0, x1, y1) in pixels) -> scores [K, C].

    class_embed: a tensor [C, E], a .npy written by tools/text_embeddings.py (rows in the order all_classes + ['background']) or a .pt
    dict name -> vector.  seen_classes / all_classes: lists or json paths, 'background' is appended to both (fvit_head.py:38-39);
    seen_classes=None makes every class a base class -- the transfer head, one exponent alpha.  fused: True = the one-launch kernel
    (NotImplementedError on a backend without BOX_SCORES), False = the fallback route, None = FUSED_SCORES_DEFAULT where the backend has
    the kernel."""

    def __init__(self, class_embed, seen_classes=None, all_classes=None, vlm_temperature=100.0, alpha=0.2, beta=0.45, fixed_temperature=0,
                 learned_temperature=50.0, learn_bg=False, featmap_stride=16, ops=None, fused=None, target_means=(0., 0., 0., 0.),
                 target_stds=(0.1, 0.1, 0.2, 0.2), reg_class_agnostic=True):
        super().__init__()
        # the bbox_coder of every F-ViT config: DeltaXYWHBBoxCoder(target_means, target_stds), class-agnostic regression
        self.target_means, self.target_stds, self.reg_class_agnostic = tuple(target_means), tuple(target_stds), bool(reg_class_agnostic)
        assert class_embed is not None, "class embed is None"
        if fixed_temperature != 0:                                                     # fvit_head.py:27-31
            self.detect_temperature = fixed_temperature
        else:
            self.detect_temperature = nn.Parameter(torch.tensor(float(learned_temperature)))
        self.vlm_temperature, self.alpha, self.beta, self.learn_bg = float(vlm_temperature), float(alpha), float(beta), bool(learn_bg)
        self.featmap_stride = featmap_stride
        names, seen = _names(all_classes), _names(seen_classes)
        if seen is not None and names is None:
            raise ValueError("seen_classes needs all_classes")
        self.all_classes = None if names is None else names + ["background"]
        self.seen_classes = None if seen is None else seen + ["background"]
        embed = _load_embed(class_embed, self.all_classes)
        C = embed.shape[0]
        base = torch.ones(C, dtype=torch.bool)
        if self.seen_classes is not None:                                              # :40-44
            base = torch.zeros(C, dtype=torch.bool)
            base[[self.all_classes.index(s) for s in self.seen_classes]] = True
        self.base_idx, self.novel_idx = base, ~base
        all_embed = F.normalize(embed.permute(1, 0).contiguous(), p=2, dim=0)          # :48-49  [E, C]
        self.register_buffer("all_embeddings", all_embed)
        if learn_bg:
            self.bg_embedding = nn.Parameter(all_embed[:, -1:].clone())                # :52-53
        if ops is None and torch.cuda.is_available():
            from .hip import HipOps
            ops = HipOps()
        self.ops = ops
        has = bool(getattr(ops, "BOX_SCORES", False))
        if fused and not has:
            raise NotImplementedError(f"OpenVocabBoxScores(fused=True) needs the box-scores form of cs_roialign_fwd, which the kernel backend "
                                      f"{getattr(ops, 'name', type(ops).__name__)!r} does not provide (no BOX_SCORES)")
        self.fused = bool(FUSED_SCORES_DEFAULT and has) if fused is None else bool(fused)
        self._rows = self._rows_key = self._expo = self._expo_key = None

    # -------------------------------------------------------------------------------------------- state
    @property
    def all_embed(self):                                                               # :55-61
        if self.learn_bg:
            return torch.cat([self.all_embeddings[:, :-1], F.normalize(self.bg_embedding, dim=0)], dim=1)
        return self.all_embeddings

    def _embed_rows(self):
        """The [C, E] fp32 copy the kernel reads, rebuilt only when all_embeddings / bg_embedding change (or move)."""
        src = (self.all_embeddings,) + ((self.bg_embedding,) if self.learn_bg else ())
        key = tuple((t.data_ptr(), t._version, t.device, param_steps(t)) for t in src)     # a fused optimizer moves no version
        if key != self._rows_key:
            with torch.no_grad():
                self._rows, self._rows_key = self.all_embed.detach().float().t().contiguous(), key
        return self._rows

    def exponents(self, device=None):
        """w [C]: alpha on base classes, beta on novel ones (:116-119); rebuilt only when alpha / beta / the split change."""
        device = self.all_embeddings.device if device is None else device
        key = (self.alpha, self.beta, device, self.base_idx.data_ptr(), self.base_idx._version)
        if key != self._expo_key:
            w = torch.where(self.base_idx, torch.tensor(self.alpha), torch.tensor(self.beta)).float()
            self._expo, self._expo_key = w.to(device), key
        return self._expo

    # -------------------------------------------------------------------------------------------- the training branch
    def class_logits(self, x_cls):
        """fvit_head.py:108-109: plain torch, differentiable."""
        all_embed = self.all_embed.type_as(x_cls)
        return x_cls / x_cls.norm(dim=-1, keepdim=True) @ all_embed * self.detect_temperature

    # -------------------------------------------------------------------------------------------- the VLM branch
    def _token_map(self, vlm_feat):
        """[B, E, h, w] -> (feat [B, h, w, E] whose strides are (Ntok*E, w*E, E, 1), Ntok): the tower's token-major map in place when
        vlm_feat is the view forward_intermediates returns, one permute-copy for a map from elsewhere."""
        B, E, h, w = vlm_feat.shape
        nhwc = vlm_feat.permute(0, 2, 3, 1)
        ok = vlm_feat.dtype == torch.float32 and nhwc.stride(3) == 1 and nhwc.stride(2) == E and nhwc.stride(1) == w * E \
            and nhwc.stride(0) % E == 0 and nhwc.stride(0) >= h * w * E and nhwc.data_ptr() % 16 == 0
        if not ok:
            nhwc = nhwc.float().contiguous()
        return nhwc, nhwc.stride(0) // E

    def _normalised_rois(self, rois, h, w):
        r = rois.detach().float().clone()
        r[:, [1, 3]] /= float(w * self.featmap_stride)
        r[:, [2, 4]] /= float(h * self.featmap_stride)
        return r

    def _pool_fallback(self, vlm_feat, rois):
        B, E, h, w = vlm_feat.shape
        rois = rois.detach().float()
        extent = torch.stack([(rois[:, 3] - rois[:, 1]) / (2.0 * w * self.featmap_stride), (rois[:, 4] - rois[:, 2]) / (2.0 * h * self.featmap_stride)], 1)
        walk = (rois[:, 0] >= 0) & (rois[:, 0] < B) & (extent > 0).all(1) & (extent <= 1).all(1)        # the kernel's bounded-box rule
        ops = self._ops_for(vlm_feat)
        if getattr(ops, "BOX_SCORES", False):                                          # that backend pools the token-major map in place
            tokens, _ = self._token_map(vlm_feat.detach())
        else:
            tokens = vlm_feat.detach().float().permute(0, 2, 3, 1).reshape(B, h * w, E).contiguous()
        pooled = tokens.new_zeros(rois.shape[0], E)
        idx = torch.nonzero(walk)[:, 0]
        if idx.numel():
            part = tokens.new_empty(idx.numel(), E)
            ops.roialign_fwd(tokens, self._normalised_rois(rois[idx], h, w).contiguous(), part, h, w, 0)
            pooled[idx] = part
        return pooled

    def _ops_for(self, t):
        if self.ops is not None and (t.is_cuda or getattr(self.ops, "name", "") != "hip"):
            return self.ops
        raise RuntimeError("OpenVocabBoxScores: no kernel backend for a CPU tensor (pass ops=, e.g. the CPU reference backend)")

    def vlm_box_feats(self, vlm_feat, rois):
        """fvit_head.py:276: the pooled (not normalised) dense feature of every box, [K, E]."""
        if not self.fused:
            return self._pool_fallback(vlm_feat, rois)
        feat, _ = self._token_map(vlm_feat)
        B, h, w, E = feat.shape
        pooled = feat.new_empty(rois.shape[0], E)
        self.ops.roialign_fwd(feat, rois.detach().float().contiguous(), pooled, h, w, 0, box_scale=1.0 / self.featmap_stride)
        return pooled

    def forward(self, cls_score, vlm_feat, rois):
        assert not self.training                                                       # :67
        K, C = rois.shape[0], self.all_embeddings.shape[1]
        if self.fused:
            feat, _ = self._token_map(vlm_feat)
            B, h, w, E = feat.shape
            det = None if cls_score is None else cls_score.detach().float()
            if det is not None and det.stride(-1) != 1:
                det = det.contiguous()
            scores = feat.new_empty(K, C)
            self.ops.box_scores(feat, rois.detach().float().contiguous(), self._embed_rows(), scores, h, w, 0, 1.0 / self.featmap_stride,
                                self.vlm_temperature, det_logits=det, expo=None if det is None else self.exponents(feat.device))
            return scores
        with torch.no_grad():
            all_embed = self.all_embed.float()
            v = F.normalize(self._pool_fallback(vlm_feat, rois), dim=-1, p=2)          # :68
            vlm = (v @ all_embed * self.vlm_temperature).softmax(dim=-1)               # :113-114
            if cls_score is None:
                return vlm
            det = cls_score.detach().float().softmax(dim=-1)                           # :112
            w = self.exponents(det.device)
            return det ** (1 - w) * vlm ** w                                           # :116-119

    # -------------------------------------------------------------------------------------------- detections
    def get_bboxes(self, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None):
        """fvit_head.py:123-164 for one image, line for line, on det_post: rois [n, 5], cls_score [n, C + 1] (forward's scores; the
        background column is last), bbox_pred [n, 4] or None, img_shape (h, w[, c]) or None, scale_factor 4 numbers (or one).
        cfg None -> (bboxes, scores); cfg with score_thr, nms, max_per_img -> (det_bboxes [m, 5], det_labels [m]).  The batched,
        fixed-shape, read-back-free form of the same is det_post.detections."""
        from . import det_post
        if self.training:                                                              # :136-140 (no custom_cls_channels loss here)
            scores = F.softmax(cls_score, dim=-1) if cls_score is not None else None
        else:
            scores = cls_score
        if bbox_pred is not None:                                                      # :143-146
            bboxes = det_post.delta2bbox(rois[..., 1:], bbox_pred, self.target_means, self.target_stds, max_shape=img_shape)
        else:
            bboxes = rois[:, 1:].clone()                                               # :148-151: the reference's clamp_ acts on a copy
        if rescale and bboxes.size(0) > 0:                                             # :153-156
            sf = bboxes.new_tensor(scale_factor)
            bboxes = (bboxes.view(bboxes.size(0), -1, 4) / sf).view(bboxes.size()[0], -1)
        if cfg is None:                                                                # :158-164
            return bboxes, scores
        get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        return det_post.multiclass_nms(bboxes, scores, get("score_thr"), get("nms"), get("max_per_img"))


try:                                                      # optional: the reference registers its heads with mmdet (fvit_head.py:13)
    from mmdet.models.builder import HEADS
    HEADS.register_module(name="OpenVocabBoxScores")(OpenVocabBoxScores)
except ImportError:
    pass
