"""TEST INFRASTRUCTURE -- the F-ViT detector's kernel-backed modules chained through one training step and one inference pass
(DESIGN.md §3.26).  Not a product module: `FViT` / `FViTRoIHead` are not built in clipself_amd; this file composes the modules that exist
in the order of the reference's F-ViT/models/fvit.py (forward_train, simple_test) and F-ViT/models/fvit_head.py (_bbox_forward, the mask
forward, simple_test_bboxes), as read -- mmdet is cited, not run.

  Assembly(fused=True, ops=<backend>)   the kernel route: every layer on `ops`, every functional module on its kernels where the tensors
                                        are CUDA tensors (on the CPU the functional modules have no kernel form and take their torch route)
  Assembly(fused=False)                 the torch route throughout; .double() makes it the float64 reference of `check_scalars`
  train_step(asm, batch, keys)          FPN -> RPNHead -> anchors -> rpn_targets -> rpn_loss -> rpn_proposals (detached) -> rcnn_targets ->
                                        SingleRoIExtractor(7) -> ConvFCBBoxHead -> class_logits -> bbox_head_loss -> SingleRoIExtractor(14)
                                        on the positives -> FCNMaskHead -> mask_target -> mask_loss -> sum -> backward; returns a Record of
                                        every seam tensor and, after the backward, its gradient
  infer(asm, batch)                     eval(): rpn_proposals -> box head -> det_post.detections -> mask head -> paste_masks

The leaves are the four maps a neck would hand to the FPN (backbone -> neck has tests of its own).  In `infer` the class scores are the
softmax of the training branch's logits: the VLM blend needs the backbone's dense map, which is not part of the chain.

The checks (each raises AssertionError and prints its figures):
  check_forward   (a) every stage's recorded output against that stage's reference evaluated on the PRODUCER's recorded output
  check_replay    (b) every seam gradient against the stand-alone replay of its consumers, bit for bit
  check_scalars   (c) every loss term against the float64 torch route that is handed the kernel route's discrete decisions
  same_records    (d) two records bit for bit (live against fresh assembly)
  check_ragged    (e) finite losses and gradients, the image without ground truth, K = 0 in the mask branch
`flaw=` plants one seam error (FLAWS); tests/test_det_chain_cpu.py asserts which check rejects it.
"""
import contextlib
import itertools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import _assign_ref
import _loss_ref
import _mask_ref
import _nms_ref
import _proposal_ref
import _roi_extract_ref
from _fpn_ref import TwinFPN, rel_l2
from _thin_ref import PARITY_REL_L2, REFERENCE_MASK_HEAD, REFERENCE_RPN_HEAD, TwinMaskHead, TwinRPNHead

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
C, IMG, B, SIDES, NUM_CLASSES, EMBED, MASK = 64, 128, 3, (32, 16, 8, 4), 5, 128, 28
FLAWS = ("levels_swapped", "rpn_consumer_detached", "fc_flatten_nchw", "proposals_xywh", "stale_pack", "padding_rows_used")

# ------------------------------------------------------------------------------------------------ reference-style configs, small widths
NORM = dict(type="SyncBN", requires_grad=True)
NECK = dict(type="FPN", in_channels=[C] * 4, out_channels=C, norm_cfg=NORM, num_outs=5)
RPN_HEAD = dict(REFERENCE_RPN_HEAD, in_channels=C, feat_channels=C)
BBOX_ROI = dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0), out_channels=C,
                featmap_strides=[4, 8, 16, 32])
MASK_ROI = dict(BBOX_ROI, roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0))
BBOX_HEAD = dict(type="FViTBBoxHead", in_channels=C, fc_out_channels=EMBED, roi_feat_size=7, num_shared_fcs=2, num_classes=NUM_CLASSES,
                 reg_class_agnostic=True, norm_cfg=NORM,
                 bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[0.0, 0.0, 0.0, 0.0], target_stds=[0.1, 0.1, 0.2, 0.2]),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0))
MASK_HEAD = dict(REFERENCE_MASK_HEAD, num_convs=2, in_channels=C, conv_out_channels=C, num_classes=NUM_CLASSES)
TRAIN_CFG = dict(
    rpn=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1),
             sampler=dict(type="RandomSampler", num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False)),
    rpn_proposal=dict(nms_pre=256, max_per_img=128, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0),
    rcnn=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=True, ignore_iof_thr=-1),
              sampler=dict(type="RandomSampler", num=64, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), mask_size=MASK))
TEST_CFG = dict(rpn=dict(nms_pre=256, max_per_img=128, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0),
                rcnn=dict(score_thr=0.0001, nms=dict(type="nms", iou_threshold=0.5), max_per_img=16, mask_thr_binary=0.5))
RPN_STDS, RCNN_STDS = (1.0, 1.0, 1.0, 1.0), (0.1, 0.1, 0.2, 0.2)


class NoKernels:
    """A backend without any kernel flag: handed to a functional module as `ops`, it selects that module's torch route on any device."""
    name = "none"


def _without(cfg, *keys):
    return {k: v for k, v in cfg.items() if k not in keys}


def _bf(t):
    return t.to(BF).to(F32)


# ------------------------------------------------------------------------------------------------ the assembly
class Assembly(nn.Module):
    """One set of modules under the reference's names.  fused=True: the kernel route on `ops`; fused=False: torch.  `seed` fixes the
    initial values: convolution and FC weights that bf16 holds (the convention of the module tests' random cases), batch-norm affines off
    the identity, head weights large enough that proposals and classes differ between anchors."""

    def __init__(self, fused, ops=None, seed=0):
        super().__init__()
        from clipself_amd.bbox_head import ConvFCBBoxHead
        from clipself_amd.det_targets import AnchorGenerator, MaxIoUAssigner, RandomSampler
        from clipself_amd.fpn import FPN
        from clipself_amd.mask_head import FCNMaskHead
        from clipself_amd.ov_head import OpenVocabBoxScores
        from clipself_amd.roi_extractor import SingleRoIExtractor
        from clipself_amd.rpn_head import RPNHead
        self.fused = bool(fused)
        lay = dict(ops=ops if fused else None, fused=bool(fused))
        fn_ops = None if fused else NoKernels()                          # the functional modules: their own HipOps, or no kernels at all
        self.fn_ops = fn_ops
        g = torch.Generator().manual_seed(1000 + seed)
        self.neck = FPN(**_without(NECK, "type"), **lay)
        self.rpn_head = RPNHead(**RPN_HEAD, **lay)
        self.bbox_roi_extractor = SingleRoIExtractor(**_without(BBOX_ROI, "type"), ops=fn_ops)
        self.bbox_head = ConvFCBBoxHead(**BBOX_HEAD, fused_reg=bool(fused), **lay)
        embed = torch.randn(NUM_CLASSES + 1, EMBED, generator=g)
        self.scores = OpenVocabBoxScores(embed, ops=ops if ops is not None else NoKernels(), fused=False)
        self.mask_roi_extractor = SingleRoIExtractor(**_without(MASK_ROI, "type"), ops=fn_ops)
        self.mask_head = FCNMaskHead(**MASK_HEAD, **lay)
        ag = _without(RPN_HEAD["anchor_generator"], "type")
        self.__dict__["anchor_generator"] = AnchorGenerator(**ag)
        t = TRAIN_CFG
        self.__dict__["rpn_assigner"], self.__dict__["rpn_sampler"] = MaxIoUAssigner(**t["rpn"]["assigner"]), RandomSampler(**t["rpn"]["sampler"])
        self.__dict__["rcnn_assigner"], self.__dict__["rcnn_sampler"] = MaxIoUAssigner(**t["rcnn"]["assigner"]), RandomSampler(**t["rcnn"]["sampler"])
        with torch.no_grad():
            for name, m in self.named_modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                    scale = {"rpn_head.rpn_cls": 0.2, "rpn_head.rpn_reg": 0.05, "bbox_head.fc_reg": 0.02}.get(name)
                    if scale is not None:
                        m.weight.copy_(scale * torch.randn(m.weight.shape, generator=g))
                    else:
                        fan = m.weight[0].numel()
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                    m.weight.copy_(_bf(m.weight))
                    if m.bias is not None:
                        m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))

    def fn(self, fused_kw=True):
        """ops / fused for a functional module: fused=True on CUDA tensors of the kernel route, the torch route otherwise."""
        dev = next(self.parameters()).device
        if not fused_kw:
            return dict(ops=self.fn_ops)
        return dict(ops=self.fn_ops, fused=True if (self.fused and dev.type == "cuda") else False if not self.fused else None)


def fresh_like(asm, ops=None, state=None):
    """A new assembly (new objects, no caches, no workspaces) of asm's route on asm's device and dtype with `state` (default: asm's own)."""
    new = Assembly(asm.fused, ops=ops)
    p = next(asm.parameters())
    new = new.to(device=p.device, dtype=p.dtype)
    new.load_state_dict(asm.state_dict() if state is None else state, strict=True)
    return new.train(asm.training)


# ------------------------------------------------------------------------------------------------ the batch
def make_batch(seed=0, negatives_only=False, device="cpu"):
    """B = 3 images of 128 x 128: one with four boxes, one WITHOUT ground truth whose content fills
    40 x 56 pixels of the padded frame (so most of its proposals are clamped away and its list is short), one whose only box is 6 x 5 pixels.  negatives_only: no
    image has ground truth, so no stage has a positive.  The maps are bf16-representable fp32 values."""
    g = torch.Generator().manual_seed(2000 + seed)
    maps = [torch.randn(B, C, s, s, generator=g) for s in SIDES]
    for m in maps:                                                       # image 1 is spatially smooth: its best anchors cluster, NMS removes
        m[1] = F.interpolate(torch.randn(1, C, 2, 2, generator=g), size=m.shape[-2:], mode="bilinear", align_corners=True)[0]      # most of them
    maps = [_bf(m).to(device) for m in maps]
    boxes = [torch.tensor([[8., 8., 72., 60.], [40., 50., 120., 120.], [70., 10., 110., 50.], [20., 70., 60., 110.]]), torch.zeros(0, 4),
             torch.tensor([[60., 60., 66., 65.]])]
    labels = [torch.tensor([0, 3, 1, 4]), torch.zeros(0, dtype=torch.int64), torch.tensor([2])]
    if negatives_only:
        boxes, labels = [torch.zeros(0, 4)] * B, [torch.zeros(0, dtype=torch.int64)] * B
    yy, xx = torch.meshgrid(torch.arange(IMG, dtype=F32) + 0.5, torch.arange(IMG, dtype=F32) + 0.5, indexing="ij")
    masks = []
    for bx in boxes:                                                     # an ellipse inside each box
        ms = [(((xx - (b[0] + b[2]) / 2) / ((b[2] - b[0]) / 2)) ** 2 + ((yy - (b[1] + b[3]) / 2) / ((b[3] - b[1]) / 2)) ** 2 <= 1).to(torch.uint8) for b in bx]
        masks.append(torch.stack(ms) if ms else torch.zeros(0, IMG, IMG, dtype=torch.uint8))
    return dict(maps=maps, gt_bboxes=[b.to(device) for b in boxes], gt_labels=[l.to(device) for l in labels],
                gt_masks=[m.to(device) for m in masks], img_shapes=[(IMG, IMG), (40, 56), (IMG, IMG)])


def make_keys(seed=0, device="cpu"):
    """The samplers' random keys, drawn once on the CPU so that every route and device shares them."""
    from clipself_amd.det_targets import random_keys
    g = torch.Generator().manual_seed(3000 + seed)
    n_anchors = 3 * sum((IMG // s) ** 2 for s in (4, 8, 16, 32, 64))
    n_rcnn = TRAIN_CFG["rpn_proposal"]["max_per_img"] + 4                 # max_per_img + the largest ground-truth prefix
    return dict(rpn=random_keys((B, n_anchors), "cpu", g).to(device), rcnn=random_keys((B, n_rcnn), "cpu", g).to(device))


def rcnn_keys(keys, batch):
    """The box sampler's keys cut to [B, Nmax], Nmax = max_per_img + the batch's longest ground-truth prefix: the kernel route takes exactly
    that shape."""
    nmax = TRAIN_CFG["rpn_proposal"]["max_per_img"] + max(int(g.shape[0]) for g in batch["gt_bboxes"])
    return keys["rcnn"][:, :nmax].contiguous()


# ------------------------------------------------------------------------------------------------ the record
class Record(dict):
    """name -> tensor of one step; `grads` name -> gradient after the backward; `param_grads`; `state` the assembly's state dict before the
    step; `gt` the ground-truth boxes; `fns` name -> the autograd node that made the tensor."""

    def __init__(self):
        super().__init__()
        self.grads, self.param_grads, self.state, self.gt, self.fns, self._live = {}, {}, None, None, {}, {}

    def keep(self, name, t):
        self[name] = t.detach()
        self.fns[name] = type(t.grad_fn).__name__                        # which autograd node made it: the route that really ran
        if t.requires_grad:
            t.retain_grad()
            self._live[name] = t
        return t

    def collect(self, asm):
        self.grads = {k: (None if t.grad is None else t.grad.detach().clone()) for k, t in self._live.items()}
        self.param_grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in asm.named_parameters()}
        self._live = {}


def _xyxy_to_xywh(p):
    q = p.clone()
    q[..., 2:4] = p[..., 2:4] - p[..., 0:2]
    return q


@contextlib.contextmanager
def stale_packs():
    """The planted error `stale_pack`: det_layer.packed never rebuilds an entry it has, in every module that imported it."""
    import clipself_amd
    import importlib
    def stale(mod, build, key=None, slot="_wcache"):
        c = mod.__dict__.get(slot)
        if c is None:
            with torch.no_grad():
                c = mod.__dict__[slot] = (key, tuple(build()))
        return c[1]
    names = ("det_layer", "conv", "linear", "neck", "norm_act", "mask_head", "fpn")
    mods = [importlib.import_module(f"clipself_amd.{n}") for n in names]
    saved = [(m, m.packed) for m in mods if hasattr(m, "packed")]
    for m, _ in saved:
        m.packed = stale
    try:
        yield
    finally:
        for m, f in saved:
            m.packed = f


def anchors_of(asm, sizes, device):
    ag = asm.anchor_generator
    anchors = torch.cat(ag.grid_priors(sizes, device=device), dim=0)
    valid = torch.cat(ag.valid_flags(sizes, (IMG, IMG), device=device))
    return anchors, valid


def box_branch(asm, feats, rois, rec=None, flaw=None):
    """_bbox_forward: extractor -> shared FCs -> (class logits, box deltas)."""
    roi_feats = asm.bbox_roi_extractor(feats[:4], rois)
    if rec is not None:
        rec.keep("roi_feats", roi_feats)
    x = roi_feats
    if flaw == "fc_flatten_nchw":                                        # NCHW-ordered memory handed over as if it were channel-last rows
        K, Cc, P, _ = x.shape
        x = x.contiguous().view(K, P, P, Cc).permute(0, 3, 1, 2)
    trunk = x
    for i, fc in enumerate(asm.bbox_head.shared_fcs):
        trunk = fc(trunk)
        if rec is not None and i + 1 < len(asm.bbox_head.shared_fcs):
            rec[f"fc{i}"] = trunk.detach()
    if rec is not None:
        rec.keep("trunk", trunk)
    bbox_pred = asm.bbox_head.fc_reg(trunk)
    cls_score = asm.scores.class_logits(trunk)
    return cls_score, bbox_pred


def train_step(asm, batch, keys, flaw=None, poison=False, decisions=None):
    """One training step (module docstring).  decisions: a Record of another route whose discrete results (targets, proposals, rois,
    sampled sets, mask targets) are taken as constants instead of being computed -- the float64 route of `check_scalars`."""
    from clipself_amd import det_losses, det_masks, det_proposals, det_targets
    assert flaw is None or flaw in FLAWS, flaw
    asm.train()
    asm.zero_grad(set_to_none=True)
    rec = Record()
    rec.state = {k: v.detach().clone() for k, v in asm.state_dict().items()}
    rec.gt = [g.detach().cpu().float() for g in batch["gt_bboxes"]]
    p0 = next(asm.parameters())
    dev, dt = p0.device, p0.dtype
    leaves = [rec.keep(f"leaf{i}", m.detach().to(device=dev, dtype=dt).clone().requires_grad_(True)) for i, m in enumerate(batch["maps"])]
    feats = [rec.keep(f"fpn{i}", f) for i, f in enumerate(asm.neck(leaves))]
    rpn_in = [f.detach() for f in feats] if flaw == "rpn_consumer_detached" else feats
    cls_scores, bbox_preds = asm.rpn_head(rpn_in)
    for i, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        rec.keep(f"rpn_cls{i}", c), rec.keep(f"rpn_reg{i}", r)
    sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
    anchors, valid = anchors_of(asm, sizes, dev)
    rec["anchors"] = anchors
    take = (lambda *names: [decisions[n].to(dev) for n in names]) if decisions is not None else None
    # ---- RPN targets, loss and proposals
    if decisions is None:
        t = det_targets.rpn_targets(anchors, valid, batch["gt_bboxes"], asm.rpn_assigner, asm.rpn_sampler, (0., 0., 0., 0.), RPN_STDS,
                                    keys=keys["rpn"], **asm.fn(False))
    else:
        t = take("rpn_labels", "rpn_lw", "rpn_bt", "rpn_bw", "rpn_avg")
    for n, v in zip(("rpn_labels", "rpn_lw", "rpn_bt", "rpn_bw", "rpn_avg"), t):
        rec[n] = v.detach()
    if dt == F64:
        rl = rpn_loss64(cls_scores, bbox_preds, *t)
    else:
        rl = det_losses.rpn_loss(cls_scores, bbox_preds, *t, loss_cls=RPN_HEAD["loss_cls"], loss_bbox=RPN_HEAD["loss_bbox"], **asm.fn())
    losses = dict(loss_rpn_cls=sum(rl["loss_rpn_cls"]), loss_rpn_bbox=sum(rl["loss_rpn_bbox"]))
    rec["loss_rpn_cls_levels"], rec["loss_rpn_bbox_levels"] = torch.stack(rl["loss_rpn_cls"]).detach(), torch.stack(rl["loss_rpn_bbox"]).detach()
    if decisions is None:
        props, counts, plev, pinds = det_proposals.rpn_proposals([c.detach() for c in cls_scores], [r.detach() for r in bbox_preds], anchors,
                                                                  batch["img_shapes"], TRAIN_CFG["rpn_proposal"], stds=RPN_STDS,
                                                                  return_inds=True, **asm.fn())
        rec["proposals"], rec["counts"], rec["proposal_levels"], rec["proposal_inds"] = props, counts, plev, pinds
        # ---- R-CNN targets
        boxes = props[..., :4]
        if flaw == "proposals_xywh":
            boxes = _xyxy_to_xywh(boxes)
        if poison:                                                       # the rows past the count must never be read
            boxes = boxes.clone()
            boxes[torch.arange(boxes.shape[1], device=dev)[None, :] >= counts[:, None].to(dev)] = float("nan")
        r = det_targets.rcnn_targets(boxes, batch["gt_bboxes"], batch["gt_labels"], asm.rcnn_assigner, asm.rcnn_sampler, (0., 0., 0., 0.),
                                     RCNN_STDS, NUM_CLASSES, keys=rcnn_keys(keys, batch), return_gt_inds=True,
                                     proposal_counts=None if flaw == "padding_rows_used" else counts, **asm.fn(False))
    else:
        r = take("rois", "labels", "lw", "bt", "bw", "pos_gt_inds")
    for n, v in zip(("rois", "labels", "lw", "bt", "bw", "pos_gt_inds"), r):
        rec[n] = v.detach()
    rois, labels, lw, bt, bw, pos_gt = r
    # ---- box branch
    ext_feats = list(feats)
    if flaw == "levels_swapped":                                         # levels 1 and 2 exchanged through a resize
        ext_feats[1], ext_feats[2] = (F.interpolate(feats[2], size=feats[1].shape[-2:], mode="nearest"),
                                      F.interpolate(feats[1], size=feats[2].shape[-2:], mode="nearest"))
    if dt == F64:
        cls_score, bbox_pred = box_branch64(asm, ext_feats, rois, rec)
        bl = head_loss64(cls_score, bbox_pred, labels, lw, bt, bw)
    else:
        cls_score, bbox_pred = box_branch(asm, ext_feats, rois, rec, flaw)
        bl = det_losses.bbox_head_loss(cls_score, bbox_pred, labels, lw, bt, bw, loss_cls=BBOX_HEAD["loss_cls"], loss_bbox=BBOX_HEAD["loss_bbox"],
                                       num_classes=NUM_CLASSES, **asm.fn())
    rec.keep("cls_score", cls_score), rec.keep("bbox_pred", bbox_pred)
    losses["loss_cls"], losses["loss_bbox"] = bl["loss_cls"], bl["loss_bbox"]
    # ---- mask branch on the positives
    idx = torch.nonzero(pos_gt >= 0)[:, 0] if decisions is None else decisions["pos_idx"].to(dev)
    rec["pos_idx"] = idx
    pos_rois = rois[idx]
    if dt == F64:
        mask_feats = rec.keep("mask_feats", roi_extract64(ext_feats[:4], pos_rois, 14))
    else:
        mask_feats = rec.keep("mask_feats", asm.mask_roi_extractor(ext_feats[:4], pos_rois))
    if idx.numel():
        mask_pred = asm.mask_head(mask_feats)
    else:                                                                # mmdet's FCNMaskHead gives [0, 1, 28, 28]: no row, no layer to run
        mask_pred = mask_feats.new_zeros(0, 1, MASK, MASK) + mask_feats.sum() * 0
    rec.keep("mask_pred", mask_pred)
    if decisions is None:
        mt = det_masks.mask_target(pos_rois, pos_gt[idx], batch["gt_masks"], MASK, **asm.fn())
    else:
        mt = decisions["mask_targets"].to(dev)
    rec["mask_targets"] = mt
    ones = torch.ones(idx.numel(), dtype=F32, device=dev)
    if dt == F64:
        losses["loss_mask"] = mask_loss64(mask_pred, mt)
    else:
        losses["loss_mask"] = det_masks.mask_loss(mask_pred, mt, None, ones, True, MASK_HEAD["loss_mask"], **asm.fn())["loss_mask"]
    total = sum(losses.values())
    for k, v in losses.items():
        rec[k] = v.detach()
    rec["total"] = total.detach()
    total.backward()
    rec.collect(asm)
    return rec


def infer(asm, batch):
    """simple_test: proposals, box head, detections, mask head on the detections, pasted masks.  -> Record."""
    from clipself_amd import det_masks, det_post, det_proposals
    asm.eval()
    rec = Record()
    p0 = next(asm.parameters())
    dev, dt = p0.device, p0.dtype
    with torch.no_grad():
        feats = asm.neck([m.to(device=dev, dtype=dt) for m in batch["maps"]])
        cls_scores, bbox_preds = asm.rpn_head(feats)
        sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
        anchors, _ = anchors_of(asm, sizes, dev)
        props, counts = det_proposals.rpn_proposals(cls_scores, bbox_preds, anchors, batch["img_shapes"], TEST_CFG["rpn"], stds=RPN_STDS, **asm.fn())
        n = [int(v) for v in counts.tolist()]
        from clipself_amd.roi_extractor import bbox2roi
        rois = bbox2roi([props[b, :n[b], :4] for b in range(B)])
        cls_score, bbox_pred = box_branch(asm, feats, rois)
        scores = cls_score.float().softmax(-1)
        starts = [0] + list(itertools.accumulate(n))
        t = TEST_CFG["rcnn"]
        dets, labels, inds, dcounts = det_post.detections(rois, scores, bbox_pred, batch["img_shapes"], None, t["score_thr"], t["nms"]["iou_threshold"],
                                                          t["max_per_img"], stds=RCNN_STDS, starts=starts, Kmax=max(max(n), 1), **asm.fn(False))
        m = [int(v) for v in dcounts.tolist()]
        det_rois = bbox2roi([dets[b, :m[b], :4] for b in range(B)])
        mask_feats = asm.mask_roi_extractor(feats[:4], det_rois)
        mask_pred = asm.mask_head(mask_feats) if det_rois.shape[0] else mask_feats.new_zeros(0, 1, MASK, MASK)
        pasted = det_masks.paste_masks(mask_pred, det_rois[:, 1:], None, (IMG, IMG), None, t["mask_thr_binary"], True, **asm.fn())
    for k, v in dict(proposals=props, counts=counts, rois=rois, cls_score=cls_score, bbox_pred=bbox_pred, dets=dets, det_labels=labels,
                     det_counts=dcounts, mask_pred=mask_pred, pasted=pasted, **{f"fpn{i}": f for i, f in enumerate(feats)}).items():
        rec[k] = v.detach()
    return rec


# ------------------------------------------------------------------------------------------------ the float64 pieces of the torch route
def rpn_loss64(cls_scores, bbox_preds, labels, lw, bt, bw, avg):
    """RPNHead.loss in float64 torch: sigmoid BCE and L1, weighted, over avg + eps (mmdet's weight_reduce_loss)."""
    Bn, A = cls_scores[0].shape[:2]
    den = avg.reshape(()).double() + _loss_ref.EPS
    out, off = dict(loss_rpn_cls=[], loss_rpn_bbox=[]), 0
    for x, r in zip(cls_scores, bbox_preds):
        h, w = x.shape[-2:]
        n = h * w * A
        lab = labels[:, off:off + n].reshape(Bn, h, w, A).permute(0, 3, 1, 2)
        wts = lw[:, off:off + n].reshape(Bn, h, w, A).permute(0, 3, 1, 2).double()
        t = bt[:, off:off + n].reshape(Bn, h, w, 4 * A).permute(0, 3, 1, 2).double()
        tw = bw[:, off:off + n].reshape(Bn, h, w, 4 * A).permute(0, 3, 1, 2).double()
        off += n
        bce = F.binary_cross_entropy_with_logits(x, (lab == 0).double(), reduction="none")
        out["loss_rpn_cls"].append((bce * wts).sum() / den)
        out["loss_rpn_bbox"].append(((r - t).abs() * tw).sum() / den)
    return out


def head_loss64(cls_score, bbox_pred, labels, lw, bt, bw):
    avg = (lw > 0).sum().clamp(min=1).double()
    ok = (labels >= 0) & (labels <= NUM_CLASSES)
    ce = F.cross_entropy(cls_score, labels.long().clamp(0, NUM_CLASSES), reduction="none")
    loss_cls = (ce * lw.double() * ok.double()).sum() / (avg + _loss_ref.EPS)
    pos = ((labels >= 0) & (labels < NUM_CLASSES)).double()[:, None]
    loss_bbox = ((bbox_pred - bt.double()).abs() * bw.double() * pos).sum() / (float(cls_score.shape[0]) + _loss_ref.EPS)
    return dict(loss_cls=loss_cls, loss_bbox=loss_bbox)


def mask_loss64(mask_pred, targets):
    if mask_pred.shape[0] == 0:
        return mask_pred.sum()
    return F.binary_cross_entropy_with_logits(mask_pred[:, 0], (targets != 0).double(), reduction="mean")


def roi_extract64(feats, rois, P):
    """The extractor's contract with float64 sums (tests/_roi_extract_ref.forward_vec): forward only, which is all `check_scalars` needs."""
    maps = [f.detach().double().cpu().permute(0, 2, 3, 1).numpy() for f in feats]
    out = _roi_extract_ref.forward_vec(maps, rois.detach().float().cpu().numpy(), [4, 8, 16, 32], P)["out"]
    zero = sum(f.sum() * 0 for f in feats)
    return torch.from_numpy(out).permute(0, 3, 1, 2).to(feats[0].device) + zero


def box_branch64(asm, feats, rois, rec):
    x = rec.keep("roi_feats", roi_extract64(feats[:4], rois, 7))
    trunk = x
    for fc in asm.bbox_head.shared_fcs:
        trunk = fc(trunk)
    rec.keep("trunk", trunk)
    return asm.scores.class_logits(trunk), asm.bbox_head.fc_reg(trunk)


# ------------------------------------------------------------------------------------------------ small helpers of the checks
def bits_equal(a, b):
    """Equal bits; the sign of a zero is not compared (tests/_fpn_ref.same_bits explains why)."""
    if a is None or b is None:
        return a is None and b is None
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype.is_floating_point:
        it = {BF: torch.int16, F32: torch.int32, F64: torch.int64}[a.dtype]
        nan = torch.isnan(a) & torch.isnan(b)
        return bool((((a + 0.0).view(it) == (b + 0.0).view(it)) | nan).all())
    return bool(torch.equal(a, b))


def same_records(a, b, what):
    """(d): every tensor, gradient and parameter gradient of two records bit for bit."""
    bad = []
    for name, da, db in (("tensor", a, b), ("gradient", a.grads, b.grads), ("parameter gradient", a.param_grads, b.param_grads)):
        assert sorted(da) == sorted(db), (what, name, sorted(set(da) ^ set(db)))
        bad += [f"{name} {k}" for k in da if not bits_equal(da[k], db[k])]
    assert not bad, f"{what}: {len(bad)} differ in bits: {bad[:8]}"


def _np(t):
    return t.detach().cpu().numpy()


def _figure(tag, what, value):
    print(f"DET CHAIN [{tag}] {what}: {value}")


# ------------------------------------------------------------------------------------------------ (a) forward seams
def check_forward(rec, asm, batch, keys, tag="CPU backend"):
    """Every stage's recorded output against its reference evaluated on the producer's recorded output (module docstring)."""
    from clipself_amd import det_proposals
    cpu = lambda t: t.detach().cpu()
    L = 5
    # ---- FPN and RPN head: the float64 twins, relative L2 under the modules' own threshold
    twin = TwinFPN(**_without(NECK, "type")).double().train()
    twin.load_state_dict({k[len("neck."):]: cpu(v).double() if v.dtype.is_floating_point else cpu(v) for k, v in rec.state.items() if k.startswith("neck.")})
    outs = twin([cpu(rec[f"leaf{i}"]).double() for i in range(4)])
    for i in range(L):
        r = rel_l2(rec[f"fpn{i}"], outs[i])
        _figure(tag, f"(a) FPN output {i} rel-L2", f"{r:.4e}")
        assert r <= PARITY_REL_L2, f"(a) FPN output {i}: {r:.3e}"
    head = TwinRPNHead(**RPN_HEAD).double().train()
    sd = {k[len("rpn_head."):]: cpu(v).double() if v.dtype.is_floating_point else cpu(v) for k, v in rec.state.items() if k.startswith("rpn_head.")}
    for i in range(L):
        head.load_state_dict(sd)
        c, r = head([cpu(rec[f"fpn{i}"]).double()])
        for name, got, want in ((f"rpn_cls{i}", rec[f"rpn_cls{i}"], c[0]), (f"rpn_reg{i}", rec[f"rpn_reg{i}"], r[0])):
            v = rel_l2(got, want)
            _figure(tag, f"(a) RPN head {name} rel-L2", f"{v:.4e}")
            assert v <= PARITY_REL_L2, f"(a) {name}: {v:.3e}"
    # ---- RPN targets: the np.float32 restatement tests/_assign_ref (assign, sample, targets) on the restated anchors, the ground truth
    # and the keys; integers, weights and dx, dy bit for bit, dw, dh inside its derived bound against T64
    sizes = [tuple(rec[f"rpn_cls{i}"].shape[-2:]) for i in range(L)]
    anchors, valid = anchors_of(asm, sizes, "cpu")
    anc = _assign_ref.anchors_np(sizes)
    assert bits_equal(rec["anchors"], torch.from_numpy(anc)) and bits_equal(rec["anchors"], anchors), "(a) anchors differ from the restatement"
    gts = [cpu(g) for g in batch["gt_bboxes"]]
    gt_np = np.concatenate([_np(g).reshape(-1, 4) for g in gts]).astype(np.float32)
    gt_starts = [0] + list(itertools.accumulate(len(g) for g in gts))
    sm = TRAIN_CFG["rpn"]["sampler"]
    c = _assign_ref._case(anc, gt_np, gt_starts, _assign_ref.RPN, valid=_np(valid).astype(np.uint8), B=B, Nmax=len(anc), num=sm["num"],
                          frac=sm["pos_fraction"], ub=sm["neg_pos_ub"], stds=RPN_STDS, bg_label=1, keys=_np(keys["rpn"]).view(np.uint32))
    gi, _ = _assign_ref.assign(c)
    flags, _, cnt = _assign_ref.sample(gi, c["keys"], None, len(anc), gt_starts, len(gt_np), c["Gmax"], c["num"], c["expected_pos"], c["ub"])
    want = _assign_ref.targets(c, gi, flags)
    _same_targets("(a) rpn_targets", dict(labels=rec["rpn_labels"], label_weights=rec["rpn_lw"], bbox_targets=rec["rpn_bt"], bbox_weights=rec["rpn_bw"]),
                  want, tag)
    assert int(rec["rpn_avg"]) == max(int(cnt.sum()), 1), "(a) rpn_targets: num_total_samples"
    # ---- RPN loss: the closed form in float64 with its bounds, values and gradients with respect to the predictions
    case = dict(B=B, A=3, avg=float(rec["rpn_avg"]), levels=sizes, labels=_np(rec["rpn_labels"]), lw=_np(rec["rpn_lw"]), bt=_np(rec["rpn_bt"]),
                bw=_np(rec["rpn_bw"]), cls=[_np(rec[f"rpn_cls{i}"]) for i in range(L)], reg=[_np(rec[f"rpn_reg{i}"]) for i in range(L)])
    ref = _loss_ref.rpn_ref(case)
    got = np.stack([_np(rec["loss_rpn_cls_levels"]), _np(rec["loss_rpn_bbox_levels"])], 1)
    ok, frac = _loss_ref.inside(got, ref["losses"], ref["losses_bound"])
    _figure(tag, "(a) rpn_loss values, worst fraction of the bound", f"{frac:.3f}")
    assert ok, f"(a) rpn_loss: {frac:.3f} of the bound"
    for i in range(L):
        for name, key in ((f"rpn_cls{i}", "dcls"), (f"rpn_reg{i}", "dreg")):
            ok, frac = _loss_ref.inside(_np(rec.grads[name]), ref[key][i], ref[key + "_bound"][i])
            assert ok, f"(a) rpn_loss: gradient at {name} at {frac:.3f} of the bound"
    _figure(tag, "(a) rpn_loss gradients at the predictions", "inside the closed form's bounds")
    # ---- proposals: selection against the restatement, then NMS against the torch route on the selected rows
    cfg = TRAIN_CFG["rpn_proposal"]
    pc = dict(cls=case["cls"], reg=case["reg"], anchors=_np(anchors), nms_pre=cfg["nms_pre"], max_shape=np.array([list(s)[:2] for s in batch["img_shapes"]], np.float32),
              means=(0., 0., 0., 0.), stds=RPN_STDS, wh_ratio_clip=16 / 1000, min_bbox_size=0.0)
    sel_want = _proposal_ref.select(pc)
    dev = rec["rpn_cls0"].device
    sel = det_proposals.select([rec[f"rpn_cls{i}"] for i in range(L)], [rec[f"rpn_reg{i}"] for i in range(L)], rec["anchors"], batch["img_shapes"],
                               cfg["nms_pre"], stds=RPN_STDS, **asm.fn())
    bad = _proposal_ref.check_select(sel_want, [_np(t) for t in sel], f"DET CHAIN [{tag}] (a) select")
    assert not bad, bad
    # the NMS and the cut: tests/_nms_ref.multiclass (the contract's group form) on the rows that were selected.  An image whose closest
    # pair of boxes is further than 1e-5 from the IoU threshold in float64 (the margin the NMS tests ask of off-lattice boxes) is decided:
    # its float32 restatement must be met.  In an image inside that margin a pair's fp32 comparison may fall either way, and the float32
    # or the float64 restatement must be met.
    Bn, Ktot = sel[1].shape
    sb, ss, sg, si = (_np(t) for t in sel)
    starts = (np.arange(Bn + 1) * Ktot).astype(np.int32)
    args = (sb.reshape(-1, 4), ss.reshape(-1, 1), starts, Ktot, -1.0, cfg["nms"]["iou_threshold"], cfg["max_per_img"], sg.reshape(-1), L)
    w32, w64 = _nms_ref.multiclass(*args), _nms_ref.multiclass(*args, dtype=np.float64)
    margins = []
    for bi in range(Bn):
        live = sg[bi] >= 0
        margins.append(_nms_ref.min_iou_margin(sb[bi][live], cfg["nms"]["iou_threshold"]))
        got = (_np(rec["proposals"][bi]), int(rec["counts"][bi]), _np(rec["proposal_inds"][bi]).astype(np.int64))
        def same(w):
            rows = w[2][bi]
            picked = np.where(rows >= 0, si.reshape(-1)[np.maximum(rows, 0)], -1).astype(np.int64)
            return got[1] == int(w[3][bi]) and np.array_equal(got[2], picked) and got[0].tobytes() == w[0][bi].tobytes()
        ok = same(w32) if margins[-1] > 1e-5 else (same(w32) or same(w64))
        assert ok, f"(a) proposals of image {bi}: counts, kept anchors or bits differ from tests/_nms_ref on the selected rows (margin {margins[-1]:.2e})"
    _figure(tag, "(a) proposals: counts", rec["counts"].tolist())
    _figure(tag, "(a) proposals: smallest |IoU - threshold| per image", [f"{m:.2e}" for m in margins])
    # ---- R-CNN targets: tests/_assign_ref on the PRODUCER's proposals and counts (ground truth in front, the rows past the count invalid)
    props, pcounts = _np(rec["proposals"])[..., :4].astype(np.float32), [int(v) for v in rec["counts"].tolist()]
    rows, valid_r, st = [], [], [0]
    for bi in range(B):
        g = gt_np[gt_starts[bi]:gt_starts[bi + 1]]
        rows += [g, props[bi]]
        valid_r += [np.ones(len(g), np.uint8), (np.arange(props.shape[1]) < pcounts[bi]).astype(np.uint8)]
        st.append(st[-1] + len(g) + props.shape[1])
    sm, ac = TRAIN_CFG["rcnn"]["sampler"], TRAIN_CFG["rcnn"]["assigner"]
    rule = dict(pos=ac["pos_iou_thr"], neg=ac["neg_iou_thr"], min_pos=ac["min_pos_iou"], mlq=ac["match_low_quality"], all=True, prefix=True)
    c = _assign_ref._case(np.concatenate(rows), gt_np, gt_starts, rule, starts=st, valid=np.concatenate(valid_r), B=B, num=sm["num"],
                          frac=sm["pos_fraction"], ub=sm["neg_pos_ub"], stds=RCNN_STDS, bg_label=NUM_CLASSES,
                          gt_labels=np.concatenate([_np(l).reshape(-1) for l in batch["gt_labels"]]).astype(np.int32),
                          keys=_np(rcnn_keys(keys, batch)).view(np.uint32))
    gi, _ = _assign_ref.assign(c)
    _, sel_r, _ = _assign_ref.sample(gi, c["keys"], st, len(c["boxes"]), gt_starts, len(gt_np), c["Gmax"], c["num"], c["expected_pos"], c["ub"])
    want = _assign_ref.targets(c, gi, None, sel_r)
    n = B * sm["num"]
    assert bits_equal(rec["rois"], torch.from_numpy(want["rois"].reshape(n, 5))), \
        "(a) rcnn_targets: rois differ from the restatement's choice on the recorded proposals"
    _same_targets("(a) rcnn_targets", dict(labels=rec["labels"], label_weights=rec["lw"], bbox_targets=rec["bt"], bbox_weights=rec["bw"]), want, tag)
    gsel = np.take_along_axis(gi, np.maximum(sel_r, 0), 1)
    pg = np.where((sel_r >= 0) & want["pos"], np.asarray(gt_starts[:-1])[:, None] + gsel - 1, -1).reshape(-1)
    assert np.array_equal(_np(rec["pos_gt_inds"]).astype(np.int64), pg.astype(np.int64)), "(a) rcnn_targets: pos_gt_inds"
    # ---- the two extractors: the contract with float64 sums on the recorded FPN outputs, per-element bound of tests/_roi_extract_ref
    maps = [_np(rec[f"fpn{i}"].double().permute(0, 2, 3, 1)) for i in range(4)]
    for name, r, P in (("roi_feats", rec["rois"], 7), ("mask_feats", rec["rois"][rec["pos_idx"]], 14)):
        if r.shape[0] == 0:
            assert rec[name].shape[0] == 0
            continue
        ref = _roi_extract_ref.forward_vec(maps, _np(r.float()), [4, 8, 16, 32], P)
        ok, frac = _loss_ref.inside(_np(rec[name].permute(0, 2, 3, 1)), ref["out"], ref["bound"])
        _figure(tag, f"(a) extractor {name}, worst fraction of the bound", f"{frac:.3f}")
        assert ok, f"(a) {name}: {frac:.3f} of the bound"
    # ---- box head: each FC against float64 of its bf16-rounded operands on its recorded input, per element inside tests/_fc_ref.bound:
    # 2 (K + S + 1) u sum|terms| and the bf16 rounding of the output.  S, the number of K slices the library chose, is at most K / 64
    # (a slice holds at least one K tile), which is what the bound is taken with.  fc_reg writes fp32: S = 1, no output rounding.
    import _fc_ref
    x = cpu(rec["roi_feats"]).flatten(1)
    for i, name in enumerate(("fc0", "trunk")):
        w, b = cpu(rec.state[f"bbox_head.shared_fcs.{i}.weight"]), cpu(rec.state[f"bbox_head.shared_fcs.{i}.bias"])
        xb, wb = x.to(BF).double(), w.to(BF).double()
        y = F.relu(F.linear(xb, wb, b.double()))
        bound = _fc_ref.bound(xb.abs() @ wb.abs().T + b.double().abs(), x.shape[1], x.shape[1] // 64, y, True)
        ok, frac = _loss_ref.inside(_np(rec[name].double()), y.numpy(), bound.numpy())
        _figure(tag, f"(a) box head shared FC {i}, worst fraction of the bound", f"{frac:.3f}")
        assert ok, f"(a) box head shared FC {i}: {frac:.3f} of the bound"
        x = cpu(rec[name]).float()
    t = cpu(rec["trunk"]).double()
    w, b = cpu(rec.state["bbox_head.fc_reg.weight"]), cpu(rec.state["bbox_head.fc_reg.bias"])
    tb, wb = cpu(rec["trunk"]).to(BF).double(), w.to(BF).double()
    y = F.linear(tb, wb, b.double())
    ok, frac = _loss_ref.inside(_np(rec["bbox_pred"].double()), y.numpy(), _fc_ref.bound(tb.abs() @ wb.abs().T + b.double().abs(), t.shape[1], 1).numpy())
    _figure(tag, "(a) fc_reg, worst fraction of the bound", f"{frac:.3f}")
    assert ok, f"(a) fc_reg: {frac:.3f} of the bound"
    emb = cpu(rec.state["scores.all_embeddings"]).double()
    temp = cpu(rec.state["scores.detect_temperature"]).double()
    # No kernel runs at this stage: plain fp32 torch on the recorded trunk.  Per element, with E terms: the norm is a sum of E squares and a
    # root, (E / 2 + 2) u relative on every x / |x|, the division one u, the dot product in any order (E + 1) u of sum|terms|, the product
    # with the temperature one u: below (2 E + 8) u temp sum_e |x_e / |x|| |embed_ec|.
    xh = t / t.norm(dim=-1, keepdim=True)
    E = t.shape[1]
    ok, frac = _loss_ref.inside(_np(rec["cls_score"].double()), (xh @ emb * temp).numpy(), ((2 * E + 8) * U * temp.abs() * (xh.abs() @ emb.abs())).numpy())
    _figure(tag, "(a) class_logits (torch, no kernel), worst fraction of (2 E + 8) u temp sum|terms|", f"{frac:.3f}")
    assert ok, f"(a) class_logits: {frac:.3f} of the bound"
    # ---- box-head loss: the closed form with its bounds
    R = rec["cls_score"].shape[0]
    hc = dict(R=R, C1=NUM_CLASSES + 1, bg=NUM_CLASSES, x=_np(rec["cls_score"].float()), lw=_np(rec["lw"]), labels=_np(rec["labels"]), cw=None, avg=None,
              bp=_np(rec["bbox_pred"].float()), bt=_np(rec["bt"]), bw=_np(rec["bw"]))
    ref = _loss_ref.head_ref(hc)
    ok, frac = _loss_ref.inside(np.array([float(rec["loss_cls"]), float(rec["loss_bbox"])]), ref["out"][[0, 2]], ref["out_bound"][[0, 2]])
    _figure(tag, "(a) bbox_head_loss values, worst fraction of the bound", f"{frac:.3f}")
    assert ok, f"(a) bbox_head_loss: {frac:.3f} of the bound"
    ok, frac = _loss_ref.inside(_np(rec.grads["bbox_pred"]), ref["dbbox"], ref["dbbox_bound"])
    assert ok, f"(a) bbox_head_loss: gradient at bbox_pred at {frac:.3f} of the bound"
    ok, frac = _loss_ref.inside(_np(rec.grads["cls_score"]), ref["dcls"], ref["dcls_bound"])
    assert ok, f"(a) bbox_head_loss: gradient at cls_score at {frac:.3f} of the bound"
    # ---- mask head, mask targets, mask loss
    K = rec["mask_feats"].shape[0]
    if K:
        mh = TwinMaskHead(**MASK_HEAD).double().train()
        mh.load_state_dict({k[len("mask_head."):]: cpu(v).double() if v.dtype.is_floating_point else cpu(v) for k, v in rec.state.items()
                            if k.startswith("mask_head.")})
        v = rel_l2(rec["mask_pred"], mh(cpu(rec["mask_feats"]).double()))
        _figure(tag, "(a) mask head logits rel-L2", f"{v:.4e}")
        assert v <= PARITY_REL_L2, f"(a) mask head: {v:.3e}"
        pr = rec["rois"][rec["pos_idx"]]
        tv = _mask_ref.target_vec(_np(pr.float()), _np(rec["pos_gt_inds"][rec["pos_idx"]]), _np(torch.cat([cpu(m) for m in batch["gt_masks"]])), MASK)
        assert _mask_ref.binary_target_ok(tv, _np(rec["mask_targets"])), "(a) mask_target differs from the restatement outside its undecided cells"
        mc = dict(R=K, C=1, M=MASK, pred=_np(rec["mask_pred"].float()), labels=None, targets=_np(rec["mask_targets"]), w=np.ones(K, np.float32))
        ref = _mask_ref.loss_ref(mc)
        ok, frac = _mask_ref.inside(np.array([float(rec["loss_mask"])]), ref["out"][:1], ref["out_bound"][:1])
        _figure(tag, "(a) mask_loss value, fraction of the bound", f"{frac:.3f}")
        assert ok, f"(a) mask_loss: {frac:.3f} of the bound"
        ok, frac = _mask_ref.inside(_np(rec.grads["mask_pred"]), ref["dpred"], ref["dpred_bound"])
        assert ok, f"(a) mask_loss: gradient at mask_pred at {frac:.3f} of the bound"
    else:
        assert float(rec["loss_mask"]) == 0.0, "(a) mask_loss of no rows"


def _same_targets(what, got, want, tag):
    """The comparison of tests/test_gpu_det_targets.py: `got` (tensors of any leading shape) against the record of _assign_ref.targets --
    labels, label weights, box weights and dx, dy bit for bit, dw, dh exactly 0 off the positives, inside `bound` against `t64` on them
    (the bound _assign_ref.bbox2delta derives for a device logf), and the restatement's own bits where gwh == pwh."""
    g = {k: v.detach().cpu().numpy().reshape(want[k].shape) for k, v in got.items()}
    assert np.array_equal(g["labels"].astype(np.int64), want["labels"].astype(np.int64)), \
        f"{what}: labels differ in {int((g['labels'] != want['labels']).sum())} slots"
    for k in ("label_weights", "bbox_weights"):
        assert _assign_ref.same_float_bits(g[k], want[k]), f"{what}: {k} differ"
    bt, ref = g["bbox_targets"], want["bbox_targets"]
    assert _assign_ref.same_float_bits(np.ascontiguousarray(bt[..., :2]), np.ascontiguousarray(ref[..., :2])), f"{what}: dx, dy differ in bits"
    pos = want["pos"]
    assert not bt[..., 2:][~pos].any(), f"{what}: dw, dh off the positives are not 0"
    frac = 0.0
    if pos.any():
        d, t64, bound = bt[..., 2:][pos].astype(np.float64), want["t64"][..., 2:][pos], want["bound"][..., 2:][pos]
        ok, frac = _loss_ref.inside(d, t64, bound)
        assert ok, f"{what}: dw, dh at {frac:.3f} of the bound"
    assert _assign_ref.same_float_bits(bt[want["unit"]], ref[want["unit"]]), f"{what}: gwh == pwh must give exactly (0 - mean) / std"
    _figure(tag, f"{what} dw, dh on {int(pos.sum())} positives, worst fraction of the bound", f"{frac:.3f}")


# ------------------------------------------------------------------------------------------------ (b) backward seams by replay
def _fold_matches(total, terms):
    """Whether `total` has the bits of a left-to-right fp32 sum of `terms` in SOME order: autograd accumulates the consumers' gradients one
    after another in an order of its own, fp32 addition commutes, so these folds are all the sums it can form.  -> the order or None."""
    for order in itertools.permutations(range(len(terms))):
        acc = terms[order[0]].float().clone()
        for j in order[1:]:
            acc = acc + terms[j].float()
        if bits_equal(total.float().contiguous(), acc.contiguous()):
            return order
    return None


def _nchw(t):
    return t.detach().clone().contiguous().requires_grad_(True)


def check_replay(rec, asm, ops=None, tag="CPU backend"):
    """(b): each consumer of a seam tensor alone, on a fresh module with the recorded state and a detached contiguous NCHW clone of the
    recorded input, forward and backward with the recorded upstream gradient.  Outputs and seam gradients bit for bit; the RPN stack's
    parameter gradients, a sum over five calls, inside 2 L 2^-24 sum |terms|."""
    L = 5
    fresh = lambda: fresh_like(asm, ops, rec.state).train()
    # ---- the RPN stack, level by level
    rpn_dx, rpn_dp = [], []
    for i in range(L):
        m = fresh().rpn_head
        x = _nchw(rec[f"fpn{i}"])
        c, r = m.forward_single(x)
        assert bits_equal(c, rec[f"rpn_cls{i}"]) and bits_equal(r, rec[f"rpn_reg{i}"]), f"(b) RPN level {i}: chain output != stand-alone output"
        torch.autograd.backward([c, r], [rec.grads[f"rpn_cls{i}"], rec.grads[f"rpn_reg{i}"]])
        rpn_dx.append(x.grad)
        rpn_dp.append({k: p.grad.detach().double() for k, p in m.named_parameters()})
    worst = 0.0
    for k in rpn_dp[0]:
        total = sum(d[k] for d in rpn_dp)
        bound = 2 * L * U * sum(d[k].abs() for d in rpn_dp)
        got = rec.param_grads[f"rpn_head.{k}"].double().cpu()
        err = (got - total.cpu()).abs()
        assert bool((err <= bound.cpu()).all()), f"(b) rpn_head.{k}: the chain's gradient is not the sum of the per-level replays"
        worst = max(worst, float((err / bound.cpu().clamp_min(1e-300)).max()))
    _figure(tag, "(b) RPN parameter gradients against the sum of 5 replays, worst fraction of 2 L u sum|terms|", f"{worst:.3f}")
    # ---- the two extractors
    ext_dx = {}
    for name, mod, rois in (("roi_feats", "bbox_roi_extractor", rec["rois"]), ("mask_feats", "mask_roi_extractor", rec["rois"][rec["pos_idx"]])):
        xs = [_nchw(rec[f"fpn{i}"]) for i in range(4)]
        out = getattr(fresh(), mod)(xs, rois)
        assert bits_equal(out, rec[name]), f"(b) {name}: chain output != stand-alone output on the recorded FPN levels"
        if rec.grads.get(name) is not None and out.requires_grad:
            out.backward(rec.grads[name])
        ext_dx[name] = [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]
    # ---- every FPN output: the sum of its consumers
    for i in range(L):
        terms = [rpn_dx[i]]
        if i < 4:
            terms += [ext_dx["roi_feats"][i], ext_dx["mask_feats"][i]]
        if i == 3:                                                       # level 4 is the subsample [..., ::2, ::2] of level 3
            up = torch.zeros_like(rec[f"fpn3"])
            up[..., ::2, ::2] = rec.grads["fpn4"]
            terms.append(up)
        order = _fold_matches(rec.grads[f"fpn{i}"], terms)
        _figure(tag, f"(b) FPN output {i}: gradient = sum of {len(terms)} consumer replays", "equal bits" if order is not None else "DIFFERENT")
        assert order is not None, f"(b) FPN output {i}: the chain's gradient is no sum of its {len(terms)} consumers' replays"
    # ---- RoI features -> shared FCs; trunk -> class branch + fc_reg
    f = fresh()
    x = _nchw(rec["roi_feats"])
    trunk = x
    for fc in f.bbox_head.shared_fcs:
        trunk = fc(trunk)
    assert bits_equal(trunk, rec["trunk"]), "(b) shared FCs: chain output != stand-alone output on the NCHW clone of the RoI features"
    trunk.backward(rec.grads["trunk"])
    assert bits_equal(x.grad, rec.grads["roi_feats"]), "(b) RoI features: gradient != the shared FCs' replay"
    t1, t2 = _nchw(rec["trunk"]), _nchw(rec["trunk"])
    f = fresh()
    cs = f.scores.class_logits(t1)
    assert bits_equal(cs, rec["cls_score"]), "(b) class_logits: chain output != stand-alone output"
    cs.backward(rec.grads["cls_score"])
    bp = f.bbox_head.fc_reg(t2)
    assert bits_equal(bp, rec["bbox_pred"]), "(b) fc_reg: chain output != stand-alone output"
    bp.backward(rec.grads["bbox_pred"])
    order = _fold_matches(rec.grads["trunk"], [t1.grad, t2.grad])
    _figure(tag, "(b) FC trunk: gradient = class branch + fc_reg replays", "equal bits" if order is not None else "DIFFERENT")
    assert order is not None, "(b) FC trunk: the chain's gradient is not the sum of its two consumers' replays"
    # ---- mask features -> mask head
    if rec["mask_feats"].shape[0]:
        x = _nchw(rec["mask_feats"])
        mp = fresh().mask_head(x)
        assert bits_equal(mp, rec["mask_pred"]), "(b) mask head: chain output != stand-alone output"
        mp.backward(rec.grads["mask_pred"])
        assert bits_equal(x.grad, rec.grads["mask_feats"]), "(b) mask features: gradient != the mask head's replay"
        _figure(tag, "(b) RoI features, mask features: gradient = the head's replay", "equal bits")


# ------------------------------------------------------------------------------------------------ (c) the scalars
LOSS_TERMS = ("loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask", "total")


def check_scalars(rec, batch, keys, tag="CPU backend"):
    """(c): every loss term against the float64 torch route on the same leaves and state, handed the kernel route's discrete decisions."""
    ref = Assembly(False).double()
    ref.load_state_dict({k: v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu() for k, v in rec.state.items()})
    host = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != "maps"}
    host["maps"] = [rec[f"leaf{i}"].cpu() for i in range(4)]
    host["gt_bboxes"], host["gt_labels"], host["gt_masks"] = ([t.cpu() for t in batch[k]] for k in ("gt_bboxes", "gt_labels", "gt_masks"))
    dec = Record()
    dec.update({k: v.detach().cpu() for k, v in rec.items()})
    want = train_step(ref, host, None, decisions=dec)
    worst = 0.0
    for k in LOSS_TERMS:
        a, b = float(rec[k]), float(want[k])
        rel = abs(a - b) / max(abs(b), 1e-300) if b != 0 else abs(a)
        _figure(tag, f"(c) {k}", f"kernel route {a:.8e}, float64 torch route {b:.8e}, relative {rel:.3e}")
        worst = max(worst, rel)
    assert worst <= PARITY_REL_L2, f"(c) a loss term is {worst:.3e} from the float64 torch route (threshold {PARITY_REL_L2})"
    return want


# ------------------------------------------------------------------------------------------------ (e) empty and ragged rows
def check_ragged(rec, asm, tag="CPU backend"):
    """(e): every loss and gradient finite; the image without ground truth (index 1) contributes only negatives; with no positive at all
    the mask loss is 0 and every mask-head parameter gradient is zero or None."""
    for k in LOSS_TERMS:
        assert bool(torch.isfinite(rec[k]).all()), f"(e) {k} is not finite"
    for name, g in list(rec.grads.items()) + list(rec.param_grads.items()):
        assert g is None or bool(torch.isfinite(g).all()), f"(e) the gradient at {name} is not finite"
    num = TRAIN_CFG["rcnn"]["sampler"]["num"]
    lab = rec["labels"].reshape(B, num).cpu()
    live = rec["lw"].reshape(B, num).cpu() > 0
    assert bool((lab[1][live[1]] == NUM_CLASSES).all()), "(e) the image without ground truth has a sampled row that is not background"
    assert bool((rec["rpn_labels"][1][rec["rpn_lw"][1] > 0] == 1).all()), "(e) the image without ground truth has a foreground anchor"
    counts = rec["counts"].cpu()
    props = rec["proposals"].cpu()
    for b in range(B):                                                   # a sampled row is a ground truth or one of the first counts[b] proposals
        rows = rec["rois"].reshape(B, num, 5)[b].cpu()
        rows = rows[rows[:, 0] >= 0][:, 1:]
        pool = torch.cat([props[b, :int(counts[b]), :4], rec.gt[b]])
        hit = (rows[:, None, :] == pool[None, :, :]).all(-1).any(1) if rows.numel() else torch.ones(0, dtype=torch.bool)
        assert bool(hit.all()), f"(e) image {b}: {int((~hit).sum())} sampled rows are neither ground truth nor one of its {int(counts[b])} proposals"
    if rec["pos_idx"].numel() == 0:
        assert float(rec["loss_mask"]) == 0.0, "(e) mask_loss with K = 0"
        for k, g in rec.param_grads.items():
            if k.startswith("mask_head."):
                assert g is None or float(g.abs().max()) == 0.0, f"(e) {k} has a gradient without a positive"
    _figure(tag, "(e) sampled positives per image", [int(((lab[b] < NUM_CLASSES) & live[b]).sum()) for b in range(B)])
