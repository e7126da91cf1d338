"""Times the detector's losses on the MI355X: csl_rpn_loss and csl_bbox_head_loss (HipOps.rpn_loss / bbox_head_loss,
clipself_amd/det_losses.py) against mmdet 2.28.1's formulation in fp32 torch on the same device: per level permute().reshape() of the
dense maps, _expand_onehot_labels (nonzero) + binary_cross_entropy_with_logits, L1 on the boxes, weight_reduce_loss; for the box head
the reference's cross_entropy with its in-place -inf on a copy of the logits, `avg_factor = max(sum(label_weights > 0).item(), 1)`,
accuracy through topk, `if pos_inds.any()` and boolean-mask indexing; backward through autograd.  The per-level target lists mmdet's
get_targets hands to loss_single are built outside the timed region.

Shapes, 8 images:
  rpn640    5 levels of a 640^2 image, A = 3: 8 x 102 300 anchors, 256 sampled per image
  rpn1024   5 levels of a 1024^2 image:       8 x 261 888 anchors, 256 sampled per image
  head66    R = 8 x 512 rows, C1 = 66 (OV-COCO: 48 base classes weighted 1, 17 novel masked, background)
  head1204  R = 8 x 512 rows, C1 = 1204 (OV-LVIS: 337 rare classes masked, background 0.9)

Method: every variant is warmed up; a window is `--iters` calls between two device events; `--windows` windows per variant, the variants
alternated window by window in one process; the median and the spread (min .. max) are reported.  "fwd" is the losses alone, "fwd+bwd"
the losses, backward() with a non-unit upstream gradient on every loss, and the gradients of all predictions (for the kernels: the
autograd Functions of det_losses, so the upstream multiply of the saved gradients is included).  Prints a markdown table and one JSON
line per shape."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BACKBONE_FWD_BWD_MS = 22.0                                 # the B/16 backbone forward + backward, 8 images (profiles/neck_bench.md)
EPS = torch.finfo(torch.float32).eps


def mmdet_rpn(cls_scores, bbox_preds, lab_l, lw_l, bt_l, bw_l, num_total_samples):
    """RPNHead.loss as mmdet 2.28.1 writes it: loss_single per level."""
    out_c, out_b = [], []
    for cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights in zip(cls_scores, bbox_preds, lab_l, lw_l, bt_l, bw_l):
        labels, label_weights = labels.reshape(-1), label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, 1)
        bin_labels = labels.new_full((labels.size(0), 1), 0)
        valid_mask = (labels >= 0) & (labels != -100)
        inds = torch.nonzero(valid_mask & (labels < 1), as_tuple=False)
        if inds.numel() > 0:
            bin_labels[inds, labels[inds]] = 1
        weight = label_weights.view(-1, 1) * valid_mask.view(-1, 1).float()
        loss = F.binary_cross_entropy_with_logits(cls_score, bin_labels.float(), reduction="none")
        out_c.append((loss * weight).sum() / (num_total_samples + EPS))
        bbox_targets, bbox_weights = bbox_targets.reshape(-1, 4), bbox_weights.reshape(-1, 4)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        out_b.append((torch.abs(bbox_pred - bbox_targets) * bbox_weights).sum() / (num_total_samples + EPS))
    return out_c, out_b


def mmdet_head(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, class_weight, bg):
    """BBoxHead.loss (reg_class_agnostic=True) with the reference's cross_entropy."""
    avg_factor = max(torch.sum(label_weights > 0).float().item(), 1.)
    pred = cls_score.clone()                                # the reference writes into the head's output; a copy keeps the runs equal
    mask_out = class_weight < 0.00001
    pred[:, mask_out] = -float("inf")
    loss = F.cross_entropy(pred, labels, weight=class_weight, reduction="none", ignore_index=-100)
    loss_cls = (loss * label_weights).sum() / (avg_factor + EPS)
    _, pred_label = pred.topk(1, dim=1)
    acc = pred_label.t().eq(labels.view(1, -1)).reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / pred.size(0))
    pos_inds = (labels >= 0) & (labels < bg)
    if pos_inds.any():
        loss_bbox = (torch.abs(bbox_pred[pos_inds] - bbox_targets[pos_inds]) * bbox_weights[pos_inds]).sum() / (bbox_targets.size(0) + EPS)
    else:
        loss_bbox = bbox_pred[pos_inds].sum()
    return loss_cls, acc, loss_bbox


def alternate(variants, iters, n_windows):
    """{name: fn} -> {name: (median, min, max)} ms per call; one window of each variant in turn."""
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(n_windows):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def rpn_shape(side, B, ops, gen):
    from clipself_amd import det_losses as D
    A, sizes = 3, [(side // s, side // s) for s in (4, 8, 16, 32, 64)]
    N = sum(h * w * A for h, w in sizes)
    cls = [torch.randn(B, A, h, w, generator=gen).cuda().requires_grad_() for h, w in sizes]
    reg = [torch.randn(B, 4 * A, h, w, generator=gen).cuda().requires_grad_() for h, w in sizes]
    labels = torch.ones(B, N, dtype=torch.int32)
    lw, bt, bw = torch.zeros(B, N), torch.zeros(B, N, 4), torch.zeros(B, N, 4)
    for b in range(B):
        pick = torch.randperm(N, generator=gen)[:256]
        lw[b, pick] = 1
        labels[b, pick[:128]] = 0
        bw[b, pick[:128]] = 1
        bt[b, pick[:128]] = torch.randn(128, 4, generator=gen)
    labels, lw, bt, bw = labels.cuda(), lw.cuda(), bt.cuda(), bw.cuda()
    num = torch.tensor(256 * B, device="cuda")
    avg = num.to(torch.float32).reshape(1)
    up = [0.5 + 0.1 * l for l in range(len(sizes))]
    # what mmdet's get_targets hands over: per-level lists (images_to_levels), labels as int64
    lab_l, lw_l, bt_l, bw_l, off = [], [], [], [], 0
    for h, w in sizes:
        n = h * w * A
        lab_l.append(labels[:, off:off + n].long().contiguous()), lw_l.append(lw[:, off:off + n].contiguous())
        bt_l.append(bt[:, off:off + n].contiguous()), bw_l.append(bw[:, off:off + n].contiguous())
        off += n
    preds = cls + reg

    def clear():
        for p in preds:
            p.grad = None

    def k_fwd():
        ops.rpn_loss([c.detach() for c in cls], [r.detach() for r in reg], labels, lw, bt, bw, avg, grad=False)

    def k_call():
        ops.rpn_loss([c.detach() for c in cls], [r.detach() for r in reg], labels, lw, bt, bw, avg, grad=True)

    def k_fb():
        clear()
        out = D.rpn_loss(cls, reg, labels, lw, bt, bw, num, ops=ops, fused=True)
        sum(u * (a + b) for u, a, b in zip(up, out["loss_rpn_cls"], out["loss_rpn_bbox"])).backward()

    def t_fwd():
        with torch.no_grad():
            mmdet_rpn(cls, reg, lab_l, lw_l, bt_l, bw_l, 256.0 * B)

    def t_fb():
        clear()
        oc, ob = mmdet_rpn(cls, reg, lab_l, lw_l, bt_l, bw_l, 256.0 * B)
        sum(u * (a + b) for u, a, b in zip(up, oc, ob)).backward()

    return dict(kernel_fwd=k_fwd, kernel_fwd_with_grads=k_call, kernel_fwd_bwd=k_fb, torch_fwd=t_fwd, torch_fwd_bwd=t_fb), N


def head_shape(C1, B, ops, gen):
    from clipself_amd import det_losses as D
    R, bg = B * 512, C1 - 1
    x = (torch.randn(R, C1, generator=gen) * 3).cuda().requires_grad_()
    bp = torch.randn(R, 4, generator=gen).cuda().requires_grad_()
    cw = torch.ones(C1)
    masked = 17 if C1 == 66 else 337
    cw[torch.randperm(bg, generator=gen)[:masked]] = 0
    cw[-1] = 0.9 if C1 != 66 else 1.0
    live = torch.nonzero(cw[:bg] > 0)[:, 0]
    labels = torch.full((R,), bg, dtype=torch.int32)
    lw, bt, bw = torch.ones(R), torch.zeros(R, 4), torch.zeros(R, 4)
    for b in range(B):
        s = b * 512
        labels[s:s + 128] = live[torch.randint(0, live.numel(), (128,), generator=gen)].to(torch.int32)
        bw[s:s + 128] = 1
        bt[s:s + 128] = torch.randn(128, 4, generator=gen)
        lw[s + 500:s + 512] = 0                               # slots the sampler could not fill
    labels, lw, bt, bw, cw_d = labels.cuda(), lw.cuda(), bt.cuda(), bw.cuda(), cw.cuda()
    labels64 = labels.long()
    loss_cls = D.CustomCrossEntropyLoss(use_sigmoid=False, class_weight=cw.tolist())

    def clear():
        x.grad = bp.grad = None

    def k_fwd():
        ops.bbox_head_loss(x.detach(), labels, lw, bp.detach(), bt, bw, bg, cw_d, None, grad=False)

    def k_call():
        ops.bbox_head_loss(x.detach(), labels, lw, bp.detach(), bt, bw, bg, cw_d, None, grad=True)

    def k_fb():
        clear()
        out = D.bbox_head_loss(x, bp, labels, lw, bt, bw, loss_cls=loss_cls, num_classes=bg, ops=ops, fused=True)
        (0.7 * out["loss_cls"] + 1.3 * out["loss_bbox"]).backward()

    def t_fwd():
        with torch.no_grad():
            mmdet_head(x, bp, labels64, lw, bt, bw, cw_d, bg)

    def t_fb():
        clear()
        lc, _, lb = mmdet_head(x, bp, labels64, lw, bt, bw, cw_d, bg)
        (0.7 * lc + 1.3 * lb).backward()

    return dict(kernel_fwd=k_fwd, kernel_fwd_with_grads=k_call, kernel_fwd_bwd=k_fb, torch_fwd=t_fwd, torch_fwd_bwd=t_fb), R


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--shapes", default="rpn640,rpn1024,head66,head1204")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args(argv)

    from clipself_amd.hip import HipOps
    ops = HipOps()
    gen = torch.Generator().manual_seed(0)
    rows = []
    for name in args.shapes.split(","):
        if name.startswith("rpn"):
            variants, n = rpn_shape(int(name[3:]), args.images, ops, gen)
        else:
            variants, n = head_shape(int(name[4:]), args.images, ops, gen)
        res = alternate(variants, args.iters, args.windows)
        rows.append((name, n, res))
        print(json.dumps(dict(shape=name, images=args.images, rows=n,
                              **{k + "_ms": dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for k, v in res.items()})), flush=True)
    print("\n| shape | rows | kernel fwd ms | kernel fwd + grads (one call) ms | kernel fwd + bwd ms (min .. max) | torch fwd ms | torch fwd + bwd ms (min .. max) | "
          "fwd + bwd: torch / kernel | kernel fwd + bwd of the 22 ms backbone fwd + bwd |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, n, r in rows:
        kb, tb = r["kernel_fwd_bwd"], r["torch_fwd_bwd"]
        print(f"| {name} | {n} | {r['kernel_fwd'][0]:.3f} | {r['kernel_fwd_with_grads'][0]:.3f} | {kb[0]:.3f} ({kb[1]:.3f} .. {kb[2]:.3f}) | "
              f"{r['torch_fwd'][0]:.3f} | {tb[0]:.3f} ({tb[1]:.3f} .. {tb[2]:.3f}) | {tb[0] / kb[0]:.1f} x | {100 * kb[0] / BACKBONE_FWD_BWD_MS:.1f} % |")


if __name__ == "__main__":
    main()
