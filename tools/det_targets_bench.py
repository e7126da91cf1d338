"""Times the detector's training-target stage on the MI355X: csa_assign, csa_sample and csa_targets (HipOps.assign / sample / bbox_targets,
clipself_amd/det_targets.py) against the route mmdet takes on the same device -- plain torch on the GPU, once per image: the [G, N] IoU
matrix in memory, two max passes, a Python loop over the ground truths for the low-quality matches, nonzero() / randperm with their
host read-backs, bbox2delta on the sampled rows.

Shapes, 8 images, 64 ground truths per image:
  rpn640    102 300 anchors (3 x (160^2 + ... + 10^2), a 640^2 image), MaxIoUAssigner(0.7, 0.3, 0.3, match_low_quality), RandomSampler(256, 0.5)
  rpn1024   261 888 anchors (a 1024^2 image), the same configuration
  rcnn      1000 proposals + the ground truths in front, MaxIoUAssigner(0.5, 0.5, 0.5), RandomSampler(512, 0.25), stds (.1, .1, .2, .2)
Ground truths: seeded boxes of 3 .. 40 % of the image side.  Proposals: jittered ground truths and random boxes, half each.

Method: every shape is warmed up; a window is `--iters` calls between two device events; `--windows` windows, the median and the spread
(min .. max) are reported, per stage and for the three together.  The torch-on-device route is timed with the host clock around a
synchronised loop of `--torch-reps` calls (it synchronises by itself, many times per image).  Prints a markdown table and one JSON line
per shape."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BACKBONE_FWD_BWD_MS = 22.0                                 # the B/16 backbone forward + backward, 8 images (profiles/neck_bench.md)
SHAPES = {
    "rpn640": dict(side=640, rpn=True),
    "rpn1024": dict(side=1024, rpn=True),
    "rcnn": dict(side=1024, rpn=False, proposals=1000),
}


def make_gts(images, per_image, side, gen):
    out = []
    for _ in range(images):
        wh = (torch.rand(per_image, 2, generator=gen) * 0.37 + 0.03) * side
        xy = torch.rand(per_image, 2, generator=gen) * (side - wh)
        out.append(torch.cat([xy, xy + wh], dim=1))
    return out


def make_proposals(gts, n, side, gen):
    out = []
    for g in gts:
        pick = torch.randint(0, g.shape[0], (n,), generator=gen)
        near = g[pick] + torch.randn(n, 4, generator=gen) * 6.0
        wh = (torch.rand(n, 2, generator=gen) * 0.4 + 0.02) * side
        xy = torch.rand(n, 2, generator=gen) * (side - wh)
        far = torch.cat([xy, xy + wh], dim=1)
        use = (torch.rand(n, generator=gen) < 0.5) & (near[:, 2] > near[:, 0] + 1) & (near[:, 3] > near[:, 1] + 1)
        out.append(torch.where(use[:, None], near, far))
    return out


def mmdet_style_image(boxes, gts, pos_thr, neg_thr, min_pos, low_quality, num, pos_fraction, prefix, stds):
    """What mmdet runs for one image, in torch on the device of `boxes`."""
    from clipself_amd.det_targets import bbox_overlaps
    overlaps = bbox_overlaps(gts, boxes)                                   # [G, N] in memory
    max_ov, argmax = overlaps.max(dim=0)
    gt_max, _ = overlaps.max(dim=1)
    gt_inds = overlaps.new_full((boxes.shape[0],), -1, dtype=torch.long)
    gt_inds[(max_ov >= 0) & (max_ov < neg_thr)] = 0
    pos = max_ov >= pos_thr
    gt_inds[pos] = argmax[pos] + 1
    if low_quality:
        for i in range(gts.shape[0]):
            if gt_max[i] >= min_pos:                                         # a read-back per ground truth
                gt_inds[overlaps[i, :] == gt_max[i]] = i + 1
    if prefix:
        boxes = torch.cat([gts, boxes])
        gt_inds = torch.cat([torch.arange(1, gts.shape[0] + 1, device=boxes.device), gt_inds])
    pos_inds = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(1)
    want = int(num * pos_fraction)
    if pos_inds.numel() > want:
        pos_inds = pos_inds[torch.randperm(pos_inds.numel(), device=boxes.device)[:want]]
    neg_inds = torch.nonzero(gt_inds == 0, as_tuple=False).squeeze(1)
    want = num - pos_inds.numel()
    if neg_inds.numel() > want:
        neg_inds = neg_inds[torch.randperm(neg_inds.numel(), device=boxes.device)[:want]]
    p, g = boxes[pos_inds], gts[gt_inds[pos_inds] - 1]
    pxy, pwh = (p[:, :2] + p[:, 2:]) * 0.5, p[:, 2:] - p[:, :2]
    gxy, gwh = (g[:, :2] + g[:, 2:]) * 0.5, g[:, 2:] - g[:, :2]
    deltas = torch.cat([(gxy - pxy) / pwh, (gwh / pwh).log()], dim=1) / torch.tensor(stds, device=boxes.device)
    labels = boxes.new_full((boxes.shape[0],), 1, dtype=torch.long)
    labels[pos_inds] = 0
    weights = boxes.new_zeros(boxes.shape[0])
    weights[pos_inds] = 1
    weights[neg_inds] = 1
    targets = boxes.new_zeros(boxes.shape[0], 4)
    targets[pos_inds] = deltas
    return labels, weights, targets


def windows(fn, iters, n_windows):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--gts", type=int, default=64)
    ap.add_argument("--shapes", default="rpn640,rpn1024,rcnn")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=2, help="0 = skip the torch-on-device route")
    args = ap.parse_args(argv)

    from clipself_amd import det_targets as T
    from clipself_amd.hip import HipOps
    ops = HipOps()
    gen = torch.Generator().manual_seed(0)
    rows = []
    for name in args.shapes.split(","):
        sp = SHAPES[name]
        side, B = sp["side"], args.images
        gts = make_gts(B, args.gts, side, gen)
        gts_dev = [g.cuda() for g in gts]
        gt_starts = torch.arange(B + 1, dtype=torch.int32, device="cuda") * args.gts
        gcat = torch.cat(gts_dev)
        if sp["rpn"]:
            ag = T.AnchorGenerator(strides=[4, 8, 16, 32, 64], ratios=[0.5, 1.0, 2.0], scales=[8])
            boxes = torch.cat(ag.grid_priors([(side // s, side // s) for s in (4, 8, 16, 32, 64)], device="cuda"))
            starts, N, prefix = None, boxes.shape[0], False
            thr = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True)
            num, frac, stds, bg = 256, 0.5, (1., 1., 1., 1.), 1
            per_image = [boxes] * B
        else:
            props = make_proposals(gts, sp["proposals"], side, gen)
            per_image = [p.cuda() for p in props]
            boxes = torch.cat([torch.cat([g, p]) for g, p in zip(gts_dev, per_image)]).contiguous()
            N, prefix = args.gts + sp["proposals"], True
            starts = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
            thr = dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False)
            num, frac, stds, bg = 512, 0.25, (.1, .1, .2, .2), 65
        K = boxes.shape[0]
        keys = T.random_keys((B, N), "cuda", torch.Generator(device="cuda").manual_seed(1))
        state = {}

        def assign():
            state["gi"], state["mo"] = ops.assign(boxes, starts, gcat, gt_starts, B, N, args.gts, gt_prefix=prefix, **thr)

        def sample():
            state["fl"], state["sel"], state["cnt"] = ops.sample(state["gi"], keys, starts, K, gt_starts, gcat.shape[0], args.gts, num, int(num * frac))

        def targets():
            if sp["rpn"]:
                ops.bbox_targets(boxes, starts, gcat, None, gt_starts, args.gts, state["gi"], flags=state["fl"], stds=stds, bg_label=bg)
            else:
                ops.bbox_targets(boxes, starts, gcat, None, gt_starts, args.gts, state["gi"], sel=state["sel"], stds=stds, bg_label=bg)

        def assign_plain():                                 # the first IoU pass alone: no per-ground-truth maximum, no second pass
            ops.assign(boxes, starts, gcat, gt_starts, B, N, args.gts, gt_prefix=prefix, **dict(thr, match_low_quality=False))

        def all_three():
            assign(), sample(), targets()

        all_three()
        torch.cuda.synchronize()
        counts = state["cnt"].tolist()
        res = {k: windows(f, args.iters, args.windows) for k, f in (("assign", assign), ("assign_no_lowq", assign_plain), ("sample", sample), ("targets", targets),
                                                                    ("all", all_three))}
        torch_ms = None
        if args.torch_reps > 0:
            def torch_route():
                for b in range(B):
                    mmdet_style_image(per_image[b], gts_dev[b], thr["pos_iou_thr"], thr["neg_iou_thr"], thr["min_pos_iou"], thr["match_low_quality"],
                                      num, frac, prefix, stds)
            torch_route()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.torch_reps):
                torch_route()
            torch.cuda.synchronize()
            torch_ms = (time.perf_counter() - t0) * 1e3 / args.torch_reps
        rows.append((name, N, res, torch_ms, counts))
        print(json.dumps(dict(shape=name, images=B, rows_per_image=N, gts_per_image=args.gts, sampled=counts,
                              **{k + "_ms": dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for k, v in res.items()},
                              torch_on_device_ms=None if torch_ms is None else round(torch_ms, 2))))
    print("\n| shape | rows / image | assign ms | sample ms | targets ms | all three ms (min .. max) | torch on device ms | of the 22 ms backbone fwd + bwd |")
    print("|---|---|---|---|---|---|---|---|")
    for name, N, res, torch_ms, _ in rows:
        a = res["all"]
        print(f"| {name} | {N} | {res['assign'][0]:.3f} | {res['sample'][0]:.3f} | {res['targets'][0]:.3f} | {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) | "
              f"{'-' if torch_ms is None else f'{torch_ms:.1f}'} | {100 * a[0] / BACKBONE_FWD_BWD_MS:.1f} % |")


if __name__ == "__main__":
    main()
