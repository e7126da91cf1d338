"""Times the RPN proposal step on the MI355X: csp_select (HipOps.rpn_select) and the whole det_proposals.rpn_proposals against the torch
route of clipself_amd/det_proposals.py on the same device -- mmdet's formulation: per level a sigmoid, a sort, gathers and a decode, then
the existing csd_nms.  The comparison is never the new kernels against themselves.

Shapes, 8 images, A = 3, five levels (strides 4 .. 64), nms_pre 2000, max_per_img 1000, iou 0.7:
  640    levels 160, 80, 40, 20, 10 squared    N = 102 300 anchors per image
  1024   levels 256, 128, 64, 32, 16 squared   N = 261 888
Maps: seeded normal logits (sigma 2, mean -2) and deltas (sigma 0.5); anchors from det_targets.AnchorGenerator (ratios 0.5, 1, 2, scale 8).

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  The two routes' outputs
are compared on every shape (anchor indices and levels equal, boxes and scores to the last bits of torch's exp).  Prints a markdown table
and one JSON line per shape.  Each figure is also given as a share of the 22 ms backbone forward + backward (profiles/neck_bench.md);
for `select`, the bytes it must read (the cls maps once) are set against its time."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BACKBONE_MS = 22.0                                         # backbone forward + backward, 8 images (profiles/neck_bench.md)
SHAPES = {"640": 640, "1024": 1024}
STRIDES = (4, 8, 16, 32, 64)
CFG = dict(nms_pre=2000, max_per_img=1000, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)


def make_shape(side, images, A, gen):
    from clipself_amd.det_targets import AnchorGenerator
    sizes = [(side // s, side // s) for s in STRIDES]
    cls = [(torch.randn(images, A, h, w, generator=gen) * 2 - 2).cuda() for h, w in sizes]
    reg = [(torch.randn(images, 4 * A, h, w, generator=gen) * 0.5).cuda() for h, w in sizes]
    gen_a = AnchorGenerator(strides=list(STRIDES), ratios=[0.5, 1.0, 2.0], scales=[8])
    anchors = torch.cat(gen_a.grid_priors(sizes, device="cuda"), 0).contiguous()
    shapes = torch.tensor([[float(side), float(side)]] * images, device="cuda")
    return cls, reg, anchors, shapes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--shapes", default="640,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args(argv)
    from clipself_amd import det_proposals as D
    from clipself_amd.hip import HipOps
    ops = HipOps()
    A = 3
    print(f"{args.images} images; windows of {args.iters} calls, {args.windows} windows, variants alternated\n")
    print("| shape | anchors / image | variant | µs median (min .. max) | torch route / kernels | share of the 22 ms backbone fwd + bwd | cls bytes read once | GB/s of cls |")
    print("|---|---|---|---|---|---|---|---|")
    for name in args.shapes.split(","):
        cls, reg, anchors, shapes = make_shape(SHAPES[name], args.images, A, torch.Generator().manual_seed(0))
        N = anchors.shape[0]
        variants = {
            "select, kernels": lambda: D.select(cls, reg, anchors, shapes, CFG["nms_pre"], ops=ops, fused=True),
            "select, torch route": lambda: D.select(cls, reg, anchors, shapes, CFG["nms_pre"], ops=ops, fused=False),
            "rpn_proposals, kernels": lambda: D.rpn_proposals(cls, reg, anchors, shapes, CFG, ops=ops, fused=True, return_inds=True),
            "rpn_proposals, torch route": lambda: D.rpn_proposals(cls, reg, anchors, shapes, CFG, ops=ops, fused=False, return_inds=True),
        }
        outs = {k: fn() for k, fn in variants.items()}
        torch.cuda.synchronize()
        sk, st = outs["select, kernels"], outs["select, torch route"]
        pk, pt = outs["rpn_proposals, kernels"], outs["rpn_proposals, torch route"]
        agree = dict(select_inds_equal=bool(torch.equal(sk[3], st[3])), select_levels_equal=bool(torch.equal(sk[2], st[2])),
                     select_box_max_abs_diff=float((sk[0] - st[0]).abs().max()), select_score_max_abs_diff=float((sk[1] - st[1]).abs().max()),
                     proposals_counts_equal=bool(torch.equal(pk[1], pt[1])), proposals_inds_equal=bool(torch.equal(pk[3], pt[3])),
                     counts=pk[1].tolist())

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters * 1e3

        for fn in variants.values():
            window(fn)
        times = {k: [] for k in variants}
        for _ in range(args.windows):
            for k, fn in variants.items():
                times[k].append(window(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        cls_bytes = args.images * N * 4
        for k in variants:
            base = med[k.replace("torch route", "kernels")]
            ratio = f"{med[k] / base:.1f} x" if "torch" in k else ""
            bw = f"{cls_bytes / med[k] / 1e3:.0f}" if k == "select, kernels" else ""
            print(f"| {name} | {N} | {k} | {med[k]:.0f} ({min(times[k]):.0f} .. {max(times[k]):.0f}) | {ratio} | {100 * med[k] / 1e3 / BACKBONE_MS:.2f} % | "
                  f"{cls_bytes if k.startswith('select') else ''} | {bw} |")
        print(json.dumps(dict(shape=name, N=N, median_us=med, all_us=times, cls_bytes=cls_bytes, **agree)), file=sys.stderr)


if __name__ == "__main__":
    main()
