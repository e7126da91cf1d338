"""Times the detector's open-vocabulary scoring tail on the MI355X: the one-launch route (HipOps.box_scores through
OpenVocabBoxScores(fused=True)) against the composition of the parts that existed before it, in one process, alternating.

  composition = HipOps.roialign_fwd on boxes converted to the normalised form (on the token-major map in place, tok_off = 1)
                -> F.normalize -> matmul with all_embed * vlm_temperature -> softmax;  softmax of the detector's logits;
                det ** (1 - w) * vlm ** w                                        (fvit_head.py:68, 112-119 as torch launches)

Shapes: 8 images x 1000 boxes on a 64 x 64 map (1024-pixel images, stride 16), (E, C) = (512, 66), (512, 1204), (768, 1204).
Boxes: the size mix of RPN proposals after NMS, generated as -- side scale s log-uniform in [16, 1024] pixels, aspect ratio a log-uniform
in [1/3, 3], width s * sqrt(a), height s / sqrt(a), centre uniform on the image, clipped to the image, sides of at least one pixel;
images in mmdet's bbox2roi order (all boxes of image 0, then image 1, ...).  Seeded.

Method (measuring-on-mi355x): every shape is warmed up on both routes; a window is `--iters` calls between two device events; windows of
the two routes alternate `--windows` times and the medians are reported, with the spread (min .. max).  Outputs of the two routes are
compared first.  Bytes are what each route's launches must move by its algorithm, computed from the shapes: the map cells the boxes
touch (common to both), the class table, and every intermediate a launch writes and a later launch reads back.

Prints a markdown table and one JSON line per shape.  Needs the GPU; there is no CPU path."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FROZEN_PASS_MS = 16.1                                      # the frozen B/16 tower pass this tail follows (profiles/, README)


def rpn_like_boxes(images, per_image, size, gen):
    n = images * per_image
    s = torch.exp(torch.rand(n, generator=gen) * math.log(size / 16.0)) * 16.0
    a = torch.exp((torch.rand(n, generator=gen) * 2 - 1) * math.log(3.0))
    w, h = s * a.sqrt(), s / a.sqrt()
    cx, cy = torch.rand(n, generator=gen) * size, torch.rand(n, generator=gen) * size
    x0, y0 = (cx - w / 2).clamp(0, size - 1), (cy - h / 2).clamp(0, size - 1)
    x1, y1 = torch.minimum((cx + w / 2).clamp(0, size), x0 + w).clamp_min(x0 + 1), torch.minimum((cy + h / 2).clamp(0, size), y0 + h).clamp_min(y0 + 1)
    idx = torch.arange(images).repeat_interleave(per_image).float()
    return torch.stack([idx, x0, y0, x1, y1], dim=1).contiguous()


def touched_cells(rois, stride, grid):
    r = rois[:, 1:] / stride - 0.5
    span = lambda lo, hi: (hi.clamp(0, grid - 1).floor() + 1 - lo.clamp(0, grid - 1).floor() + 1).clamp(1, grid)
    return float((span(r[:, 0], r[:, 2]) * span(r[:, 1], r[:, 3])).sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--boxes", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--shapes", default="512x66,512x1204,768x1204", help="E x C, comma separated")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    args = ap.parse_args(argv)
    from clipself_amd.hip import HipOps
    from clipself_amd.ov_head import OpenVocabBoxScores
    ops = HipOps()
    Bn, g, stride = args.images, args.grid, args.stride
    gen = torch.Generator().manual_seed(0)
    rois = rpn_like_boxes(Bn, args.boxes, g * stride, gen)
    K = rois.shape[0]
    cells = touched_cells(rois, stride, g)
    rois_dev = rois.cuda()
    normed = rois_dev.clone()
    normed[:, 1:] /= float(g * stride)
    print(f"{Bn} images x {args.boxes} boxes, {g} x {g} map, stride {stride}; {cells / K:.0f} map cells per box; windows of {args.iters} calls, "
          f"{args.windows} alternations\n")
    print("| E | C | fused ms (min .. max) | composition ms (min .. max) | fused / composition | pooling ms: fused-form / old kernel | fused MB | composition MB "
          "| fused share of the frozen pass |")
    print("|---|---|---|---|---|---|---|---|---|")
    for shape in args.shapes.split(","):
        E, C = (int(v) for v in shape.split("x"))
        dense = F.normalize(torch.randn(Bn, g * g + 1, E, generator=gen), dim=-1).cuda()
        fmap = dense[:, 1:].reshape(Bn, g, g, E).permute(0, 3, 1, 2)                    # what forward_intermediates returns
        embed = F.normalize(torch.randn(C, E, generator=gen), dim=-1)
        det = (torch.randn(K, C, generator=gen) * 4).cuda()
        head = OpenVocabBoxScores(embed, alpha=0.2, beta=0.45, featmap_stride=stride, ops=ops, fused=True).cuda().eval()
        all_embed, w, T = head.all_embed.float(), head.exponents(), head.vlm_temperature
        pooled = torch.empty(K, E, device="cuda")

        def fused():
            return head(det, fmap, rois_dev)

        def composed():
            ops.roialign_fwd(dense, normed, pooled, g, g, 1)
            vlm = (F.normalize(pooled, dim=-1, p=2) @ all_embed * T).softmax(dim=-1)
            return det.softmax(dim=-1) ** (1 - w) * vlm ** w

        def pool_new():
            ops.roialign_fwd(dense, rois_dev, pooled, g, g, 1, box_scale=1.0 / stride)

        def pool_old():
            ops.roialign_fwd(dense, normed, pooled, g, g, 1)

        a, b = fused(), composed()
        torch.cuda.synchronize()
        rel = float(((a.double().log() - b.double().log()).abs()).max())
        assert rel < 1e-3, f"the two routes disagree: max |d log score| {rel}"

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters

        routes = {"fused": fused, "composed": composed, "pool_new": pool_new, "pool_old": pool_old}
        for fn in routes.values():
            window(fn)
        times = {k: [] for k in routes}
        for _ in range(args.windows):
            for k, fn in routes.items():
                times[k].append(window(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        MB = 1.0 / (1 << 20)
        map_bytes = cells * E * 4
        groups = (K + 15) // 16 if E + C <= 2292 else (K + 7) // 8
        fused_bytes = map_bytes + groups * C * E * 4 + 2 * K * C * 4 + K * 20                       # map, table per group, det in, scores out, boxes
        comp_bytes = (map_bytes + K * 20 + K * E * 4                                                # pool: map, boxes -> pooled
                      + 2 * K * E * 4                                                               # normalize: pooled -> unit rows
                      + K * E * 4 + C * E * 4 + K * C * 4                                           # matmul -> logits
                      + 2 * K * C * 4                                                               # * T
                      + 2 * K * C * 4 + 2 * K * C * 4                                               # the two softmaxes
                      + 2 * K * C * 4 + 2 * K * C * 4 + 3 * K * C * 4)                              # two pows, the product
        fmt = lambda k: f"{med[k]:.3f} ({min(times[k]):.3f} .. {max(times[k]):.3f})"
        print(f"| {E} | {C} | {fmt('fused')} | {fmt('composed')} | {med['fused'] / med['composed']:.2f} | {med['pool_new']:.3f} / {med['pool_old']:.3f} | "
              f"{fused_bytes * MB:.0f} | {comp_bytes * MB:.0f} | {100 * med['fused'] / FROZEN_PASS_MS:.1f} % |")
        print(json.dumps(dict(E=E, C=C, K=K, fused_ms=med["fused"], composed_ms=med["composed"], pool_new_ms=med["pool_new"], pool_old_ms=med["pool_old"],
                              fused_all=times["fused"], composed_all=times["composed"], max_dlog=rel, fused_bytes=fused_bytes, composed_bytes=comp_bytes)),
              file=sys.stderr)


if __name__ == "__main__":
    main()
