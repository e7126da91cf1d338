"""Times the detector's post-processing tail on the MI355X: csd_nms (mask, scan and top-k kernels behind HipOps.nms) and csd_delta2bbox
against the torch route of clipself_amd/det_post.py, the only other implementation on this stack.

Shapes, 8 images:
  coco   8 x 1000 boxes, C = 65,   score_thr 0.01, iou 0.4, max 100   (F-ViT/configs/ov_coco test_cfg.rcnn)
  lvis   8 x 1000 boxes, C = 1203, score_thr 1e-4, iou 0.5, max 300   (ov_lvis)
  rpn    8 x (5 levels x 2000) boxes in the group form, iou 0.7, max 1000, no score threshold   (rpn_proposal)
Boxes: the size mix of tools/ov_scores_bench.py (rpn_like_boxes), seeded; in the rpn shape consecutive runs of 2000 boxes are the levels.
Scores: softmax over C + 1 classes of seeded cosine-like logits (normal, sigma 0.12, clipped to [-1, 1]) times the detector temperature 50,
background dropped; rpn: sigmoid of seeded normal logits.  The candidate counts that result are recorded: time depends on them.

Method (measuring-on-mi355x): every shape is warmed up; a window is `--iters` calls between two device events; `--windows` windows, the
median and the spread (min .. max) are reported.  The torch route runs on the host, once per shape (`--torch-reps`), timed with the host
clock; it is a Python loop per list and per kept box and is reported for scale, not as a rival.  Kernel outputs are compared with the torch
route's on every shape it runs on.  Per-kernel times come from a kernel trace of `--trace SHAPE` (calls only, no timing) taken in a run of
its own.  Prints a markdown table and one JSON line per shape.  The kernel columns need the GPU; `--torch-only` times the torch route alone."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ov_scores_bench import rpn_like_boxes  # noqa: E402

FROZEN_PASS_MS = 16.08                                     # the frozen B/16 pass with taps, 8 images (profiles/backbone_taps_bench.md)
SHAPES = {
    "coco": dict(per_image=1000, C=65, score_thr=0.01, iou=0.4, max_num=100),
    "lvis": dict(per_image=1000, C=1203, score_thr=1e-4, iou=0.5, max_num=300),
    "rpn": dict(per_image=10000, C=1, G=5, score_thr=float("-inf"), iou=0.7, max_num=1000),
}


def make_shape(name, images, gen):
    sp = SHAPES[name]
    n = sp["per_image"]
    K = images * n
    starts = torch.arange(images + 1, dtype=torch.int32) * n
    if "G" in sp:
        per = n // sp["G"]
        boxes = rpn_like_boxes(images, n, 1024, gen)[:, 1:]
        group = torch.arange(sp["G"], dtype=torch.int32).repeat_interleave(per).repeat(images)
        scores = torch.sigmoid(torch.randn(K, 1, generator=gen) * 2)
        return boxes.contiguous(), scores, starts, group
    boxes = rpn_like_boxes(images, n, 1024, gen)[:, 1:].contiguous()
    logits = (torch.randn(K, sp["C"] + 1, generator=gen) * 0.12).clamp(-1, 1) * 50.0
    return boxes, logits.softmax(dim=-1)[:, :sp["C"]].contiguous(), starts, None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--shapes", default="coco,lvis,rpn")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--torch-reps", type=int, default=1, help="0 = skip the torch route (and the comparison)")
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--trace", default=None, help="SHAPE: 3 warm-up + `--iters` calls of that shape and nothing else (for a kernel trace)")
    args = ap.parse_args(argv)
    from clipself_amd import det_post
    ops = None
    if not args.torch_only:
        from clipself_amd.hip import HipOps
        ops = HipOps()
    print(f"{args.images} images; windows of {args.iters} calls, {args.windows} windows; torch route: {args.torch_reps} run(s) on the host\n")
    print("| shape | boxes / image | lists / image | candidates / image | kept / image (before the cut) | nms µs (min .. max) | delta2bbox µs | "
          "torch route ms | outputs bit-equal | nms share of the frozen pass |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in ([args.trace] if args.trace else args.shapes.split(",")):
        sp = SHAPES[name]
        gen = torch.Generator().manual_seed(0)
        boxes, scores, starts, group = make_shape(name, args.images, gen)
        K, C, G, n = boxes.shape[0], sp["C"], sp.get("G", 0), sp["per_image"]
        cand = int((scores > sp["score_thr"]).sum())
        res = dict(shape=name, K=K, C=C, G=G, candidates_per_image=cand / args.images)
        torch_ms, ref = float("nan"), None
        if args.torch_reps and not args.trace:
            ts = []
            for _ in range(args.torch_reps):
                t0 = time.perf_counter()
                ref = det_post.nms_torch(boxes, scores, starts, n, sp["score_thr"], sp["iou"], sp["max_num"], group, G)
                ts.append((time.perf_counter() - t0) * 1e3)
            torch_ms = statistics.median(ts)
        nms_us, d2b_us, spread, kept = float("nan"), float("nan"), "", float("nan")
        if ops is not None:
            b, s, st, g = boxes.cuda(), scores.cuda(), starts.cuda(), None if group is None else group.cuda()
            deltas = (torch.randn(K, 4, generator=gen) * 0.5).cuda()
            out4 = torch.empty(K, 4, device="cuda")
            ms = torch.tensor([[1024.0, 1024.0]] * args.images, device="cuda")
            sc = torch.tensor([[1.6, 1.6, 1.6, 1.6]] * args.images, device="cuda")

            def run_nms():
                return ops.nms(b, s, st, n, sp["score_thr"], sp["iou"], sp["max_num"], g, G)

            def run_d2b():
                return ops.delta2bbox(b, deltas, out4, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), 16 / 1000, st, ms, sc)

            got = run_nms()
            torch.cuda.synchronize()
            if args.trace:
                for _ in range(2 + args.iters):
                    run_nms()
                    run_d2b()
                torch.cuda.synchronize()
                print(f"traced {name}: {3 + args.iters} csd_nms calls")
                return
            if ref is not None:                            # the same fp32 arithmetic on both routes: every output is expected bit-equal
                res["equal_to_torch_route"] = all(torch.equal(x.cpu().view(torch.int32), y.view(torch.int32)) for x, y in zip(got, ref))
            # kept before the cut: the per-image append counter the scan kernel leaves at the head of the workspace
            ws = ops._ws[("clipself_det.h", b.device)]     # HipOps' one buffer for this header and device
            kept = float(ws[:4 * args.images].view(torch.int32).float().mean())

            def window(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.iters * 1e3

            window(run_nms), window(run_d2b)
            t_n, t_d = [], []
            for _ in range(args.windows):
                t_n.append(window(run_nms))
                t_d.append(window(run_d2b))
            nms_us, d2b_us = statistics.median(t_n), statistics.median(t_d)
            spread = f" ({min(t_n):.0f} .. {max(t_n):.0f})"
            res.update(nms_us=nms_us, nms_all=t_n, delta2bbox_us=d2b_us, kept_per_image=kept, counts=got[3].tolist())
        res.update(torch_ms=torch_ms)
        print(f"| {name} | {n} | {G or C} | {cand / args.images:.0f} | {kept:.0f} | {nms_us:.0f}{spread} | {d2b_us:.1f} | {torch_ms:.0f} | {res.get('equal_to_torch_route', 'n/a')} | "
              f"{100 * nms_us / 1e3 / FROZEN_PASS_MS:.1f} % |")
        print(json.dumps(res), file=sys.stderr)


if __name__ == "__main__":
    main()
