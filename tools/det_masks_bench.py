"""Times the detector's mask branch on the MI355X: csm_mask_target, csm_mask_loss and csm_paste_masks (HipOps.mask_target / mask_loss /
paste_masks, clipself_amd/det_masks.py) against the torch route of the same module on the same device (`fused=False`: the same contract
in plain fp32 torch, in chunks of 32 rows), and the paste also against a plain zero fill of its output (`Tensor.zero_()`), which is the
write bandwidth the kernel can at best reach.

Shapes:
  target    8 images x 128 mask slots, 64 ground truths per image, 1024^2 uint8 masks (512 MB on the device), M = 28; boxes of 16 .. 640 px
  loss      the same 1024 rows, C = 1, M = 28: forward + backward through the autograd Function, non-unit upstream gradient
  paste100  100 detections pasted into a 1024^2 image, C = 1, M = 28, thr = 0.5
  paste300  300 detections

Method: every variant is warmed up; a window is `--iters` calls between two device events; `--windows` windows per variant, the variants
alternated window by window in one process; the median and the spread (min .. max) are reported.  Prints a markdown table and one JSON
line per shape."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BACKBONE_FWD_BWD_MS = 22.0                                 # the B/16 backbone forward + backward, 8 images (profiles/neck_bench.md)


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


def random_boxes(n, side, gen, smin=16.0, smax=640.0):
    w = smin * (smax / smin) ** torch.rand(n, generator=gen)
    h = smin * (smax / smin) ** torch.rand(n, generator=gen)
    x0, y0 = torch.rand(n, generator=gen) * (side - w), torch.rand(n, generator=gen) * (side - h)
    return torch.stack([x0, y0, x0 + w, y0 + h], dim=1)


def target_shape(B, ops, gen, side=1024, slots=128, gts=64, M=28):
    from clipself_amd import det_masks as DM
    R, G = B * slots, B * gts
    masks = torch.zeros(G, side, side, dtype=torch.uint8, device="cuda")
    gb = random_boxes(G, side, gen).round().long()
    yy = torch.arange(side, device="cuda")[:, None]
    xx = torch.arange(side, device="cuda")[None, :]
    for g in range(G):                                        # an ellipse inside each ground-truth box
        x0, y0, x1, y1 = (int(v) for v in gb[g])
        cy, cx, ry, rx = (y0 + y1) / 2, (x0 + x1) / 2, max((y1 - y0) / 2, 1), max((x1 - x0) / 2, 1)
        masks[g] = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1).to(torch.uint8)
    rows = (torch.arange(R) // slots * gts + torch.randint(0, gts, (R,), generator=gen)).to(torch.int32)
    jit = gb[rows.long()].float() + torch.randn(R, 4, generator=gen) * 6.0      # proposals around their ground truth
    boxes = torch.stack([jit[:, 0], jit[:, 1], torch.maximum(jit[:, 2], jit[:, 0] + 4), torch.maximum(jit[:, 3], jit[:, 1] + 4)], dim=1)
    rois = torch.cat([(torch.arange(R) // slots).float()[:, None], boxes], dim=1).cuda().contiguous()
    rows = rows.cuda()
    out = torch.empty(R, M, M, dtype=torch.uint8, device="cuda")

    def kernel():
        ops.mask_target(rois, rows, masks, M, out=out)

    def torch_route():
        DM.mask_target(rois, rows, masks, M, fused=False)

    return dict(kernel=kernel, torch=torch_route), R, (rois, rows, masks)


def loss_shape(data, ops, gen, M=28):
    from clipself_amd import det_masks as DM
    rois, rows, masks = data
    R = rois.shape[0]
    targets = ops.mask_target(rois, rows, masks, M)
    pred = (torch.randn(R, 1, M, M, generator=gen) * 2).cuda().requires_grad_()
    w = torch.ones(R, device="cuda")
    w[::7] = 0

    def run(fused):
        pred.grad = None
        out = DM.mask_loss(pred, targets, None, w, ops=ops, fused=fused)
        (out["loss_mask"] * 0.7).backward()

    def k_call():
        ops.mask_loss(pred.detach(), None, targets, w)

    return dict(kernel=lambda: run(True), kernel_one_call=k_call, torch=lambda: run(False)), R


def paste_shape(N, ops, gen, side=1024, M=28):
    from clipself_amd import det_masks as DM
    logits = (torch.randn(N, 1, M, M, generator=gen) * 2).cuda()
    boxes = random_boxes(N, side, gen).cuda().contiguous()
    out = torch.empty(N, side, side, dtype=torch.uint8, device="cuda")

    def kernel():
        ops.paste_masks(logits, None, boxes, side, side, 0.5, out=out)

    def torch_route():
        DM.paste_masks(logits, boxes, None, (side, side), fused=False)

    return dict(kernel=kernel, torch=torch_route, zero_fill=lambda: out.zero_()), N


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--shapes", default="target,loss,paste100,paste300")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args(argv)

    from clipself_amd.hip import HipOps
    ops = HipOps()
    gen = torch.Generator().manual_seed(0)
    rows, data = [], None
    for name in args.shapes.split(","):
        if name in ("target", "loss"):
            if data is None:
                tv, n, data = target_shape(args.images, ops, gen)
            variants, n = (tv, n) if name == "target" else loss_shape(data, ops, gen)
        else:
            data = tv = None
            torch.cuda.empty_cache()
            variants, n = paste_shape(int(name[5:]), ops, gen)
        res = alternate(variants, args.iters, args.windows)
        rows.append((name, n, res))
        print(json.dumps(dict(shape=name, rows=n, **{k + "_ms": dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4))
                                                     for k, v in res.items()})), flush=True)
    print("\n| shape | rows | kernel ms (min .. max) | torch route ms (min .. max) | torch / kernel | kernel of the 22 ms backbone fwd + bwd | "
          "zero fill ms | zero fill / kernel |")
    print("|---|---|---|---|---|---|---|---|")
    for name, n, r in rows:
        k, t = r["kernel"], r["torch"]
        z = r.get("zero_fill")
        print(f"| {name} | {n} | {k[0]:.3f} ({k[1]:.3f} .. {k[2]:.3f}) | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {t[0] / k[0]:.1f} x | "
              f"{100 * k[0] / BACKBONE_FWD_BWD_MS:.1f} % | {'' if z is None else f'{z[0]:.3f}'} | {'' if z is None else f'{100 * z[0] / k[0]:.0f} %'} |")


if __name__ == "__main__":
    main()
