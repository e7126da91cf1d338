"""Times the detector's RoI extractor on the MI355X: csr_roi_extract_fwd / csr_roi_extract_bwd (HipOps.roi_extract_*) on the configs' own
shapes, against the traffic floor and against the torch route of clipself_amd/roi_extractor.py, the only other implementation here.

Shapes, 8 images, C = 256, four levels:
  test    8 x 1000 boxes, P = 7,  1024 x 1024 image at strides 4 .. 32      (test_cfg.rcnn: 1000 proposals per image)
  train   8 x 512 boxes,  P = 7,  the same maps, forward + backward         (train_cfg.rcnn sampler: 512 per image)
  mask    8 x 100 boxes,  P = 14, the same maps                             (the OV-LVIS mask head's extractor)
  l14     8 x 1000 boxes, P = 7,  896 x 896 image at strides 3.5 .. 28      (the L/14 towers)
Boxes: the size mix of tools/ov_scores_bench.py (rpn_like_boxes), seeded.  Maps and upstream gradients: seeded normal.

Method (measuring-on-mi355x): every shape is warmed up; a window is `--iters` calls between two device events; the variants (forward,
backward, the NCHW -> channel-last copy of the pyramid) are interleaved window by window; `--windows` windows, median and spread.
Traffic floor: forward = the distinct map cells the boxes' samples can touch (union of the boxes' cell rectangles per level and image)
times C * 4 bytes, plus the K * P * P * C * 4 byte write; backward = the read of dout plus a read-modify-write of the same cells.
It is divided by the 6.3 TB/s float4 stream rate this project measured (profiles/adamw_guard_bench.md) and by the measured time.
The torch route runs on the host on the first `--torch-boxes` boxes of the same inputs (a Python loop per box: reported per box, for
scale, not as a rival); the kernels' output on those boxes is compared with it.  Prints a markdown table and one JSON line per shape."""
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
STREAM_BYTES_PER_S = 6.3e12                                # profiles/adamw_guard_bench.md: the float4 stream ceiling
SHAPES = {
    "test": dict(per_image=1000, P=7, image=1024, strides=[4, 8, 16, 32]),
    "train": dict(per_image=512, P=7, image=1024, strides=[4, 8, 16, 32]),
    "mask": dict(per_image=100, P=14, image=1024, strides=[4, 8, 16, 32]),
    "l14": dict(per_image=1000, P=7, image=896, strides=[3.5, 7, 14, 28]),
}


def touched_cells(rois, levels, strides, grids, images):
    """Distinct cells per level that a box's samples can touch: the union of the boxes' cell rectangles."""
    total = 0
    for l, (s, g) in enumerate(zip(strides, grids)):
        mask = torch.zeros(images, g, g, dtype=torch.bool)
        for r in rois[levels == l].tolist():
            lo = lambda v: int(min(max(v / s - 0.5, 0), g - 1))
            mask[int(r[0]), lo(r[2]):lo(r[4]) + 2, lo(r[1]):lo(r[3]) + 2] = True
        total += int(mask.sum())
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--shapes", default="test,train,mask,l14")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--torch-boxes", type=int, default=200, help="0 = skip the torch route (and the comparison)")
    args = ap.parse_args(argv)
    from clipself_amd import roi_extractor
    from clipself_amd.hip import HipOps
    ops = HipOps()
    B, C = args.images, args.channels
    print(f"{B} images, C = {C}; windows of {args.iters} calls, {args.windows} windows, variants interleaved; torch route on {args.torch_boxes} boxes\n")
    print("| shape | boxes | P | forward µs (min .. max) | floor MB | of stream rate | backward µs (min .. max) | floor MB | of stream rate | "
          "NCHW -> channel-last copy µs | torch route ms / box (fwd) | max abs diff | forward share of the frozen pass |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in args.shapes.split(","):
        sp = SHAPES[name]
        gen = torch.Generator().manual_seed(0)
        P, strides = sp["P"], sp["strides"]
        grids = [int(round(sp["image"] / s)) for s in strides]
        rois = rpn_like_boxes(B, sp["per_image"], sp["image"], gen)
        rois = rois[torch.randperm(rois.shape[0], generator=gen)].contiguous()
        K = rois.shape[0]
        levels = roi_extractor.map_roi_levels_torch(rois, len(strides), 56)
        cells = touched_cells(rois, levels, strides, grids, B)
        fwd_bytes = (cells * C + K * P * P * C) * 4
        bwd_bytes = (2 * cells * C + K * P * P * C) * 4
        nchw = [torch.randn(B, C, g, g, generator=gen).cuda() for g in grids]
        maps = [f.contiguous(memory_format=torch.channels_last) for f in nchw]
        rows = [m.permute(0, 2, 3, 1).reshape(-1, C) for m in maps]
        scales = [1.0 / s for s in strides]
        gg = [(g, g) for g in grids]
        r = rois.cuda()
        out = torch.empty(K * P * P, C, device="cuda")
        dout = torch.randn(K * P * P, C, generator=gen).cuda()
        dmaps = [torch.zeros_like(m) for m in rows]

        run_f = lambda: ops.roi_extract_fwd(rows, gg, scales, r, out, B, P, 0, 56.0)
        run_b = lambda: ops.roi_extract_bwd(dout, r, dmaps, gg, scales, B, P, 0, 56.0)
        run_c = lambda: [f.contiguous(memory_format=torch.channels_last) for f in nchw]

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters * 1e3

        for fn in (run_f, run_b, run_c):
            window(fn)
        t = {"f": [], "b": [], "c": []}
        for _ in range(args.windows):
            t["f"].append(window(run_f))
            t["b"].append(window(run_b))
            t["c"].append(window(run_c))
        med = {k: statistics.median(v) for k, v in t.items()}
        torch_ms, diff = float("nan"), float("nan")
        if args.torch_boxes:
            n = min(args.torch_boxes, K)
            cpu = [f.cpu() for f in nchw]
            t0 = time.perf_counter()
            ref = roi_extractor.roi_extract_torch(cpu, rois[:n], P, 0, strides, 56)
            torch_ms = (time.perf_counter() - t0) * 1e3 / n
            run_f()
            torch.cuda.synchronize()
            diff = float((out.view(K, P, P, C)[:n].permute(0, 3, 1, 2).cpu() - ref).abs().max())
        frac = lambda nbytes, us: 100 * nbytes / STREAM_BYTES_PER_S / (us * 1e-6)
        spread = lambda v: f"{statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f})"
        print(f"| {name} | {B} x {sp['per_image']} | {P} | {spread(t['f'])} | {fwd_bytes / 1e6:.0f} | {frac(fwd_bytes, med['f']):.0f} % | {spread(t['b'])} | "
              f"{bwd_bytes / 1e6:.0f} | {frac(bwd_bytes, med['b']):.0f} % | {spread(t['c'])} | {torch_ms:.2f} | {diff:.2e} | "
              f"{100 * med['f'] / 1e3 / FROZEN_PASS_MS:.1f} % |")
        print(json.dumps(dict(shape=name, K=K, P=P, C=C, grids=grids, boxes_per_level=[int((levels == l).sum()) for l in range(len(strides))],
                              touched_cells=cells, fwd_us=med["f"], bwd_us=med["b"], copy_us=med["c"], fwd_all=t["f"], bwd_all=t["b"],
                              fwd_floor_bytes=fwd_bytes, bwd_floor_bytes=bwd_bytes, torch_ms_per_box=torch_ms, max_abs_diff=diff)), file=sys.stderr)
        del nchw, maps, rows, dmaps, out, dout
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
