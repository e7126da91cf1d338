"""Times the box head's first FC, Linear(C * 49, out) + ReLU on the RoI map, on the MI355X: linear.LinearAct(spatial=(256, 49), act="relu")
on cs_gemm_nt's ReLU epilogue, with the deterministic split-K swept over `splits` in {1, 2, 4, 8, automatic}, against torch's own
F.relu(nn.Linear(x.flatten(1))) on the same input, in fp32 and under bf16 autocast.  The yardstick is torch's route, never the new
kernels against themselves; torch's side includes the copy its flatten makes of a channel-last map.

Shapes (rows, in, out), channel-last bf16 maps [rows, 256, 7, 7] (what a ConvModule on bf16 rows hands on):
  train  (4096, 12544, 512)    FViTBBoxHead.shared_fcs[0] on 8 x 512 sampled RoIs
  infer  (8000, 12544, 512)    the same on 8 x 1000 proposals
  fc2    (4096, 512, 512)      shared_fcs[1], cls_fcs[0], reg_fcs[0] (rows [4096, 512], no map)
  l14    (4096, 12544, 768)    the ViT-L/14 configs' fc_out_channels
Each is measured forward (no graph) and forward + backward (input, weight and bias gradients, upstream gradient in the output's dtype).
Then the whole bbox_head.ConvFCBBoxHead (4 shared convs, 2 shared FCs, 1 + 1 branch FCs, fc_reg) forward + backward at 8 x 512 RoIs:
all kernels, the kernels with torch's FCs, and all torch (fused=False).

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  Prints markdown tables
and the two verdicts the defaults rest on: FUSED_FC_DEFAULT (the kernel route wins forward + backward against the faster torch variant
at the training shape) and whether the automatic `splits` is no slower than splits=1 at any shape beyond the window-to-window spread."""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_BF16 = 2.5e15
SHAPES = {"train": (4096, 12544, 512), "infer": (8000, 12544, 512), "fc2": (4096, 512, 512), "l14": (4096, 12544, 768)}
SPLITS = (1, 2, 4, 8, None)
BF16, F32 = torch.bfloat16, torch.float32


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def measure(variants, iters, windows):
    for fn in variants.values():
        window(fn, max(2, iters // 2))
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return times


def fmt(v):
    return f"{statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f})"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="train,infer,fc2,l14")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--no-head", action="store_true")
    args = ap.parse_args(argv)
    from clipself_amd.bbox_head import ConvFCBBoxHead
    from clipself_amd.hip import HipOps
    from clipself_amd.linear import LinearAct
    ops = HipOps()
    print(f"windows of {args.iters} calls, {args.windows} windows, variants alternated; {ops.num_cus} compute units\n")
    print("| shape | pass | variant | µs median (min .. max) | faster torch variant / this | TFLOP/s | share of bf16 MFMA peak |")
    print("|---|---|---|---|---|---|---|")
    wins, auto_ok = {}, {}
    for name in [s for s in args.shapes.split(",") if s]:
        rows, inf, out = SHAPES[name]
        spatial = (256, 49) if inf == 256 * 49 else None
        g = torch.Generator().manual_seed(0)
        if spatial:
            x = torch.randn(rows, 256, 7, 7, generator=g).to(BF16).cuda().contiguous(memory_format=torch.channels_last)
        else:
            x = torch.randn(rows, inf, generator=g).to(BF16).cuda()
        dy = torch.randn(rows, out, generator=g).cuda()
        dys = {F32: dy, BF16: dy.to(BF16)}
        ref = torch.nn.Linear(inf, out).cuda()
        mods = {}
        for s in SPLITS:
            m = mods[s] = LinearAct(inf, out, act="relu", spatial=spatial, ops=ops, fused=True, splits=s).cuda()
            m.load_state_dict(ref.state_dict(), strict=True)
        chosen = ops.gemm_nt_splits(rows, out, inf)
        xg = x.clone().requires_grad_(True)

        def torch_fp32(inp):
            return F.relu(ref(inp.flatten(1).float() if spatial else inp.float()))

        def torch_autocast(inp):
            with torch.autocast("cuda", dtype=BF16):
                return F.relu(ref(inp.flatten(1) if spatial else inp))

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(x)
            return run

        def fwd_bwd(fn, params):
            def run():
                xg.grad = None
                for p in params:
                    p.grad = None
                y = fn(xg)
                y.backward(dys[y.dtype])
            return run
        label = lambda s: f"kernels, splits={'automatic (%d)' % chosen if s is None else s}"
        fns = {label(s): (mods[s], list(mods[s].parameters())) for s in SPLITS}
        fns["torch fp32"] = (torch_fp32, list(ref.parameters()))
        fns["torch bf16 autocast"] = (torch_autocast, list(ref.parameters()))
        flops_f = 2.0 * rows * inf * out
        for pname, variants, flops in (("forward", {k: fwd(fn) for k, (fn, _) in fns.items()}, flops_f),
                                       ("forward + backward", {k: fwd_bwd(fn, ps) for k, (fn, ps) in fns.items()
                                                               if "splits=2" not in k and "splits=4" not in k and "splits=8" not in k},
                                        3 * flops_f)):
            times = measure(variants, args.iters, args.windows)
            med = {k: statistics.median(v) for k, v in times.items()}
            best_torch = min(med["torch fp32"], med["torch bf16 autocast"])
            for k in variants:
                tf = flops / med[k] / 1e6
                print(f"| {name} {SHAPES[name]} | {pname} | {k} | {fmt(times[k])} | {best_torch / med[k]:.2f} x | {tf:.0f} | "
                      f"{100 * tf * 1e12 / PEAK_BF16:.1f} % |")
            if pname == "forward":
                t1, ta = times[label(1)], times[label(None)]
                # "no slower beyond the spread": the automatic median is below the slowest window of splits=1
                auto_ok[name] = statistics.median(ta) <= max(max(t1), statistics.median(t1) * 1.02)
            else:
                wins[name] = med[label(None)] < best_torch
        del x, dy, xg, mods, ref
        torch.cuda.empty_cache()

    if not args.no_head:
        cfg = dict(in_channels=256, fc_out_channels=512, roi_feat_size=7, num_classes=1203, reg_class_agnostic=True,
                   norm_cfg=dict(type="SyncBN"), num_shared_convs=4, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1)
        torch.manual_seed(0)
        heads = {"all kernels": ConvFCBBoxHead(ops=ops, fused=True, **cfg).cuda(),
                 "kernels, torch FCs": ConvFCBBoxHead(ops=ops, fused=True, **cfg).cuda(),
                 "all torch (fused=False)": ConvFCBBoxHead(ops=ops, fused=False, **cfg).cuda()}
        for h in heads.values():
            h.load_state_dict(heads["all kernels"].state_dict(), strict=True)
        h = heads["kernels, torch FCs"]
        for m in list(h.shared_fcs) + list(h.cls_fcs) + list(h.reg_fcs):
            m.fused = False
        x = torch.randn(4096, 256, 7, 7, generator=torch.Generator().manual_seed(1)).cuda().contiguous(memory_format=torch.channels_last)
        xg = x.clone().requires_grad_(True)

        def step(h):
            def run():
                xg.grad = None
                for p in h.parameters():
                    p.grad = None
                x_cls, bbox_pred = h(xg)
                (x_cls.sum() + bbox_pred.sum()).backward()
            return run
        times = measure({k: step(h) for k, h in heads.items()}, max(2, args.iters // 3), max(3, args.windows // 2))
        print("\nConvFCBBoxHead forward + backward, 8 x 512 RoIs [4096, 256, 7, 7] fp32 channel-last\n")
        print("| variant | µs median (min .. max) | all torch / this |\n|---|---|---|")
        base = statistics.median(times["all torch (fused=False)"])
        for k, v in times.items():
            print(f"| {k} | {fmt(v)} | {base / statistics.median(v):.2f} x |")
    print(f"\nkernel route wins forward + backward at: {wins}  ->  FUSED_FC_DEFAULT = {bool(wins.get('train'))}")
    print(f"automatic splits no slower than splits=1 (forward) at: {auto_ok}")


if __name__ == "__main__":
    main()
