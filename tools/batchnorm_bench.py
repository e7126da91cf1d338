"""Times batch norm + ReLU on channel-last maps on the MI355X: norm_act.BatchNormAct2d on the HIP kernels (include/clipself_bn.h) against
torch's own F.batch_norm + F.relu on the same device and the same input, and one box-head ConvModule against Conv2d + BatchNorm2d + ReLU
in fp32 and under bf16 autocast.  The yardstick is torch's route, never the new kernels against themselves.

Shapes (N, C, H, W), training mode, channel-last inputs and upstream gradients in fp32 and in bf16:
  box     (4096, 256, 7, 7)      200 704 rows: the shared_convs of FViTBBoxHead (the mask head's 1024 x 14 x 14 has the same rows)
  rpn640  (8, 256, 160, 160)     204 800 rows: rpn_conv / fpn_convs, level 0 at 640 x 640
  rpn1024 (8, 256, 256, 256)     524 288 rows: the same at 1024 x 1024
  neck    (8, 768, 128, 128)     131 072 rows of 768 channels, fp32 only: the norm between the neck's two Deconv2x2
Each is measured forward (no graph) and forward + backward (input, weight and bias gradients).  torch's variants: F.relu out of place and
in place (mmcv's ConvModule builds ReLU(inplace=True)); the faster one is the yardstick.

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  Then every kernel alone
at every shape with the bytes it must move and the achieved bytes/s beside the 6.3 TB/s float4 stream ceiling on record in
profiles/adamw_guard_bench.md.  Prints markdown tables, one JSON line per shape on stderr, and the verdict for FUSED_BN_DEFAULT."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

STREAM_CEILING = 6.3e12
SHAPES = {"box": (4096, 256, 7, 7), "rpn640": (8, 256, 160, 160), "rpn1024": (8, 256, 256, 256), "neck": (8, 768, 128, 128)}
BF16, F32 = torch.bfloat16, torch.float32
DT = {F32: "fp32", BF16: "bf16"}


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
    ap.add_argument("--shapes", default="box,rpn640,rpn1024,neck")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args(argv)
    from clipself_amd.hip import HipOps
    from clipself_amd.norm_act import BatchNormAct2d, ConvModule
    ops = HipOps()
    print(f"windows of {args.iters} calls, {args.windows} windows, variants alternated\n")
    print("| shape | input | pass | variant | µs median (min .. max) | faster torch variant / this |")
    print("|---|---|---|---|---|---|")
    verdict, kernel_rows = {}, []
    for name in [s for s in args.shapes.split(",") if s]:
        N, C, H, W = SHAPES[name]
        M = N * H * W
        g = torch.Generator().manual_seed(0)
        x32 = (torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3).cuda().contiguous(memory_format=torch.channels_last)
        dy32 = torch.randn(N, C, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        for dtype in ((F32,) if name == "neck" else (F32, BF16)):
            x, dy = x32.to(dtype), dy32.to(dtype)
            xg = x.clone().requires_grad_(True)
            mod = BatchNormAct2d(C, act="relu", ops=ops, fused=True).cuda()
            ref = torch.nn.BatchNorm2d(C).cuda()
            fns = {"kernels": (mod, mod), "torch, F.relu": (lambda t: F.relu(ref(t)), ref), "torch, F.relu in place": (lambda t: F.relu_(ref(t)), ref)}
            with torch.no_grad():
                want = F.relu(F.batch_norm(x.double(), None, None, None, None, True)).float()
                err = {k: float((fn(x).float() - want).norm() / want.norm()) for k, (fn, _) in fns.items()}

            def fwd(fn):
                def run():
                    with torch.no_grad():
                        return fn(x)
                return run

            def fwd_bwd(fn, m):
                def run():
                    xg.grad = None
                    m.weight.grad = m.bias.grad = None
                    fn(xg).backward(dy)
                return run
            rec = dict(shape=name, dims=SHAPES[name], input=DT[dtype], rel_l2_vs_float64=err)
            for pname, variants in (("forward", {k: fwd(fn) for k, (fn, _) in fns.items()}),
                                    ("forward + backward", {k: fwd_bwd(fn, m) for k, (fn, m) in fns.items()})):
                times = measure(variants, args.iters, args.windows)
                med = {k: statistics.median(v) for k, v in times.items()}
                best_torch = min(v for k, v in med.items() if k != "kernels")
                for k in variants:
                    print(f"| {name} {M} x {C} | {DT[dtype]} | {pname} | {k} | {fmt(times[k])} | {best_torch / med[k]:.2f} x |")
                rec[pname] = dict(median_us=med, all_us=times)
                if pname != "forward":
                    verdict[f"{name} {DT[dtype]}"] = med["kernels"] < best_torch
            print(json.dumps(rec), file=sys.stderr)
            # every kernel alone
            X, dY = (t.permute(0, 2, 3, 1).reshape(M, C) for t in (x, dy))
            Y, dX = torch.empty_like(X), torch.empty_like(X)
            recd, st, sums = (torch.empty(n, device="cuda") for n in (2 * C + 4, 4 * C + 4, 2 * C))
            gamma, beta = mod.weight.detach(), mod.bias.detach()
            ops.bn_stats(X, recd)
            ops.bn_finalize(recd, C, gamma, beta, 1e-5, 0.1, None, None, st)
            es = X.element_size()
            alone = {"csb_stats": (lambda: ops.bn_stats(X, recd), 1), "csb_finalize": (lambda: ops.bn_finalize(recd, C, gamma, beta, 1e-5, 0.1, None, None, st), 0),
                     "csb_apply": (lambda: ops.bn_apply(X, st, 1, Y), 2), "csb_bwd_reduce": (lambda: ops.bn_bwd_reduce(dY, X, st, 1, sums), 2),
                     "csb_bwd_apply": (lambda: ops.bn_bwd_apply(dY, X, st, 1, sums, gamma, dX), 3)}
            times = measure({k: fn for k, (fn, _) in alone.items()}, args.iters, args.windows)
            for k, (_, passes) in alone.items():
                kernel_rows.append((name, M, C, DT[dtype], k, times[k], passes * M * C * es))
            del x, dy, xg, X, dY, Y, dX, mod, ref
            torch.cuda.empty_cache()
        del x32, dy32
        torch.cuda.empty_cache()

    print("\nevery kernel alone (csb_stats and csb_bwd_reduce include their second, combining launch)\n")
    print("| shape | map | kernel | µs median (min .. max) | bytes the kernel must move | achieved | share of the 6.3 TB/s stream ceiling |")
    print("|---|---|---|---|---|---|---|")
    for name, M, C, dt, k, v, nbytes in kernel_rows:
        med = statistics.median(v)
        if nbytes:
            rate = nbytes / med * 1e6
            print(f"| {name} {M} x {C} | {dt} | {k} | {fmt(v)} | {nbytes / 1e6:.0f} MB | {rate / 1e12:.2f} TB/s | {100 * rate / STREAM_CEILING:.0f} % |")
        else:
            print(f"| {name} {M} x {C} | {dt} | {k} | {fmt(v)} | | | |")

    # one box-head ConvModule, forward + backward, against torch's Conv2d + BatchNorm2d + ReLU in fp32 and under bf16 autocast
    N, C, H, W = SHAPES["box"]
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, C, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(N, C, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    xg = x.clone().requires_grad_(True)
    cm = ConvModule(C, C, ops=ops, fused=True).cuda()
    cm_torch_norm = ConvModule(C, C, ops=ops, fused=True).cuda()
    cm_torch_norm.bn.fused = False
    ref = torch.nn.Sequential(torch.nn.Conv2d(C, C, 3, padding=1, bias=False), torch.nn.BatchNorm2d(C), torch.nn.ReLU(inplace=True)).cuda()
    ref = ref.to(memory_format=torch.channels_last)

    def autocast(t):
        with torch.autocast("cuda", dtype=BF16):
            return ref(t)

    def step(fn, m):
        def run():
            xg.grad = None
            for p in m.parameters():
                p.grad = None
            y = fn(xg)
            y.backward(dy.to(y.dtype))
        return run
    variants = {"ConvModule: Conv3x3 + kernels' norm": step(cm, cm), "ConvModule: Conv3x3 + torch's norm": step(cm_torch_norm, cm_torch_norm),
                "torch fp32": step(ref, ref), "torch bf16 autocast": step(autocast, ref)}
    times = measure(variants, args.iters, args.windows)
    med = {k: statistics.median(v) for k, v in times.items()}
    best_torch = min(med["torch fp32"], med["torch bf16 autocast"])
    print(f"\none box-head ConvModule {SHAPES['box']}, forward + backward, channel-last fp32 input\n")
    print("| variant | µs median (min .. max) | faster torch variant / this |\n|---|---|---|")
    for k, v in times.items():
        print(f"| {k} | {fmt(v)} | {best_torch / med[k]:.2f} x |")
    print(f"\nkernel route wins forward + backward at: {verdict}  ->  FUSED_BN_DEFAULT = {bool(verdict) and all(verdict.values())}")


if __name__ == "__main__":
    main()
