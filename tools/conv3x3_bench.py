"""Times Conv2d(256, 256, 3, padding=1) of the detector heads on the MI355X: conv.Conv3x3 on the implicit kernel (csc_conv3x3) and on the
im2col route (csc_im2col3x3 + cs_gemm_nt) against torch's own F.conv2d on the same device, in fp32 and under bf16 autocast.  The yardstick
is torch's route, never the new kernels against themselves.

Shapes (N, C, H, W), channel-last fp32 inputs (what SingleRoIExtractor and the FPN hand on), Cin = Cout = 256:
  box    (4096, 256, 7, 7)       the four shared_convs of FViTBBoxHead on 8 x 512 RoI tiles
  mask   (1024, 256, 14, 14)     the four convolutions of FCNMaskHead
  rpn640 (8, 256, 160, 160)      RPNHead / fpn_convs, level 0 at 640 x 640
  rpn1024 (8, 256, 256, 256)     the same at 1024 x 1024
Each is measured forward (no graph) and forward + backward (input, weight and bias gradients, upstream gradient channel-last fp32).

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  Prints a markdown table,
the achieved share of the 2.5 PFLOP/s bf16 MFMA peak of the implicit kernel beside that of cs_gemm_nt on the explicit matrix
(M = 200 704, N = 256, K = 2304; bf16 operands and output: the difference is what the gather costs), the launches of one backward at
the box head's shape each timed alone, and one JSON line per shape."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_BF16 = 2.5e15
SHAPES = {"box": (4096, 256, 7, 7), "mask": (1024, 256, 14, 14), "rpn640": (8, 256, 160, 160), "rpn1024": (8, 256, 256, 256)}
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="box,mask,rpn640,rpn1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args(argv)
    from clipself_amd.conv import Conv3x3, pack_weights
    from clipself_amd.hip import HipOps
    ops = HipOps()
    print(f"windows of {args.iters} calls, {args.windows} windows, variants alternated\n")
    print("| shape | pass | variant | µs median (min .. max) | faster torch variant / this | TFLOP/s | share of bf16 MFMA peak |")
    print("|---|---|---|---|---|---|---|")
    verdict = {}
    for name in [s for s in args.shapes.split(",") if s]:
        N, C, H, W = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        x = torch.randn(N, C, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        dy = torch.randn(N, C, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        dys = {F32: dy, BF16: dy.to(BF16)}                 # the upstream gradient in the output's dtype, made once
        mods = {r: Conv3x3(C, C, ops=ops, fused=True, route=r).cuda() for r in ("implicit", "im2col")}
        ref = torch.nn.Conv2d(C, C, 3, padding=1).cuda().to(memory_format=torch.channels_last)
        for m in mods.values():
            m.load_state_dict(ref.state_dict(), strict=True)
        xg = x.clone().requires_grad_(True)

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

        def autocast(inp):
            with torch.autocast("cuda", dtype=BF16):
                return ref(inp)
        fns = {"implicit kernel": (mods["implicit"], list(mods["implicit"].parameters())),
               "im2col + cs_gemm_nt": (mods["im2col"], list(mods["im2col"].parameters())),
               "torch fp32": (ref, list(ref.parameters())), "torch bf16 autocast": (autocast, list(ref.parameters()))}
        with torch.no_grad():
            y_ref = ref(x).double()
            err = {k: float((fn(x).double() - y_ref).norm() / y_ref.norm()) for k, (fn, _) in fns.items()}
        flops_f = 2.0 * N * H * W * C * 9 * C
        rec = dict(shape=name, dims=SHAPES[name], rel_l2_vs_torch_fp32=err)
        for pname, variants, flops in (("forward", {k: fwd(fn) for k, (fn, _) in fns.items()}, flops_f),
                                       ("forward + backward", {k: fwd_bwd(fn, ps) for k, (fn, ps) in fns.items()}, 3 * flops_f)):
            times = measure(variants, args.iters, args.windows)
            med = {k: statistics.median(v) for k, v in times.items()}
            best_torch = min(med["torch fp32"], med["torch bf16 autocast"])
            for k in variants:
                tf = flops / med[k] / 1e6
                print(f"| {name} {SHAPES[name]} | {pname} | {k} | {med[k]:.0f} ({min(times[k]):.0f} .. {max(times[k]):.0f}) | "
                      f"{best_torch / med[k]:.2f} x | {tf:.0f} | {100 * tf * 1e12 / PEAK_BF16:.1f} % |")
            rec[pname] = dict(median_us=med, all_us=times)
            if pname != "forward":
                verdict[name] = min(med["implicit kernel"], med["im2col + cs_gemm_nt"]) < best_torch
        print(json.dumps(rec), file=sys.stderr)
        del x, dy, xg, mods, ref
        torch.cuda.empty_cache()

    # what the gather costs: the implicit kernel on the box head's bf16 rows against cs_gemm_nt on the explicit matrix of the same problem
    N, C, H, W = SHAPES["box"]
    M, K = N * H * W, 9 * C
    g = torch.Generator().manual_seed(1)
    X = torch.randn(M, C, generator=g).to(BF16).cuda()
    Wg = pack_weights(torch.randn(C, C, 3, 3, generator=g) * K ** -0.5)[0].cuda()
    bias = torch.randn(C, generator=g).cuda()
    cols = torch.empty(M, K, dtype=BF16, device="cuda")
    ops.im2col3x3(X, cols, N, H, W)
    Y = torch.empty(M, C, dtype=BF16, device="cuda")
    variants = {"csc_conv3x3 (implicit, bf16 in / out)": lambda: ops.conv3x3(X, Wg, Y, bias, N, H, W),
                "cs_gemm_nt on the explicit matrix": lambda: ops.gemm_nt(cols, Wg, Y, bias, epi=0),
                "csc_im2col3x3 alone": lambda: ops.im2col3x3(X, cols, N, H, W)}
    times = measure(variants, args.iters, args.windows)
    print(f"\nM = {M}, N = {C}, K = {K} ({2.0 * M * C * K / 1e9:.0f} GFLOP), bf16 operands and output\n")
    print("| kernel | µs median (min .. max) | TFLOP/s | share of the 2.5 PFLOP/s bf16 MFMA peak |")
    print("|---|---|---|---|")
    for k, v in times.items():
        med = statistics.median(v)
        tf = 2.0 * M * C * K / med / 1e6
        gemm = "im2col" not in k
        print(f"| {k} | {med:.0f} ({min(v):.0f} .. {max(v):.0f}) | {tf:.0f} | {100 * tf * 1e12 / PEAK_BF16:.1f} % |" if gemm else
              f"| {k} | {med:.0f} ({min(v):.0f} .. {max(v):.0f}) | {M * K * 2 / med / 1e6:.2f} TB/s written | |")
    # the launches of one backward on the implicit route at the box head's shape (fp32 upstream gradient, fp32 dx), each timed alone
    from clipself_amd.det_layer import row_chunks
    dY32 = torch.randn(M, C, generator=g).cuda()
    dY, dX, dWg, db = torch.empty(M, C, dtype=BF16, device="cuda"), torch.empty(M, C, device="cuda"), torch.zeros(C, K, device="cuda"), torch.zeros(C, device="cuda")
    chunks = row_chunks(M, K * 2)
    ws = torch.empty(max(ops.gemm_wgrad_tn_workspace(C, K, n) for _, n in chunks), dtype=torch.uint8, device="cuda")

    def im2col_chunks():
        for r0, n in chunks:
            ops.im2col3x3(X, cols[:n], N, H, W, r0)

    def wgrad_chunks():
        for r0, n in chunks:
            ops.gemm_wgrad_tn(dY[r0:r0 + n], cols[:n], dWg, ws)
    pieces = {"cs_cast_f32_bf16 of dY": lambda: ops.cast_f32_bf16(dY32, dY),
              "csc_conv3x3 (dgrad, fp32 out)": lambda: ops.conv3x3(dY, Wg, dX, None, N, H, W),
              f"csc_im2col3x3, {len(chunks)} chunks": im2col_chunks, f"cs_gemm_wgrad_tn, {len(chunks)} chunks": wgrad_chunks,
              "cs_colsum_bf16 of dY": lambda: ops.colsum_bf16(dY, db)}
    times = measure(pieces, args.iters, args.windows)
    print(f"\nthe launches of one backward at the box head's shape, each alone\n\n| launch | µs median (min .. max) |\n|---|---|")
    for k, v in times.items():
        print(f"| {k} | {statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f}) |")
    print(f"| sum | {sum(statistics.median(v) for v in times.values()):.0f} |")
    print(f"\nkernel route wins forward + backward at: {verdict}  ->  FUSED_CONV_DEFAULT = {bool(verdict) and all(verdict.values())}")


if __name__ == "__main__":
    main()
