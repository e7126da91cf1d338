"""Detector-backbone pass on the MI355X: the token-taps kernel against the torch expression it replaces, and the whole frozen pass.

    python tools/backbone_bench.py [--out profiles/backbone_taps_bench.md] [--batch 8] [--reps 15]

Workloads: the shipped F-ViT detector configs -- EVA02-CLIP-B-16 at 1024 x 1024, out_indices [3, 5, 7, 11], and EVA02-CLIP-L-14-336 at
896 x 896, out_indices [6, 10, 14, 23]; 8 images per GPU; 64 x 64 = 4096 patch tokens + CLS either way.  Seeded weights (timings do not
depend on the values).

Per tap: HipOps.tokens_to_nchw (fp32 and bf16 output) and x.view(B, N, C)[:, 1:].permute(0, 2, 1).contiguous() on the same stream tensor,
alternated window by window in one process (device events around `--inner` launches each, the median over `--reps` windows), outputs
compared bit for bit first.  Bytes = what the copy must move (read B*h*w*C fp32, write the same count in the output type); the ceiling is
the measured float4-copy rate of the part, 6.29 TB/s.
Whole pass: EVAVisionTower.forward_intermediates (taps + map) against the same pass without taps, images per second, and the taps' share.
Needs the GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

STREAM_CEILING = 6.29e12                   # bytes / s, measured float4 copy on the MI355X (8.0 TB/s by specification)
WORKLOADS = [("EVA02-CLIP-B-16", 1024, [3, 5, 7, 11]), ("EVA02-CLIP-L-14-336", 896, [6, 10, 14, 23])]


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def alternate(fns, reps, inner):
    """Median seconds per call of each fn, windows alternated fn by fn."""
    for fn in fns:
        window(fn, 3)
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            t.append(window(fn, inner))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "backbone_taps_bench.md"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--pass-reps", type=int, default=12)
    ap.add_argument("--pass-inner", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("backbone_bench needs the GPU: nothing here can be measured on a CPU")
    from clipself_amd.open_clip import create_model
    lines = ["# Detector backbone: token taps and the whole frozen pass", "",
             f"`python tools/backbone_bench.py --batch {args.batch} --reps {args.reps} --inner {args.inner}` on {torch.cuda.get_device_name(0)}; "
             f"medians over {args.reps} windows of {args.inner} launches, kernel and torch expression alternated window by window "
             f"(min - max in brackets).  Ceiling: {STREAM_CEILING / 1e12:.2f} TB/s (measured float4 copy).", ""]
    for name, size, taps in WORKLOADS:
        model = create_model(name, pretrained="eva", cache_dir=None, trainable=False)
        tower, ops = model.visual, model.visual.engine.ops
        cfg = tower.cfg
        B, g = args.batch, size // cfg.patch_size
        N, C = g * g + 1, cfg.width
        x = torch.randn(B * N, C, device="cuda")
        out32, out16 = torch.empty(B, C, g, g, device="cuda"), torch.empty(B, C, g, g, device="cuda", dtype=torch.bfloat16)
        expr = lambda: x.view(B, N, C)[:, 1:].permute(0, 2, 1).contiguous()
        expr16 = lambda: x.view(B, N, C)[:, 1:].permute(0, 2, 1).contiguous().to(torch.bfloat16)
        ops.tokens_to_nchw(x, B, N, C, out32)
        ops.tokens_to_nchw(x, B, N, C, out16)
        same = torch.equal(out32.view(B, C, g * g), expr()) and torch.equal(out16.view(B, C, g * g), expr16())
        k32, t32, k16, t16 = alternate([lambda: ops.tokens_to_nchw(x, B, N, C, out32), expr,
                                        lambda: ops.tokens_to_nchw(x, B, N, C, out16), expr16], args.reps, args.inner)
        elems = B * g * g * C
        lines += [f"## {name} at {size} x {size}, {B} images: stream [{B * N}, {C}] fp32 -> [{B}, {C}, {g}, {g}]", "",
                  f"Outputs bit-identical to the torch expression: {'yes' if same else 'NO'}.", "",
                  "| one tap | time (us) | bytes moved (MB) | rate (TB/s) | of the ceiling |", "|---|---|---|---|---|"]
        for label, (med, lo, hi), nbytes in (("kernel, fp32 out", k32, elems * 8), ("torch permute + contiguous, fp32", t32, elems * 8),
                                            ("kernel, bf16 out", k16, elems * 6), ("torch permute + contiguous + to(bf16)", t16, elems * 6)):
            lines.append(f"| {label} | {med * 1e6:.1f} ({lo * 1e6:.1f} - {hi * 1e6:.1f}) | {nbytes / 1e6:.1f} | {nbytes / med / 1e12:.2f} | "
                         f"{100 * nbytes / med / STREAM_CEILING:.0f} % |")
        lines += ["", f"Kernel / torch: fp32 {k32[0] / t32[0]:.2f}x the time, bf16 {k16[0] / t16[0]:.2f}x "
                      f"(the torch bf16 form is two kernels and moves {elems * 14 / 1e6:.1f} MB).", ""]
        images = torch.randn(B, 3, size, size, device="cuda")
        with_taps = lambda: tower.forward_intermediates(images, taps)
        without = lambda: tower.engine.encode_dense(images)
        (pt, ptlo, pthi), (pn, pnlo, pnhi) = alternate([with_taps, without], args.pass_reps, args.pass_inner)
        lines += [f"Whole frozen pass, {cfg.layers} blocks, taps after blocks {taps} + the dense map: {pt * 1e3:.2f} ms ({ptlo * 1e3:.2f} - {pthi * 1e3:.2f}) "
                  f"= {B / pt:.1f} images / s; the same pass without taps {pn * 1e3:.2f} ms ({pnlo * 1e3:.2f} - {pnhi * 1e3:.2f}) "
                  f"(medians over {args.pass_reps} alternated windows of {args.pass_inner} passes).  Four times the standalone kernel time above: "
                  f"{4 * k32[0] * 1e3:.3f} ms = {100 * 4 * k32[0] / pt:.2f} % of the pass time -- a figure from the kernel alone, not from "
                  f"the pass; the difference of the two pass medians is {(pt - pn) * 1e3:.3f} ms, to be read against their spread.", "",
                  "Rates above the float4-copy ceiling are warm-cache rates: every window re-reads the same stream tensor, part of which the "
                  "256 MB last-level cache still holds; the torch expression runs under the same condition.", ""]
        del model, tower, x, out32, out16, images
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
