"""Detector neck on the MI355X: the 2x2 transposed convolutions as GEMMs on the token stream (neck.Deconv2x2) against torch's convolutions.

    python tools/neck_bench.py [--out profiles/neck_bench.md] [--batch 8] [--reps 9]

Workloads: the shipped F-ViT detector shapes -- EVA02-CLIP-B-16 at 1024 x 1024 (width 768) and EVA02-CLIP-L-14-336 at 896 x 896 (width
1024), 64 x 64 grid either way, 8 images, BN in interpolate1.  Seeded weights (timings do not depend on the values).

Part `neck`: from the tower's fp32 stream [B*N, C] to the two outputs interpolate1(tap 0) and interpolate2(tap 1).  Three variants
alternated window by window in one process: torch fp32 (HipOps.tokens_to_nchw fp32 maps -> nn.ConvTranspose2d through MIOpen), torch under
bf16 autocast (the same maps), fused (cs_cast_f32_bf16 rows -> Deconv2x2).  Each variant includes the copy of the stream it needs.
Forward (no_grad) and forward + backward (grad enabled; fixed output gradients, all six neck gradients and the input gradient of the
second layer) are timed separately: device events around `--inner` iterations, medians over `--reps` windows.
Part `model`: the whole EvaCLIPViT training-mode forward + backward with each neck.

Every (workload, part) runs in a child process of its own under a time limit; the parent never opens the GPU, stops at the first child
that fails, and writes the table.  Needs the GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {"b16": ("EVA02-CLIP-B-16", 1024, [3, 5, 7, 11]), "l14": ("EVA02-CLIP-L-14-336", 896, [6, 10, 14, 23])}
VARIANTS = ("torch fp32", "torch bf16 autocast", "fused")
CHILD_LIMIT = 420                                 # seconds per child: MIOpen may search for its convolution kernels on first use


def window(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def alternate(fns, reps, inner):
    """(median, min, max) seconds per call of each fn, windows alternated fn by fn."""
    for fn in fns:
        window(fn, 2)
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            t.append(window(fn, inner))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def build(name, fused, taps):
    import torch
    from clipself_amd.fvit import EvaCLIPViT
    torch.manual_seed(1)
    return EvaCLIPViT(name, None, out_indices=taps, norm_cfg=dict(type="BN", requires_grad=True), fused_neck=fused).cuda().train()


def child(args):
    import torch
    from clipself_amd.neck import TokenRows
    name, size, taps = WORKLOADS[args.workload]
    plain, fused = build(name, False, taps), build(name, True, taps)
    fused.load_state_dict(plain.state_dict(), strict=True)
    ops, cfg = plain.visual.engine.ops, plain.visual.cfg
    B, g, C = args.batch, size // cfg.patch_size, plain.width
    N = g * g + 1
    gen = torch.Generator(device="cuda").manual_seed(2)
    grads = [torch.randn(B, C, 4 * g, 4 * g, device="cuda", generator=gen), torch.randn(B, C, 2 * g, 2 * g, device="cuda", generator=gen)]
    result = {"workload": args.workload, "part": args.part, "name": name, "size": size, "batch": B, "grid": g, "width": C,
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner}
    if args.part == "neck":
        x = torch.randn(B * N, C, device="cuda", generator=gen)

        def torch_neck(autocast):
            def run():
                maps = [ops.empty((B, C, g, g), torch.float32) for _ in range(2)]
                for m in maps:
                    ops.tokens_to_nchw(x, B, N, C, m)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    return [plain.interpolate1(maps[0]), plain.interpolate2(maps[1])]
            return run

        def fused_neck():
            rows = [ops.empty((B * N, C), torch.bfloat16) for _ in range(2)]
            for r in rows:
                ops.cast_f32_bf16(x, r)
            return [fused.interpolate1(TokenRows(rows[0], B, g, g, 1)), fused.interpolate2(TokenRows(rows[1], B, g, g, 1))]

        runs = [torch_neck(False), torch_neck(True), fused_neck]

        def fwd(run):
            def f():
                with torch.no_grad():
                    run()
            return f

        def fwd_bwd(run, mod):
            def f():
                mod.zero_grad(set_to_none=True)
                outs = run()
                torch.autograd.backward(outs, [gr.to(o.dtype) for gr, o in zip(grads, outs)])
            return f
        with torch.no_grad():
            ref, got = runs[0](), runs[2]()
        result["rel_l2_fused_vs_fp32"] = [float((a.double() - b.double()).norm() / b.double().norm()) for a, b in zip(got, ref)]
        del ref, got
        result["forward"] = alternate([fwd(r) for r in runs], args.reps, args.inner)
        result["forward_backward"] = alternate([fwd_bwd(r, m) for r, m in zip(runs, (plain, plain, fused))], args.reps, args.inner)
    else:
        images = torch.randn(B, 3, size, size, device="cuda", generator=gen)

        def step(mod, autocast):
            def f():
                mod.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    outs = mod(images)
                torch.autograd.backward(list(outs[:2]), [gr.to(o.dtype) for gr, o in zip(grads, outs)])
            return f
        result["forward_backward"] = alternate([step(plain, False), step(plain, True), step(fused, False)], args.reps, args.inner)
    torch.cuda.synchronize()
    Path(args.json).write_text(json.dumps(result))
    print(json.dumps(result))


def fmt(t):
    med, lo, hi = t
    return f"{med * 1e3:.2f} ({lo * 1e3:.2f} - {hi * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "neck_bench.md"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--workload", choices=sorted(WORKLOADS))
    ap.add_argument("--part", choices=["neck", "model"])
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.workload:
        return child(args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    results = []
    for wl in WORKLOADS:
        for part in ("neck", "model"):
            js = out.with_name(f"{out.stem}_{wl}_{part}.json")
            cmd = [sys.executable, __file__, "--workload", wl, "--part", part, "--json", str(js), "--batch", str(args.batch),
                   "--reps", str(args.reps), "--inner", str(args.inner)]
            print("+", " ".join(cmd), flush=True)
            try:
                rc = subprocess.run(cmd, timeout=CHILD_LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                                  # nothing more is started on the GPU after a failure
                raise SystemExit(f"neck_bench: {wl} / {part} ended with status {rc}; stopping")
            results.append(json.loads(js.read_text()))
            js.unlink()
    r0 = results[0]
    lines = ["# Detector neck: 2x2 transposed convolutions as GEMMs on the token stream against torch's convolutions", "",
             f"`python tools/neck_bench.py --batch {args.batch} --reps {args.reps} --inner {args.inner}` on {r0['device']}; milliseconds, medians over "
             f"{args.reps} windows of {args.inner} iterations, the three variants alternated window by window in one process per table "
             f"(min - max in brackets).  BN in interpolate1; each neck variant includes the copy of the fp32 stream it reads (two fp32 "
             f"maps for torch, two bf16 row casts for the fused path).", ""]
    for r in results:
        title = f"## {r['name']} at {r['size']} x {r['size']}, {r['batch']} images, {r['grid']} x {r['grid']} grid, width {r['width']}: "
        if r["part"] == "neck":
            lines += [title + "the neck alone", "", "| variant | forward (no_grad) | forward + backward |", "|---|---|---|"]
            lines += [f"| {v} | {fmt(r['forward'][i])} | {fmt(r['forward_backward'][i])} |" for i, v in enumerate(VARIANTS)]
            fb = [t[0] for t in r["forward_backward"]]
            lines += ["", f"Fused against the faster torch variant, forward + backward: {fb[2] / min(fb[:2]):.2f}x the time.  Fused outputs "
                          f"against the fp32 torch neck: rel-L2 {r['rel_l2_fused_vs_fp32'][0]:.2e} / {r['rel_l2_fused_vs_fp32'][1]:.2e}.", ""]
        else:
            lines += [title + "EvaCLIPViT training-mode forward + backward", "", "| neck | forward + backward | images / s |", "|---|---|---|"]
            lines += [f"| {v} | {fmt(r['forward_backward'][i])} | {r['batch'] / r['forward_backward'][i][0]:.1f} |" for i, v in enumerate(VARIANTS)]
            lines.append("")
    text = "\n".join(lines)
    out.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
