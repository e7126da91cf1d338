"""Times the detector's feature pyramid, fpn.FPN(in_channels=[w]*4, out_channels=256, num_outs=5, norm_cfg=SyncBN), on the MI355X: the
kernel route (Conv1x1 on cs_gemm_nt, forms 7 / 8 of cs_transpose_bf16 for the top-down step, Conv3x3, BatchNormAct2d) against the module's
own torch route (fused=False) in fp32 and under bf16 autocast with channels-last inputs.  The yardstick is torch's route, never the new
kernels against themselves.

Inputs are what EvaCLIPViT returns at B = 8: four NCHW fp32 maps, the two finest requiring a gradient (the neck's transposed convolutions
train, the two coarser maps come from the frozen tower).  Shapes (finest level's side, Cin):
  b16_640   160 / 80 / 40 / 20, 768      ViT-B/16 at 640 x 640
  b16_1024  256 / 128 / 64 / 32, 768     ViT-B/16 at 1024 x 1024
  l14_896   256 / 128 / 64 / 32, 1024    ViT-L/14-336 at 896 x 896
Measured, forward + backward each: the whole module (all kernels; kernels with torch's top-down step; torch fp32; torch bf16 autocast);
its three parts alone on detached inputs (laterals with their norms / top-down path / output convolutions with their norms); the
NCHW fp32 -> bf16 rows conversion in front of the laterals (HipOps.nchw_to_rows), as a share of the laterals' time; and forms 7 / 8 alone
at every level pair against fine + F.interpolate(coarse, scale_factor=2) and its autograd, with GB/s beside the 6.3 TB/s stream figure.

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  Prints markdown tables
and the verdicts the defaults rest on: fpn.FUSED_FPN_DEFAULT (the top-down kernels) and conv.FUSED_CONV1X1_DEFAULT (the laterals)."""
import argparse
import contextlib
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

STREAM_TBS = 6.3
SHAPES = {"b16_640": (160, 768), "b16_1024": (256, 768), "l14_896": (256, 1024)}
BF16, F32 = torch.bfloat16, torch.float32
B, COUT = 8, 256


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


def table(title, times, torch_keys):
    med = {k: statistics.median(v) for k, v in times.items()}
    best = min(med[k] for k in torch_keys)
    print(f"\n{title}\n\n| variant | µs median (min .. max) | faster torch variant / this |\n|---|---|---|")
    for k, v in times.items():
        print(f"| {k} | {fmt(v)} | {best / med[k]:.2f} x |")
    return med, best


def autocast(on):
    return torch.autocast("cuda", dtype=BF16) if on else contextlib.nullcontext()


def step(fn, leaves, params, amp=False):
    """One forward + backward of fn(leaves) -> tensors, with an upstream gradient of ones (prepared once, per output dtype and shape)."""
    ones = {}

    def run():
        for t in leaves:
            t.grad = None
        for p in params:
            p.grad = None
        with autocast(amp):
            outs = fn(leaves)
        outs = [o for o in outs if o.requires_grad]
        for o in outs:
            if (o.dtype, tuple(o.shape)) not in ones:
                ones[o.dtype, tuple(o.shape)] = torch.ones_like(o)
        torch.autograd.backward(outs, [ones[o.dtype, tuple(o.shape)] for o in outs])
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="b16_640,b16_1024,l14_896")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args(argv)
    from clipself_amd.det_layer import rows_bf16
    from clipself_amd.fpn import FPN, TopDownFn
    from clipself_amd.hip import HipOps
    ops = HipOps()
    print(f"windows of {args.iters} calls, {args.windows} windows, variants alternated; {ops.num_cus} compute units; B = {B}, "
          f"out_channels = {COUT}, norm_cfg = SyncBN (one rank), training mode")
    verdict_td, verdict_lat, verdict_all = {}, {}, {}
    for name in [s for s in args.shapes.split(",") if s]:
        side, cin = SHAPES[name]
        sides = [side >> i for i in range(4)]
        g = torch.Generator(device="cuda").manual_seed(0)
        xs = [torch.randn(B, cin, s, s, generator=g, device="cuda").requires_grad_(i < 2) for i, s in enumerate(sides)]
        xs_cl = [x.detach().contiguous(memory_format=torch.channels_last).requires_grad_(x.requires_grad) for x in xs]
        torch.manual_seed(0)
        cfg = dict(in_channels=[cin] * 4, out_channels=COUT, num_outs=5, norm_cfg=dict(type="SyncBN", requires_grad=True))
        mods = {"all kernels": FPN(ops=ops, fused=True, **cfg), "kernels, torch top-down": FPN(ops=ops, fused=True, **cfg),
                "torch fp32": FPN(ops=ops, fused=False, **cfg), "torch bf16 autocast, channels-last": FPN(ops=ops, fused=False, **cfg)}
        for m in mods.values():
            m.cuda().train().load_state_dict(mods["all kernels"].state_dict(), strict=True)
        hybrid = mods["kernels, torch top-down"]
        hybrid._merge = lambda fine, coarse: fine + F.interpolate(coarse, size=fine.shape[2:], mode="nearest")
        amp_key = "torch bf16 autocast, channels-last"
        torch_keys = ("torch fp32", amp_key)
        print(f"\n## {name}: levels {' / '.join(str(s) for s in sides)}, Cin {cin}")

        # ---- the whole module
        whole = {k: step(lambda leaves, m=m: m(tuple(leaves)), xs_cl if k == amp_key else xs, list(m.parameters()), amp=k == amp_key)
                 for k, m in mods.items()}
        med, best = table("whole module, forward + backward", measure(whole, args.iters, args.windows), torch_keys)
        verdict_all[name] = med["all kernels"] < best
        verdict_td[name] = med["all kernels"] < best and med["all kernels"] < med["kernels, torch top-down"]

        # ---- the parts alone, on detached inputs
        def lateral_outs(m, leaves, amp):
            with torch.no_grad(), autocast(amp):
                return [c(x).detach() for c, x in zip(m.lateral_convs, leaves)]

        def merged_of(m, lats, amp):
            with torch.no_grad(), autocast(amp):
                out = list(lats)
                for i in range(3, 0, -1):
                    out[i - 1] = m._merge(out[i - 1], out[i])
                return [t.detach() for t in out]

        def topdown(m):
            def fn(lats):
                out = list(lats)
                for i in range(3, 0, -1):
                    out[i - 1] = m._merge(out[i - 1], out[i])
                return out[:3]
            return fn
        parts = {"laterals (1x1 + norm)": {}, "top-down path": {}, "output convolutions (3x3 + norm)": {}}
        for k, m in mods.items():
            if k == "kernels, torch top-down":
                continue
            amp, leaves = k == amp_key, (xs_cl if k == amp_key else xs)
            lats = [t.requires_grad_(True) for t in lateral_outs(m, leaves, amp)]
            mer = [t.requires_grad_(True) for t in merged_of(m, lats, amp)]
            parts["laterals (1x1 + norm)"][k] = step(lambda lv, m=m: [c(x) for c, x in zip(m.lateral_convs, lv)], leaves,
                                                     list(m.lateral_convs.parameters()), amp)
            parts["top-down path"][k] = step(topdown(m), lats, [], amp)
            parts["output convolutions (3x3 + norm)"][k] = step(lambda lv, m=m: [c(x) for c, x in zip(m.fpn_convs, lv)], mer,
                                                                list(m.fpn_convs.parameters()), amp)
        part_med = {}
        for title, variants in parts.items():
            part_med[title], best = table(f"{title} alone, forward + backward", measure(variants, args.iters, args.windows), torch_keys)
            if title.startswith("laterals"):
                verdict_lat[name] = part_med[title]["all kernels"] < best

        # ---- the conversion in front of the laterals
        conv = measure({"nchw_to_rows": lambda: [rows_bf16(ops, x.detach()) for x in xs]}, args.iters, args.windows)["nchw_to_rows"]
        lat = part_med["laterals (1x1 + norm)"]["all kernels"]
        print(f"\nNCHW fp32 -> bf16 rows of the four inputs (HipOps.nchw_to_rows): {fmt(conv)} µs = "
              f"{100 * statistics.median(conv) / lat:.1f} % of the kernel laterals' forward + backward ({lat:.0f} µs)")

        # ---- forms 7 / 8 alone
        print("\nforms 7 / 8 alone, C = 256\n\n| level pair | type | variant | µs median (min .. max) | GB/s | share of "
              f"{STREAM_TBS} TB/s | torch / this |\n|---|---|---|---|---|---|---|")
        for hs in sides[1:]:
            for dt in (F32, BF16):
                es = 4 if dt == F32 else 2
                coarse = torch.randn(B * hs * hs, COUT, generator=g, device="cuda").to(dt)
                fine = torch.randn(4 * B * hs * hs, COUT, generator=g, device="cuda").to(dt)
                work, pooled = fine.clone(), torch.empty_like(coarse)
                cm = coarse.view(B, hs, hs, COUT).permute(0, 3, 1, 2).requires_grad_(True)
                fm = fine.view(B, 2 * hs, 2 * hs, COUT).permute(0, 3, 1, 2).requires_grad_(True)
                nb_c, nb_f = coarse.numel() * es, fine.numel() * es
                variants = {
                    "form 7 (accumulate in place)": (lambda: ops.upsample2x_add(coarse, work, B, hs, hs, COUT, True), nb_c + 2 * nb_f),
                    "form 8 (overwrite)": (lambda: ops.pool2x(fine, pooled, B, hs, hs, COUT, False), nb_c + nb_f),
                    "torch fine + interpolate, forward": (lambda: fm.detach() + F.interpolate(cm.detach(), scale_factor=2, mode="nearest"), None),
                    "kernels forward + backward (copy, form 7, form 8)": (step(lambda lv: [TopDownFn.apply(lv[0], lv[1], ops)], [fm, cm], []),
                                                                          2 * nb_f + nb_c + 2 * nb_f + nb_f + nb_c),
                    "torch forward + backward": (step(lambda lv: [lv[0] + F.interpolate(lv[1], scale_factor=2, mode="nearest")], [fm, cm], []), None),
                }
                times = measure({k: v[0] for k, v in variants.items()}, args.iters, args.windows)
                med = {k: statistics.median(v) for k, v in times.items()}
                ref = {"form 7 (accumulate in place)": "torch fine + interpolate, forward", "form 8 (overwrite)": None,
                       "kernels forward + backward (copy, form 7, form 8)": "torch forward + backward"}
                for k, (_, nbytes) in variants.items():
                    gbs = "" if nbytes is None else f"{nbytes / med[k] / 1e3:.0f}"
                    share = "" if nbytes is None else f"{100 * nbytes / med[k] / 1e3 / (STREAM_TBS * 1e3):.0f} %"
                    ratio = f"{med[ref[k]] / med[k]:.2f} x" if ref.get(k) else ""
                    print(f"| {2 * hs} <- {hs} | {'fp32' if dt == F32 else 'bf16'} | {k} | {fmt(times[k])} | {gbs} | {share} | {ratio} |")
        del xs, xs_cl, mods, whole, parts
        torch.cuda.empty_cache()
    print(f"\nall kernels win forward + backward against the faster torch variant at: {verdict_all}")
    print(f"... and against the kernels with torch's top-down step: {verdict_td}  ->  FUSED_FPN_DEFAULT = {all(verdict_td.values())}")
    print(f"kernel laterals win forward + backward against the faster torch variant at: {verdict_lat}  ->  "
          f"FUSED_CONV1X1_DEFAULT = {all(verdict_lat.values())}")


if __name__ == "__main__":
    main()
