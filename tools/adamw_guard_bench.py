#!/usr/bin/env python
"""Step tail (gradient clipping + AdamW) on the flat buffers of EVA02-CLIP-B-16 and EVA02-CLIP-L-14-336, synthetic gradients,
--grad-clip-norm 1.0: the torch passage (clip_grad_norm_ over the parameter views + the unguarded cs_adamw_step), the guarded
cs_adamw_step (norm, finalise and update in one C-ABI call) and the unguarded cs_adamw_step alone.  Stream events around each call,
the variants interleaved inside every repetition, medians reported.  The W^T shadow refresh that follows AdamW in a step is the same
in every variant and is left out.

usage: tools/adamw_guard_bench.py [--reps 30] [--out profiles/adamw_guard_bench.md] [--models NAME ...]
       tools/adamw_guard_bench.py --unguarded-abi-before         (child mode: time the library named by CLIPSELF_HIP_LIB, built from the
                                                                  commit before the guard, through its 15-argument cs_adamw_step)
With --lib-before PATH the tool starts that child itself and adds its row ("unguarded, before") to the table."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from clipself_amd import hip  # noqa: E402
from clipself_amd.config import get_tower_cfg  # noqa: E402

HBM_STREAM_TBS = 6.3                                    # float4 streams, MI355X (adamw_kernel reaches it)
HYPER = (1e-5, 0.9, 0.999, 1e-8, 0.1)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    return a, b


def flat_layout(name):
    """(student, engine, parameters holding a gradient view) of the flat store with every block training (--lock-image with all groups
    unlocked, the shipped recipe); nothing is run, so no activation is allocated."""
    from clipself_amd.open_clip.model import CustomCLIP
    student = CustomCLIP(get_tower_cfg(name), trainable=True)
    student.lock_image_tower(unlocked_groups=student.visual.cfg.layers)
    student.visual._attach_grads()                      # what a backward leaves: p.grad = a view of the flat gradient buffer
    return student, student.visual.engine, [p for p in student.parameters() if p.grad is not None]


def bench_model(name, reps, ops):
    student, eng, views = flat_layout(name)
    n = eng.numel
    gen = torch.Generator(device="cuda").manual_seed(3)
    grad0 = torch.randn(n, generator=gen, device="cuda") * 1e-3
    guard = torch.zeros(ops.adamw_guard_numel(n), device="cuda")
    stream = torch.cuda.current_stream()
    bufs = (eng.master, eng.grad, eng.exp_avg, eng.exp_avg_sq, eng.shadow, eng.flags)
    step = [0]

    def unguarded():
        step[0] += 1
        ops.adamw_step(*bufs, *HYPER, step[0])

    def guarded():
        step[0] += 1
        ops.adamw_step(*bufs, *HYPER, step[0], 1.0, max_norm=1.0, skip_nonfinite=True, guard=guard)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(views, 1.0, norm_type=2.0)
        unguarded()

    variants = {"torch tail (clip_grad_norm_ + cs_adamw_step)": torch_tail, "guarded cs_adamw_step": guarded, "unguarded cs_adamw_step": unguarded}
    times = {k: [] for k in variants}
    for rep in range(reps + 3):
        events = {}
        for k, fn in variants.items():
            eng.grad.copy_(grad0)                       # clip_grad_norm_ rescales in place: every variant starts from the same gradient
            events[k] = timed(fn, stream)
        torch.cuda.synchronize()
        if rep >= 3:
            for k, (a, b) in events.items():
                times[k].append(a.elapsed_time(b) * 1e3)
    stats = guard[:4].tolist()
    active = int((eng.flags & 1).sum()) * 64
    rows = {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}
    del student
    return dict(model=name, numel=n, active=active, views=len(views), rows=rows, norm=stats[0], coef=stats[1])


def norm_pass_us(ops, n, reps):
    """The norm pass alone (launch (a) + (b) + a guarded update that finds head[2] == 0 and returns): an Inf in the gradient with skip_nonfinite."""
    g = torch.randn(n, device="cuda") * 1e-3
    g[0] = float("inf")
    flags = torch.ones(n // 64, dtype=torch.uint8, device="cuda")
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    guard = torch.zeros(ops.adamw_guard_numel(n), device="cuda")
    stream, ts = torch.cuda.current_stream(), []
    for rep in range(reps + 3):
        a, b = timed(lambda: ops.adamw_step(p, g, m, v, None, flags, *HYPER, 1, 1.0, max_norm=1.0, skip_nonfinite=True, guard=guard), stream)
        torch.cuda.synchronize()
        if rep >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    assert guard[2].item() == 0.0
    return statistics.median(ts)


def unguarded_abi_before(models, reps):
    """Child mode: the library of the commit before the guard (15-argument cs_adamw_step), raw ctypes, same buffers and hyper-parameters."""
    lib = ctypes.CDLL(os.environ["CLIPSELF_HIP_LIB"])
    vp, f, i, l = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_long
    lib.cs_adamw_step.restype, lib.cs_adamw_step.argtypes = i, [vp] * 6 + [l] + [f] * 5 + [i, f, vp]
    out = {}
    for name in models:
        student, eng, _ = flat_layout(name)               # the layout is this tree's (it did not change); the old library only sees raw pointers
        n, flags = eng.numel, eng.flags
        bufs = [torch.zeros(n, device="cuda") for _ in range(4)]
        bufs[1].normal_(0, 1e-3)
        shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        stream, ts = torch.cuda.current_stream(), []
        for rep in range(reps + 3):
            a, b = timed(lambda: lib.cs_adamw_step(*(t.data_ptr() for t in bufs), shadow.data_ptr(), flags.data_ptr(), n, *HYPER, rep + 1, 1.0,
                                                   stream.cuda_stream), stream)
            torch.cuda.synchronize()
            if rep >= 3:
                ts.append(a.elapsed_time(b) * 1e3)
        out[name] = (statistics.median(ts), min(ts), max(ts))
    print("BEFORE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--models", nargs="+", default=["EVA02-CLIP-B-16", "EVA02-CLIP-L-14-336"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adamw_guard_bench.md"))
    ap.add_argument("--lib-before", default=None, help="libclipself_hip.so built from the commit before the guard: adds the 'unguarded, before' row")
    ap.add_argument("--unguarded-abi-before", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_guard_bench.py measures on the GPU; none is visible")
    if a.unguarded_abi_before:
        unguarded_abi_before(a.models, a.reps)
        return
    before = {}
    if a.lib_before:                                    # a fresh child process, started before this one touches the device
        r = subprocess.run([sys.executable, __file__, "--unguarded-abi-before", "--reps", str(a.reps), "--models", *a.models],
                           env=dict(os.environ, CLIPSELF_HIP_LIB=a.lib_before), capture_output=True, text=True, timeout=300)
        line = [x for x in r.stdout.splitlines() if x.startswith("BEFORE ")]
        if r.returncode != 0 or not line:
            raise SystemExit(f"the 'before' child failed ({r.returncode}):\n{r.stderr[-2000:]}")
        before = json.loads(line[0][len("BEFORE "):])
    ops = hip.HipOps()
    lines = ["# Step tail: gradient clipping + AdamW, torch passage vs the guarded cs_adamw_step", "",
             f"tools/adamw_guard_bench.py, {a.reps} repetitions, variants interleaved inside each repetition, stream events, median (min .. max) in µs.",
             "Synthetic gradients (N(0, 1e-3)), `--grad-clip-norm 1.0` (the clip is active), every block training; the W^T shadow refresh that",
             "follows AdamW in a step is identical in all variants and not included.", ""]
    for name in a.models:
        res = bench_model(name, a.reps, ops)
        n = res["numel"]
        norm_us = norm_pass_us(ops, n, a.reps)
        gbs = 4.0 * n / norm_us / 1e3                   # bytes / µs -> GB/s: the pass reads the fp32 gradient once (flags: 1/256 of that)
        lines += [f"## {name}: {n / 1e6:.1f} M parameters in the flat store ({res['active'] / 1e6:.1f} M active), {res['views']} parameter views; "
                  f"gradient norm {res['norm']:.4g}, clip coefficient {res['coef']:.4g}", "",
                  "| variant | median µs | min .. max µs |", "|---|---|---|"]
        for k, (med, lo, hi) in res["rows"].items():
            lines.append(f"| {k} | {med:.1f} | {lo:.1f} .. {hi:.1f} |")
        if name in before:
            med, lo, hi = before[name]
            lines.append(f"| unguarded cs_adamw_step, library built before this change (own process) | {med:.1f} | {lo:.1f} .. {hi:.1f} |")
        lines += [f"| norm pass alone (partial sums + finalise + an update that is skipped), all {n / 1e6:.1f} M elements active | {norm_us:.1f} | |", "",
                  f"Norm pass: {4.0 * n / 1e6:.0f} MB read in {norm_us:.1f} µs = {gbs:.0f} GB/s, {100 * gbs / (HBM_STREAM_TBS * 1e3):.0f} % of the "
                  f"{HBM_STREAM_TBS} TB/s float4 stream ceiling (floor {4.0 * n / (HBM_STREAM_TBS * 1e6):.0f} µs).", ""]
    text = "\n".join(lines)
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
