#!/usr/bin/env python
"""The frozen tower's two folded-LayerNorm GEMMs at the step's launch shapes (M = 403 456 rows, K = 768) with the K loop on
v_mfma_f32_16x16x32_bf16 (the default) and on v_mfma_f32_32x32x16_bf16 (CS_GEMM_MFMA32=1): interleaved rounds in one process on one
device, random operands, median and minimum of the rounds per form.
usage (GPU box): python tools/gemm_mfma_ab.py [--shape qkv|w12|both] [--rounds 7] [--launches 10] [--warm-seconds 3] [--only new|old]
  --only: one form alone, for a rocprofv3 --pmc GRBM_GUI_ACTIVE pass of its own (held clock = GRBM_GUI_ACTIVE / 8 / duration)"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clipself_amd.hip import HipOps  # noqa: E402

BF = torch.bfloat16
SWITCH = "CS_GEMM_MFMA32"


def form(name):
    if name == "old":
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warm-seconds", type=float, default=3.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--rows", type=int, default=403456)
    o = ap.parse_args()
    ops = HipOps()
    M, K = o.rows, 768
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(M, K, device="cuda", generator=g).to(BF)
    mean, rstd = A.float().mean(-1), 1.0 / (A.float().var(-1, unbiased=False) + 1e-6).sqrt()
    print(f"device {torch.cuda.get_device_name(0)}; M = {M}, K = {K}; {o.rounds} interleaved rounds of {o.launches} launches after {o.warm_seconds} s warm-up per form", flush=True)
    for name, N, epi in (("qkv", 2304, 0), ("w12", 4096, 3)):
        if o.shape not in (name, "both"):
            continue
        B = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(BF)
        bias, colsum = torch.randn(N, device="cuda", generator=g), B.float().sum(-1)
        if epi == 3:
            C = torch.empty(M, N // 2, dtype=BF, device="cuda")
            part = torch.empty(4 * ((N // 2 + 127) // 128), M, 2, device="cuda")
            run = lambda: ops.gemm_nt_ln(A, B, C, bias=bias, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, stats_part=part, epi=3, group=N // 2)
        else:
            C = torch.empty(M, N, dtype=BF, device="cuda")
            run = lambda: ops.gemm_nt_ln(A, B, C, bias=bias, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, epi=0)
        forms = [o.only] if o.only else ["old", "new"]
        for f in forms:
            form(f)
            t0 = time.time()
            while time.time() - t0 < o.warm_seconds:
                timed(run, o.launches)
        res = {f: [] for f in forms}
        for _ in range(o.rounds):
            for f in forms:
                form(f)
                res[f].append(timed(run, o.launches))
        form("new")
        flop = 2.0 * M * N * K
        for f in forms:
            r = res[f]
            print(f"{name} N={N} epi={epi} {f:>3} ({'32x32x16' if f == 'old' else '16x16x32'}): median {statistics.median(r):7.1f} us  min {min(r):7.1f}  max {max(r):7.1f}"
                  f"  ({flop / statistics.median(r) * 1e-6:6.1f} TFLOP/s at the median)  rounds " + " ".join(f"{x:.1f}" for x in r), flush=True)
        if len(forms) == 2:
            new_med, old_min = statistics.median(res["new"]), min(res["old"])
            print(f"{name}: median of the new form {new_med:.1f} us vs minimum of the old form's rounds {old_min:.1f} us: "
                  f"{'PASS' if new_med < old_min else 'FAIL'} ({100 * (new_med / statistics.median(res['old']) - 1):+.2f} % median to median)", flush=True)
        del B, C


if __name__ == "__main__":
    main()
