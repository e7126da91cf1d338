#!/usr/bin/env python
"""GPU micro-benchmark of cs_attn_fwd on the teacher's shape (512 crops x 12 heads x 197 tokens); see profiles/r01_n_*.
env: CS_ATTN_DBG (ablation bits 1 / 2 / 4, builds with -DCS_ABLATION_SWITCHES only).   usage: python tools/attn_bench.py [crops [bwd]]
       python tools/attn_bench.py CROPS norope [bwd] [rounds]: identity tables (cos 1, sin 0) against NULL tables (no rotary embedding), the same
       inputs, timed alternately in one process; the spread of the identity leg over the rounds is the run-to-run noise (profiles/attn_norope_bench.md)"""
import sys, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clipself_amd.hip import HipOps
ops = HipOps()
B, N, H = (int(sys.argv[1]) if len(sys.argv) > 1 else 512), 197, 12
C = H * 64
qkv = torch.randn(B * N, 3 * C, device="cuda").to(torch.bfloat16)
g = 14                                                   # separable tables as rope.py:118-142 builds them
freqs = 10000.0 ** (-torch.arange(0, 32, 2).float() / 32)
ang = (torch.arange(g).float() / g * 16)[:, None] * freqs[None, :]
ang = ang.repeat_interleave(2, dim=-1)
full = torch.cat([ang[:, None, :].expand(g, g, 32), ang[None, :, :].expand(g, g, 32)], dim=-1).reshape(g * g, 64)
cos, sin = full.cos().contiguous().cuda(), full.sin().contiguous().cuda()
out = torch.empty(B * N, C, dtype=torch.bfloat16, device="cuda")
if len(sys.argv) > 2 and sys.argv[2] == "norope":
    bwd = "bwd" in sys.argv[3:]
    rounds = next((int(a) for a in sys.argv[3:] if a.isdigit()), 5)
    legs = {"identity": (torch.ones_like(cos), torch.zeros_like(sin)), "null": (None, None)}
    lse = torch.empty(B * H, N, device="cuda")
    ops.attn_fwd(qkv, None, None, out, lse, B, N, H, 0.125)
    dout, dqkv = torch.randn_like(out), torch.empty_like(qkv)
    ws = torch.empty(ops.attn_bwd_workspace(B, N, H), dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(3):
            fn()
        e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        reps = int(min(max(60.0 / max(e0.elapsed_time(e1), 1e-3), 20), 2000))       # a timed window of >= 60 ms
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    t = {(k, w): [] for k in legs for w in ("fwd", "bwd")}
    for r in range(rounds):
        for k, (c, s) in legs.items():
            t[k, "fwd"].append(timed(lambda: ops.attn_fwd(qkv, c, s, out, None, B, N, H, 0.125)))
            if bwd:
                t[k, "bwd"].append(timed(lambda: ops.attn_bwd(qkv, out, dout, lse, c, s, dqkv, ws, B, N, H, 0.125)))
    for w in ("fwd", "bwd") if bwd else ("fwd",):
        i, n = sorted(t["identity", w]), sorted(t["null", w])
        mi, mn = i[len(i) // 2], n[len(n) // 2]
        print(f"{B} x {N} x {H} attn_{w} us: identity tables median {mi:.1f} (min {i[0]:.1f} max {i[-1]:.1f}, spread {100 * (i[-1] - i[0]) / mi:.1f} %) | "
              f"NULL tables median {mn:.1f} (min {n[0]:.1f} max {n[-1]:.1f}) | NULL / identity {mn / mi:.3f}", flush=True)
    sys.exit(0)
for _ in range(3):
    ops.attn_fwd(qkv, cos, sin, out, None, B, N, H, 0.125)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    ops.attn_fwd(qkv, cos, sin, out, None, B, N, H, 0.125)
e1.record(); torch.cuda.synchronize()
print("attn_fwd us:", e0.elapsed_time(e1) * 50)
if len(sys.argv) > 2 and sys.argv[2] == "bwd":          # python tools/attn_bench.py 64 bwd : the student's backward (dsum prep + dQ + dK/dV kernels)
    lse = torch.empty(B * H, N, device="cuda")
    ops.attn_fwd(qkv, cos, sin, out, lse, B, N, H, 0.125)
    dout = torch.randn_like(out)
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(ops.attn_bwd_workspace(B, N, H), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        ops.attn_bwd(qkv, out, dout, lse, cos, sin, dqkv, ws, B, N, H, 0.125)
    e0.record()
    for _ in range(20):
        ops.attn_bwd(qkv, out, dout, lse, cos, sin, dqkv, ws, B, N, H, 0.125)
    e1.record(); torch.cuda.synchronize()
    print("attn_bwd us:", e0.elapsed_time(e1) * 50)
