"""Text-tower measurements on the MI355X (device events, warm-up, repeats; results as a markdown table):

  (a) cs_attn_query_fwd(allow = NULL), the causal kernel, at (B, L, H) = (4096, 77, 8) and (4096, 24, 8) against the route the ABI offered
      before it: the masked kernel (attn_cls_kernel) fed an explicit lower-triangular `allow` table of B * L * L bytes;
  (b) encode_text sequences / s for the EVA02-CLIP-B-16 text shape (width 512, 8 heads, 12 layers, context 77) at B = 4096, prompts whose
      end-of-text id sits at positions 4 .. 24: trimmed (the default) and trim=False.

    python tools/text_bench.py [--out profiles/text_tower_bench.md] [--batch 4096] [--reps 20]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, warmup, reps):
    """Median and minimum milliseconds of fn() over `reps` device-event pairs after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", default="EVA02-CLIP-B-16")
    args = ap.parse_args(argv)
    from clipself_amd.hip import HipOps
    from clipself_amd.init import seeded_text_state
    from clipself_amd.open_clip import create_model
    ops = HipOps()
    B, H, C = args.batch, 8, 512
    lines = [f"device: {torch.cuda.get_device_name(0)}, {ops.num_compute_units()} CUs; times are medians (minimum) of {args.reps} runs "
             f"({max(5, args.reps // 2)} for encode_text) after warm-up, device events",
             "", "| case | shape (B, L, H) | causal kernel | masked kernel + `allow` table | ratio |", "|---|---|---|---|---|"]
    for L in (77, 24):
        g = torch.Generator().manual_seed(L)
        qkv = (torch.randn(B * L, 3 * C, generator=g) * 1.5).to(torch.bfloat16).cuda()
        allow = torch.ones(L, L, dtype=torch.uint8).tril_().repeat(B, 1).cuda()
        o1, o2 = torch.empty(B * L, C, dtype=torch.bfloat16, device="cuda"), torch.empty(B * L, C, dtype=torch.bfloat16, device="cuda")
        f_new = lambda: ops.attn_query_fwd(qkv[:, :C], qkv[:, C:], None, o1, B, L, L, H, 0.125)
        f_old = lambda: ops.attn_query_fwd(qkv[:, :C], qkv[:, C:], allow, o2, B, L, L, H, 0.125)
        # the same warm-up and repeats for both sides, taken twice in alternation (new, old, new, old): the second pair is reported, the
        # first also absorbs code-object loading and the clock ramp
        for _ in range(2):
            new = timed(f_new, 5, args.reps)
            old = timed(f_old, 5, args.reps)
        err = float((o1.float() - o2.float()).norm() / o2.float().norm())
        gb = B * L * (3 * C + C) * 2 / 1e9                         # q, k, v read once, o written once
        lines.append(f"| (a) attention | ({B}, {L}, {H}) | {new[0] * 1e3:.0f} us ({new[1] * 1e3:.0f}); {gb / new[0] * 1e3:.0f} GB/s of q\\|k\\|v + o | "
                     f"{old[0] * 1e3:.0f} us ({old[1] * 1e3:.0f}) + {allow.numel() / 1e6:.1f} MB table | {old[0] / new[0]:.1f}x (outputs rel-L2 {err:.1e} apart) |")
        del qkv, allow, o1, o2
    model = create_model(args.model, "eva", trainable=False, ops=ops)
    cfg = model.visual.cfg
    model.load_state_dict(seeded_text_state(cfg, 1), strict=False)
    g = torch.Generator().manual_seed(7)
    ids = torch.zeros(B, cfg.text_context, dtype=torch.long)
    eot = torch.randint(4, 25, (B,), generator=g)
    for row in range(B):
        ids[row, :eot[row]] = torch.randint(1, cfg.text_vocab - 2, (int(eot[row]),), generator=g)
        ids[row, eot[row]] = cfg.text_vocab - 1
    ids = ids.cuda()
    lines += ["", f"| case | model | L | time per {B} sequences | sequences / s |", "|---|---|---|---|---|"]
    res = {}
    for trim in (True, False):
        t = timed(lambda: model.encode_text(ids, trim=trim), 3, max(5, args.reps // 2))
        res[trim] = t
        L = int(eot.max()) + 1 if trim else cfg.text_context
        lines.append(f"| (b) encode_text, {'trimmed' if trim else 'trim=False'} | {args.model} text tower ({cfg.text_width} / {cfg.text_heads} heads, "
                     f"{cfg.text_layers} layers) | {L} | {t[0]:.1f} ms ({t[1]:.1f}) | {B / t[0] * 1e3:,.0f} |")
    lines.append("")
    lines.append(f"trimming: {res[False][0] / res[True][0]:.1f}x")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
