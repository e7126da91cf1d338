#!/usr/bin/env python
"""One-GPU timing of the CLIPSelf step on the OpenAI-CLIP ViT family, same batch shape as BASELINE configs[1]:
usage (GPU box): python tools/openai_vit_bench.py [--extract-type v1|v2] [--steps N] [--crop-size S] [--rope-ab R] [ViT-B-16 [images [crops [size [plain]]]]]
("plain" = teacher without the folded LayerNorms / CLS-only last block, the A/B switch of engine_openai.py; --extract-type v1 = the student
pools every box through an extra query token (mask-attention pooling) instead of the dense map + RoIAlign; profiles/maskattn_train_bench.md;
--crop-size: the teacher's crops at another size than the student's image, e.g. `--crop-size 224 ViT-B-16 2 20 1024` = the reference recipe's
1024^2 student).  env CLIPSELF_ATTN_IDENTITY_ROPE=1: the attention kernels get identity rotary tables instead of none (the A/B switch of
ClipVitEngine.rope_tables; profiles/attn_norope_bench.md) -- the line printed says which form ran.  --rope-ab R: R rounds of `--steps` steps
with the switch on, then off, alternately in this process, one line per window and the medians at the end."""
import os
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clipself_amd.init import synthetic_batch  # noqa: E402
from clipself_amd.open_clip import create_model  # noqa: E402
from clipself_amd.training.clipself import CLIPSelf  # noqa: E402
from clipself_amd.training.optim import FlatAdamW  # noqa: E402
from clipself_amd.training.train import train_step  # noqa: E402

argv = sys.argv[1:]
EXTRACT, n, CROP, AB = "v2", 6, 0, 0
for flag in ("--extract-type", "--steps", "--crop-size", "--rope-ab"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--steps":
            n = int(argv[i + 1])
        elif flag == "--crop-size":
            CROP = int(argv[i + 1])
        elif flag == "--rope-ab":
            AB = int(argv[i + 1])
        else:
            EXTRACT = argv[i + 1]
        del argv[i:i + 2]
assert EXTRACT in ("v1", "v2")
MODEL = argv[0] if argv else "ViT-B-16"
B, K = (int(argv[1]) if len(argv) > 1 else 64), (int(argv[2]) if len(argv) > 2 else 32)
dev = "cuda:0"
student = create_model(MODEL, "", precision="amp_bf16", device=dev)
teacher = create_model(MODEL, "", precision="amp_bf16", device=dev, trainable=False)
cfg = student.visual.cfg
S = int(argv[3]) if len(argv) > 3 else cfg.image_size
plain = len(argv) > 4 and argv[4] == "plain"
if plain:
    teacher.visual.engine.fold_block_ln = teacher.visual.engine.cls_only_last_block = False
if len(argv) > 4 and argv[4] == "nocls":                     # the CLS-only last block with its own LayerNorm pass over the whole stream (round 3 form)
    teacher.visual.engine.fold_cls_block = False
if len(argv) > 4 and argv[4] == "nosplit":                  # the folded schedule with the fp32 stream + bf16 copy instead of the two 16-bit planes
    teacher.visual.engine.split_stream = False
student.lock_image_tower(unlocked_groups=cfg.layers)
student.train(); teacher.eval()
opt = FlatAdamW(student, lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
args = SimpleNamespace(device=dev, precision="amp_bf16", distributed=False, skip_scheduler=True, grad_clip_norm=None, multiscale=False,
                       extract_type=EXTRACT, cosine_weight=1.0)
CROP = CROP or S
batches = [tuple(t.to(dev) for t in synthetic_batch(B, K, S, CROP, seed=5 + j)) for j in range(2)]
method = CLIPSelf()
if AB:
    SW, step, ms = "CLIPSELF_ATTN_IDENTITY_ROPE", 0, {"1": [], "0": []}
    for r in range(AB + 1):                                  # round 0 warms both forms up
        for leg in ("1", "0"):
            os.environ[SW] = leg
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                out, _, _ = train_step(student, method, batches[step % 2], opt, None, step, teacher, args, next_batch=batches[(step + 1) % 2])
                step += 1
            torch.cuda.synchronize()
            if r:
                ms[leg].append(1e3 * (time.perf_counter() - t0) / n)
                print(f"round {r} {'identity tables' if leg == '1' else 'no tables      '}: {ms[leg][-1]:.2f} ms/step", flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(f"{MODEL} extract_type={EXTRACT}: {B} images x {K} crops ({CROP}^2) at {S}^2, {AB} rounds of {n} steps: identity tables median {med['1']:.2f} ms/step "
          f"(min {min(ms['1']):.2f} max {max(ms['1']):.2f}, spread {100 * (max(ms['1']) - min(ms['1'])) / med['1']:.2f} %) | no tables median {med['0']:.2f} "
          f"(min {min(ms['0']):.2f} max {max(ms['0']):.2f}) | no tables / identity {med['0'] / med['1']:.4f}, loss {float(out['loss'].detach()):.4f}", flush=True)
    sys.exit(0)
for i in range(3):
    out, _, _ = train_step(student, method, batches[i % 2], opt, None, i, teacher, args, next_batch=batches[(i + 1) % 2])
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(n):
    out, _, _ = train_step(student, method, batches[(i + 1) % 2], opt, None, 3 + i, teacher, args, next_batch=batches[i % 2])
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
g = S // cfg.patch_size
N, C, Hd, E, L, p = g * g + 1, cfg.width, cfg.hidden, cfg.embed_dim, cfg.layers, cfg.patch_size
pe = 2 * (N - 1) * 3 * p * p * C
blk = 8 * N * C * C + 4 * N * N * C + 4 * N * C * Hd                 # in_proj + out_proj, attention, c_fc + c_proj
blk_na = 4 * N * C * C + 4 * N * C * Hd                                # last dense block: value third of in_proj + out_proj, MLP
blk_cls = 4 * N * C * C + 4 * C * C + 4 * N * C + 4 * C * Hd          # teacher's last block for the CLS query only
if CROP != S:                                                          # the teacher's tower at its own token count
    Nc = (CROP // p) ** 2 + 1
    T = (2 * (Nc - 1) * 3 * p * p * C + (L - 1) * (8 * Nc * C * C + 4 * Nc * Nc * C + 4 * Nc * C * Hd)
         + ((8 * Nc * C * C + 4 * Nc * Nc * C + 4 * Nc * C * Hd) if plain else (4 * Nc * C * C + 4 * C * C + 4 * Nc * C + 4 * C * Hd)) + 2 * C * E)
else:
    T = pe + (L - 1) * blk + (blk if plain else blk_cls) + 2 * C * E
F = K * T + (pe + (L - 1) * blk + blk_na + 2 * (N - 1) * C * E) + 2 * ((L - 1) * blk + blk_na) + 2 * (N - 1) * C * E
tables = "identity rotary tables" if student.visual.engine.rope_tables(g)[0] is not None else "no rotary tables"
print(f"{MODEL}{' (plain teacher schedule)' if plain else ''} extract_type={EXTRACT}, attention with {tables}: {B} images x {K} crops ({CROP}^2) at {S}^2: {1e3 * dt:.1f} ms/step, {B / dt:.1f} images/s, "
      + (f"{F * B / dt / 1e12:.0f} TFLOP/s of executed matmul FLOPs ({F * B / dt / 2.5e15:.1%} of the 2.5 PFLOP/s MFMA peak), " if EXTRACT == "v2" else "")
      + f"loss {float(out['loss'].detach()):.4f}", flush=True)
