"""One digest per detector entry point, for comparing two builds of libclipself_hip.so bit for bit.

Every entry point of the detector kernels (det_post, det_assign, det_loss, det_mask, det_proposal, roi_extract) runs once on fixed-seed
random fp32 inputs -- generic values, no lattice, so a product fused into a sum (or un-fused) moves a digest -- and the tool prints
`name sha256(output bytes)`.  The inputs are drawn on the CPU, so two processes see the same bytes.

usage (GPU box), one fresh process per library:
    python tools/det_ab_bits.py > branch.txt
    CLIPSELF_HIP_LIB=<other libclipself_hip.so> python tools/det_ab_bits.py > other.txt
    diff branch.txt other.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipself_amd.hip import HipOps  # noqa: E402

G = torch.Generator().manual_seed(20240607)
DEV = "cuda"


def randn(*shape):
    return torch.randn(*shape, generator=G)


def rand(*shape):
    return torch.rand(*shape, generator=G)


def randint(lo, hi, shape, dtype=torch.int32):
    return torch.randint(lo, hi, tuple(shape), generator=G).to(dtype)


def boxes_in(n, side, lo=4.0, hi=96.0):
    """n boxes with generic fp32 corners inside (roughly) a side x side image"""
    ctr = rand(n, 2) * side
    half = rand(n, 2) * (hi - lo) * 0.5 + lo * 0.5
    return torch.cat([ctr - half, ctr + half], dim=1)


def digest(name, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print(f"{name:28s} {h.hexdigest()}", flush=True)


def starts_of(B, per):
    return torch.arange(B + 1, dtype=torch.int32) * per


def main():
    ops = HipOps()
    d = lambda t: t.to(DEV)
    means, stds = (0.05, -0.1, 0.2, -0.15), (0.5, 0.6, 1.1, 0.9)

    # ---- nms at Kmax 4096 with groups, and the multi-class form
    B, K = 2, 4096
    bx, sc = d(boxes_in(B * K, 800.0)), d(rand(B * K, 1))
    grp = d(randint(0, 5, (B * K,)))
    digest("nms_group_k4096", *ops.nms(bx, sc, d(starts_of(B, K)), K, 0.05, 0.7, 1000, grp, 5))
    C = 6
    digest("nms_multiclass", *ops.nms(bx[:2 * 1500], d(rand(2 * 1500, C)), d(starts_of(2, 1500)), 1500, 0.3, 0.5, 100))

    # ---- delta2bbox with clamp, clip and rescale
    K = 3000
    rois, dl = d(boxes_in(2 * K, 640.0)), d(randn(2 * K, 4))
    ms, sf = d(torch.tensor([[480.0, 600.0], [512.0, 640.0]])), d(rand(2, 4) + 0.5)
    digest("delta2bbox", ops.delta2bbox(rois, dl, torch.empty_like(rois), means, stds, 0.5, d(starts_of(2, K)), ms, sf))
    digest("delta2bbox_plain", ops.delta2bbox(rois, dl * 0.1, torch.empty_like(rois)))

    # ---- assign (both low-quality forms), sample, bbox_targets
    B, N, Gm = 2, 4000, 24
    ab, gt = d(boxes_in(B * N, 640.0)), d(boxes_in(B * Gm, 640.0, 20.0, 240.0))
    st, gst = d(starts_of(B, N)), d(starts_of(B, Gm))
    gi_all, ov_all = ops.assign(ab, st, gt, gst, B, N, Gm, 0.5, 0.4, 0.1, True, True)
    digest("assign_lowq_all", gi_all, ov_all)
    gi_row, ov_row = ops.assign(ab, st, gt, gst, B, N, Gm, 0.5, (0.05, 0.4), 0.1, True, False)
    digest("assign_lowq_row", gi_row, ov_row)
    digest("assign_shared_rows", *ops.assign(ab[:N], None, gt, gst, B, N, Gm, 0.6, 0.3, 0.0, False))
    keys = d(randint(-(1 << 31), 1 << 31, (B, N), torch.int64).to(torch.int32))
    flags, sel, counts = ops.sample(gi_all, keys, st, B * N, gst, B * Gm, Gm, 256, 128)
    digest("sample", flags, sel, counts)
    gl = d(randint(0, 80, (B * Gm,)))
    digest("bbox_targets_dense", *ops.bbox_targets(ab, st, gt, None, gst, Gm, gi_all, flags=flags, means=means, stds=stds))
    digest("bbox_targets_compact", *ops.bbox_targets(ab, st, gt, gl, gst, Gm, gi_all, sel=sel, means=means, stds=stds, bg_label=80))

    # ---- rpn_select: a long list (the select passes) and a short one
    A = 3
    dims = [(40, 48), (10, 12)]
    cls = [d(randn(2, A, h, w)) for h, w in dims]
    reg = [d(randn(2, 4 * A, h, w)) for h, w in dims]
    anc = d(boxes_in(sum(h * w * A for h, w in dims), 640.0))
    digest("rpn_select_long_short", *ops.rpn_select(cls, reg, anc, 1000, means, stds, 0.5, ms, 8.0))
    digest("rpn_select_pre4096", *ops.rpn_select(cls, [r * 0.1 for r in reg], anc, 4096, (0.0,) * 4, (1.0,) * 4, 16 / 1000, None, -1.0))

    # ---- mask_target, mask_loss, paste_masks
    R, Gt, H, W, M = 300, 12, 200, 304, 28
    masks = d((rand(Gt, H, W) > 0.5).to(torch.uint8))
    mr = torch.cat([torch.zeros(R, 1), boxes_in(R, 280.0, 8.0, 160.0)], dim=1)
    rows = d(randint(-1, Gt, (R,)))
    hard = ops.mask_target(d(mr), rows, masks, M)
    soft = ops.mask_target(d(mr), rows, masks, M, soft=True)
    digest("mask_target", hard)
    digest("mask_target_soft", soft)
    Cm = 3
    pred, rw = d(randn(R, Cm, M, M) * 3.0), d((rand(R) > 0.3).float() * (rand(R) + 0.5))
    out2, dpred = ops.mask_loss(pred, d(randint(0, Cm, (R,))), soft, rw)
    digest("mask_loss_soft", out2, dpred)
    out2, dpred = ops.mask_loss(pred[:, :1].contiguous(), None, hard, rw)
    digest("mask_loss_hard", out2, dpred)
    Nd, ih, iw = 40, 180, 260
    pb = d(boxes_in(Nd, 240.0, 10.0, 150.0))
    soft_out = torch.empty(Nd, ih, iw, device=DEV)
    digest("paste_masks", ops.paste_masks(pred[:Nd], d(randint(0, Cm, (Nd,))), pb, ih, iw, 0.5, soft=soft_out), soft_out)

    # ---- roi_extract forward and backward
    B, Cc, P, K = 2, 64, 7, 2000
    grids, scales = [(64, 80), (32, 40), (16, 20), (8, 10)], [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    maps = [d(randn(B * h * w, Cc)) for h, w in grids]
    rr = torch.cat([randint(0, B, (K, 1), torch.float32), boxes_in(K, 300.0, 4.0, 300.0)], dim=1)
    out = torch.empty(K * P * P, Cc, device=DEV)
    digest("roi_extract_fwd", ops.roi_extract_fwd(maps, grids, scales, d(rr), out, B, P))
    digest("roi_extract_fwd_sr2", ops.roi_extract_fwd(maps, grids, scales, d(rr), torch.empty_like(out), B, P, sampling_ratio=2))
    dmaps = [torch.zeros_like(m) for m in maps]
    ops.roi_extract_bwd(d(randn(K * P * P, Cc)), d(rr), dmaps, grids, scales, B, P)
    digest("roi_extract_bwd", *dmaps)

    # ---- rpn_loss, bbox_head_loss
    Nn = sum(h * w * A for h, w in dims)
    lab = d(randint(0, 2, (2, Nn)))
    lw, bw = d((rand(2, Nn) > 0.5).float()), d((rand(2, Nn, 4) > 0.7).float())
    losses, dcls, dreg = ops.rpn_loss(cls, reg, lab, lw, d(randn(2, Nn, 4)), bw, d(torch.tensor([256.0])))
    digest("rpn_loss", losses, *dcls, *dreg)
    R, C1 = 2048, 81
    out4, dc, db = ops.bbox_head_loss(d(randn(R, C1) * 4.0), d(randint(0, C1, (R,))), d((rand(R) > 0.2).float()), d(randn(R, 4)), d(randn(R, 4)),
                                      d((rand(R, 4) > 0.5).float()), C1 - 1, d(rand(C1) + 0.5))
    digest("bbox_head_loss", out4, dc, db)


if __name__ == "__main__":
    main()
