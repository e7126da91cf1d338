"""Times the thin 1 x 1 convolutions of the detector's RPN and mask heads (epilogues 10 / 11 of cs_gemm_nt, conv.Conv1x1Thin,
conv.thin_heads) and the two modules built on them (rpn_head.RPNHead, mask_head.FCNMaskHead) on the MI355X, against the same layers as
nn.Conv2d / nn.ConvTranspose2d (the modules' own torch route, fused=False) in fp32 on NCHW, the form the detector runs, and under bf16
autocast on channels-last inputs.  The yardstick is torch's route, never the new kernels against themselves.

Shapes (B = 8, 256 channels, A = 3 anchors: 3 + 12 output channels):
  rpn640 / rpn1024    the two heads at level 0 of a 640 x 640 (160 x 160) and a 1024 x 1024 (256 x 256) image, forward + backward
  head640 / head1024  a whole RPNHead (num_convs = 2, SyncBN) over the five levels 160 .. 10 / 256 .. 16
  mask                the mask head's tail (deconvolution + ReLU + logits) and the whole FCNMaskHead (4 convs, SyncBN, class-agnostic) at
                      1024 RoIs of 14 x 14: the 8 x 128 positive slots of training
and the two kernels alone at those row counts, with GB/s beside the 6.3 TB/s stream figure of profiles/fpn_bench.md over the bytes they
must move (the K-wide rows once plus the thin side; the gate's read is listed apart), and the weight / bias gradient of the heads
(cs_gemm_wgrad_tn at N = 16 + cs_colsum_bf16 + the dY rows) as a share of the heads' backward.

Method (measuring-on-mi355x): every variant is warmed up; a window is `--iters` calls between two device events; the variants alternate
window by window inside one process; `--windows` windows, the median and the spread (min .. max) are reported.  Prints markdown tables
and the verdict conv.FUSED_THIN_DEFAULT rests on."""
import argparse
import contextlib
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

STREAM_TBS = 6.3
BF16, F32 = torch.bfloat16, torch.float32
B, C, A = 8, 256, 3
ANCHORS = dict(scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64])
NORM = dict(type="SyncBN", requires_grad=True)


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
    """One forward + backward of fn(leaves) -> tensors, with an upstream gradient of ones (prepared once per output)."""
    ones = {}

    def run():
        for t in leaves:
            t.grad = None
        for p in params:
            p.grad = None
        with autocast(amp):
            outs = fn(leaves)
        outs = [o for o in outs]
        gs = []
        for i, o in enumerate(outs):
            if i not in ones:
                ones[i] = torch.ones_like(o)
            gs.append(ones[i])
        torch.autograd.backward(outs, gs)
    return run


def flat(out):
    return list(out[0]) + list(out[1]) if isinstance(out, tuple) else [out]


def variants_of(make, shapes, kernel_layouts):
    """{name: step} of a module: the kernel route on each of kernel_layouts, torch fp32 NCHW, torch bf16 autocast channels-last."""
    torch.manual_seed(0)
    out = {}
    for name, dtype, cl in kernel_layouts:
        m = make(True).cuda().train()
        xs = [torch.randn(s, device="cuda").to(dtype) for s in shapes]
        if cl:
            xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
        xs = [x.requires_grad_(True) for x in xs]
        out[name] = step(lambda leaves, m=m: flat(m(leaves) if len(shapes) > 1 else m(leaves[0])), xs, list(m.parameters()))
    m32 = make(False).cuda().train()
    xs = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
    out["torch fp32, NCHW"] = step(lambda leaves: flat(m32(leaves) if len(shapes) > 1 else m32(leaves[0])), xs, list(m32.parameters()))
    mcl = make(False).cuda().train().to(memory_format=torch.channels_last)
    xc = [torch.randn(s, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True) for s in shapes]
    out["torch bf16 autocast, channels-last"] = step(lambda leaves: flat(mcl(leaves) if len(shapes) > 1 else mcl(leaves[0])), xc,
                                                     list(mcl.parameters()), amp=True)
    return out


class Pair(torch.nn.Module):
    """rpn_cls | rpn_reg of one level."""

    def __init__(self, ops, fused):
        super().__init__()
        from clipself_amd.conv import Conv1x1Thin
        self.cls, self.reg = Conv1x1Thin(C, A, ops=ops, fused=fused), Conv1x1Thin(C, 4 * A, ops=ops, fused=fused)

    def forward(self, x):
        from clipself_amd.conv import thin_heads
        return thin_heads(x, (self.cls, self.reg))


class Tail(torch.nn.Module):
    """upsample + ReLU + conv_logits of the mask head."""

    def __init__(self, ops, fused):
        super().__init__()
        from clipself_amd.mask_head import FCNMaskHead
        self.head = FCNMaskHead(num_convs=0, in_channels=C, conv_out_channels=C, class_agnostic=True, ops=ops, fused=fused)

    def forward(self, x):
        return self.head(x)


def kernels_alone(ops, M, N, R, split, iters, windows, gate):
    """The two kernels at M rows of 256 channels -> rows of the bandwidth table."""
    W = (torch.randn(N, C, device="cuda") * C ** -0.5).to(BF16)
    bias = torch.randn(N, device="cuda")
    rows = []
    for dt in (BF16, F32):
        X = torch.randn(M, C, device="cuda").to(dt)
        Y = torch.empty(M * N, device="cuda") if R else torch.empty(M, N, device="cuda")
        dX = torch.empty(M, C, device="cuda", dtype=dt)
        d1 = Y[:M * split] if R and split < N else Y
        d2 = Y[M * split:] if R and split < N else None
        g = torch.randn(M, C, device="cuda").to(BF16) if gate and dt == BF16 else None
        fns = {"fwd": lambda: ops.thin_fwd(X, W, bias, Y, R=R, split=split if R and split < N else None),
               "dgrad": lambda: ops.thin_dgrad(d1, W, dX, R=R, dY2=d2)}
        if g is not None:
            fns["dgrad + gate"] = lambda: ops.thin_dgrad(d1, W, dX, R=R, dY2=d2, gate=g)
        t = measure(fns, iters, windows)
        esz = 2 if dt == BF16 else 4
        for k, v in t.items():
            must = M * C * esz + M * N * 4
            moved = must + (M * C * 2 if "gate" in k else 0)
            us = statistics.median(v)
            rows.append((f"M = {M}, N = {N}, {'planes' if R else 'rows'}, {str(dt).split('.')[-1]} rows: {k}", fmt(v), must / 1e6,
                         must / us / 1e3, must / us / 1e6 / STREAM_TBS * 100, moved / us / 1e3))
    return rows


def wgrad_alone(ops, conv_mod, name, M, N, K, geom, split, dt, iters, windows):
    """Parameter gradients alone at M rows: epilogue 12 (HipOps.thin_wgrad, dY and X read in place) against the route it replaces --
    dy_rows16 / a padded bf16 copy of dY [+ cast_f32_bf16] + cs_gemm_wgrad_tn at N = 16 + cs_colsum_bf16 (conv.thin_param_grads with
    R=None, whatever conv.THIN_WGRAD_DEFAULT says).  geom = (B, H, W) for the planes form, None for rows.  -> a table row."""
    from clipself_amd.conv import Conv1x1Thin
    holder = Conv1x1Thin(K, N, ops=ops, fused=True).cuda()
    X = torch.randn(M, K, device="cuda").to(dt)
    dW, db = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    ws = ops.empty((ops.thin_wgrad_workspace(M, N, K),), F32)
    if geom is not None:
        Bn, H, Wd = geom
        widths = [split, N - split]
        grads = [torch.randn(Bn, n, H, Wd, device="cuda") for n in widths]
        new = lambda: ops.thin_wgrad(grads[0], X, dW, db=db, R=H * Wd, dY2=grads[1], workspace=ws)

        def old():
            dYr = conv_mod.dy_rows16(ops, grads, M)
            Xb = X
            if dt != BF16:
                Xb = ops.empty((M, K), BF16)
                ops.cast_f32_bf16(X, Xb)
            conv_mod.thin_param_grads(ops, holder, dYr, Xb, widths, [(True, True)] * 2)
    else:
        dL = torch.randn(M, N, device="cuda")
        new = lambda: ops.thin_wgrad(dL, X, dW, db=db, R=0, workspace=ws)

        def old():
            dYr = ops.zeros((M, 16), BF16)
            dYr[:, :N] = dL
            Xb = X
            if dt != BF16:
                Xb = ops.empty((M, K), BF16)
                ops.cast_f32_bf16(X, Xb)
            conv_mod.thin_param_grads(ops, holder, dYr, Xb, [N], [(True, True)])
    t = measure({"new": new, "old": old}, iters, windows)
    must = M * K * (2 if dt == BF16 else 4) + M * N * 4
    un, uo = statistics.median(t["new"]), statistics.median(t["old"])
    faster = max(t["new"]) < min(t["old"])
    return (f"{name}: M = {M}, N = {N}, K = {K}, {'planes' if geom else 'rows'}, {str(dt).split('.')[-1]} X", fmt(t["new"]), fmt(t["old"]), must / 1e6,
            must / un / 1e6 / STREAM_TBS * 100, uo / un, faster)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated subset of: kernels, wgrad, fcreg, rpn640, rpn1024, head640, head1024, mask")
    ap.add_argument("--route", choices=["default", "new", "old"], default="default",
                    help="parameter gradients of the module tables: conv.THIN_WGRAD_DEFAULT as it is, forced on (epilogue 12) or off (the padded route)")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    want = lambda k: not only or k in only

    from clipself_amd import conv as conv_mod
    from clipself_amd.hip import HipOps
    from clipself_amd.mask_head import FCNMaskHead
    from clipself_amd.rpn_head import RPNHead
    ops = HipOps()
    if args.route != "default":
        conv_mod.THIN_WGRAD_DEFAULT = args.route == "new"
    print(f"# thin heads on {torch.cuda.get_device_name(0)}: {args.windows} windows of {args.iters} calls, variants alternated in one process; "
          f"parameter gradients of the modules: {'epilogue 12' if conv_mod.thin_wgrad_direct(ops) else 'the padded route'}")
    wins = []

    if want("wgrad"):
        rows = []
        for side in (160, 256):
            for dt in (BF16, F32):
                rows.append(wgrad_alone(ops, conv_mod, f"rpn{side * 4}", B * side * side, 15, C, (B, side, side), 3, dt, args.iters, args.windows))
        rows.append(wgrad_alone(ops, conv_mod, "mask tail", 4 * 1024 * 196, 1, C, None, 1, BF16, args.iters, args.windows))
        rows.append(wgrad_alone(ops, conv_mod, "fc_reg", 4096, 4, 1024, None, 4, BF16, args.iters, args.windows))
        print(f"\n## Parameter gradients alone: epilogue 12 against the padded route ({STREAM_TBS} TB/s stream figure)\n\n| shape | new µs median "
              "(min .. max) | old µs median (min .. max) | MB it must move (X + dY) | new: % of the stream figure | old / new | spreads apart |"
              "\n|---|---|---|---|---|---|---|")
        for name, tn, to, mb, pct, ratio, faster in rows:
            print(f"| {name} | {tn} | {to} | {mb:.1f} | {pct:.0f} | {ratio:.2f} x | {'yes' if faster else 'NO'} |")
        print(f"\nTHIN_WGRAD_DEFAULT by the rule (faster at every shape, spreads apart): {all(r[-1] for r in rows)}; "
              f"it is {conv_mod.THIN_WGRAD_DEFAULT} in clipself_amd/conv.py" + ("" if args.route == "default" else f" (forced {args.route} for this run)"))

    if want("fcreg"):
        from clipself_amd.bbox_head import ConvFCBBoxHead
        cfg = dict(in_channels=256, fc_out_channels=512, roi_feat_size=7, num_classes=1203, reg_class_agnostic=True,
                   norm_cfg=dict(type="SyncBN"), num_shared_convs=4, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1)
        torch.manual_seed(0)
        heads = {"all kernels, fused_reg=True (fc_reg on LinearThin)": ConvFCBBoxHead(ops=ops, fused=True, fused_reg=True, **cfg).cuda(),
                 "all kernels, fused_reg=False (fc_reg on F.linear)": ConvFCBBoxHead(ops=ops, fused=True, fused_reg=False, **cfg).cuda()}
        x = torch.randn(4096, 256, 7, 7, generator=torch.Generator().manual_seed(1)).cuda().contiguous(memory_format=torch.channels_last)
        xg = x.clone().requires_grad_(True)

        def head_step(h):
            def run():
                xg.grad = None
                for p in h.parameters():
                    p.grad = None
                x_cls, bbox_pred = h(xg)
                (x_cls.sum() + bbox_pred.sum()).backward()
            return run
        t = measure({k: head_step(h) for k, h in heads.items()}, max(2, args.iters // 3), args.windows)
        print("\n## ConvFCBBoxHead forward + backward, 8 x 512 RoIs [4096, 256, 7, 7] fp32 channel-last\n\n| variant | µs median (min .. max) |\n|---|---|")
        for k, v in t.items():
            print(f"| {k} | {fmt(v)} |")
        del heads, x, xg
        torch.cuda.empty_cache()

    if want("kernels"):
        rows = []
        for side in (160, 256):
            rows += kernels_alone(ops, B * side * side, 15, side * side, 3, args.iters, args.windows, gate=False)
        rows += kernels_alone(ops, 4 * 1024 * 196, 1, 0, 1, args.iters, args.windows, gate=True)
        print(f"\n## The kernels alone ({STREAM_TBS} TB/s stream figure)\n\n| call | µs median (min .. max) | MB it must move | GB/s | % of the "
              "stream figure | GB/s with the gate's read |\n|---|---|---|---|---|---|")
        for name, t, mb, gbs, pct, gbs_all in rows:
            print(f"| {name} | {t} | {mb:.0f} | {gbs:.0f} | {pct:.0f} | {gbs_all:.0f} |")

    layouts = [("kernels, fp32 channel-last map (what BatchNormAct2d returns)", F32, True), ("kernels, bf16 channel-last map", BF16, True),
               ("kernels, fp32 NCHW map (rows conversion in front)", F32, False)]
    for key, side in (("rpn640", 160), ("rpn1024", 256)):
        if want(key):
            v = variants_of(lambda fused: Pair(ops, fused), [(B, C, side, side)], layouts)
            med, best = table(f"## {key}: rpn_cls | rpn_reg at [{B}, {C}, {side}, {side}], forward + backward", measure(v, args.iters, args.windows),
                              ["torch fp32, NCHW", "torch bf16 autocast, channels-last"])
            wins.append((key, best / med[layouts[0][0]]))
            # the parameter gradients' share of the kernel route's backward
            m = Pair(ops, True).cuda()
            x = torch.randn(B, C, side, side, device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
            X = x.permute(0, 2, 3, 1).reshape(-1, C)
            gs = [torch.ones(B, n, side, side, device="cuda") for n in (A, 4 * A)]
            Wp, _ = conv_mod._thin_packed((m.cls, m.reg))
            dX = torch.empty_like(X)

            def params():
                dYr = conv_mod.dy_rows16(ops, gs, X.shape[0])
                conv_mod.thin_param_grads(ops, m.cls, dYr, X, [A, 4 * A], [(True, True)] * 2)
            t = measure({"thin_dgrad": lambda: ops.thin_dgrad(gs[0], Wp, dX, R=side * side, dY2=gs[1]), "dY rows + wgrad_tn (N = 16) + colsum": params},
                        args.iters, args.windows)
            a, b = statistics.median(t["thin_dgrad"]), statistics.median(t["dY rows + wgrad_tn (N = 16) + colsum"])
            print(f"\nbackward of the pair on bf16 rows: input gradient {fmt(t['thin_dgrad'])} µs, weight + bias gradients "
                  f"{fmt(t['dY rows + wgrad_tn (N = 16) + colsum'])} µs = {b / (a + b) * 100:.0f} % of the two")

    for key, side in (("head640", 160), ("head1024", 256)):
        if want(key):
            shapes = [(B, C, side >> l, side >> l) for l in range(5)]
            v = variants_of(lambda fused: RPNHead(C, C, anchor_generator=ANCHORS, num_convs=2, norm_cfg=NORM, ops=ops, fused=fused), shapes,
                            [("kernels, fp32 NCHW maps (what fpn.FPN's torch route returns)", F32, False), ("kernels, fp32 channel-last maps", F32, True)])
            med, best = table(f"## {key}: RPNHead(num_convs=2, SyncBN) over five levels from {side} x {side}, forward + backward",
                              measure(v, max(2, args.iters // 2), args.windows), ["torch fp32, NCHW", "torch bf16 autocast, channels-last"])
            wins.append((key, best / med["kernels, fp32 channel-last maps"]))

    if want("mask"):
        K = 1024
        v = variants_of(lambda fused: Tail(ops, fused), [(K, C, 14, 14)],
                        [("kernels, fp32 channel-last map", F32, True), ("kernels, bf16 channel-last map", BF16, True)])
        med, best = table(f"## mask tail: upsample + ReLU + conv_logits at [{K}, {C}, 14, 14], forward + backward", measure(v, args.iters, args.windows),
                          ["torch fp32, NCHW", "torch bf16 autocast, channels-last"])
        wins.append(("mask tail", best / med["kernels, fp32 channel-last map"]))
        v = variants_of(lambda fused: FCNMaskHead(num_convs=4, in_channels=C, conv_out_channels=C, class_agnostic=True, norm_cfg=NORM, ops=ops, fused=fused),
                        [(K, C, 14, 14)], [("kernels, fp32 NCHW map (the RoI extractor's output)", F32, False)])
        med, best = table(f"## FCNMaskHead(4 convs, SyncBN, class-agnostic) at [{K}, {C}, 14, 14], forward + backward",
                          measure(v, max(2, args.iters // 2), args.windows), ["torch fp32, NCHW", "torch bf16 autocast, channels-last"])
        wins.append(("mask head", best / med["kernels, fp32 NCHW map (the RoI extractor's output)"]))

    if wins:
        print("\n## Verdict\n")
        for k, r in wins:
            print(f"- {k}: faster torch variant / kernel route = {r:.2f} x")
        print(f"- FUSED_THIN_DEFAULT would be {'on' if all(r > 1.0 for _, r in wins) else 'off'} by the rule (a win at every measured shape); "
              f"it is {conv_mod.FUSED_THIN_DEFAULT} in clipself_amd/conv.py")


if __name__ == "__main__":
    main()
