"""`-m gpu`: the detector's mask branch on the MI355X (csm_mask_target / csm_mask_loss / csm_paste_masks, HipOps.mask_target / mask_loss /
paste_masks).

The kernels against the restatements of tests/_mask_ref.py, element by element inside the bounds its docstring derives; the two
thresholded outputs equal outside the undecided band; known answers bit for bit (unit boxes, grid-2 boxes with exact ties, dyadic boxes,
logits of -inf / 0 / +inf, zero logits with den = 1024).  Shapes are the smallest at which this layout can still go wrong
(det_mask.hip): masks 37 x 53 with ldm = 64 (rows that start off a 4-byte boundary, a ragged last word), boxes that end on the last row
and column, grids of 1, 2 and >= 4 (more than one staged chunk of rows), M = 4 | 14 | 28 | 64 (8 | 8 | 8 | 4 rows per chunk), M * M = 49
(gradient planes off a 16-byte boundary), a gradient tensor offset by 4 bytes, an image of 40 x 56 (three bands, the last one ragged)
and of 16 x 16 (one band).  The paste's known answers use M = 4 and 16: for a power of two (X + 0.5) / M and every later step of the
coordinate is exact, which M = 28 is not.  Outputs are handed in as NaN / 0xFF, so an element the kernels leave unwritten fails the
comparison; every call is made twice and must return equal bits.  The worst fraction of each bound is printed when the module is done
(pytest -s; profiles/det_masks_parity.md)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mask_ref as R  # noqa: E402

WORST = {}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    yield HipOps()
    for k in sorted(WORST):
        print(f"\nworst fraction of the bound: {k}: {WORST[k]:.4f}", end="")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(shape, dtype, misalign=False):
    """NaN (fp32) or 0xFF (uint8); misalign: the first element sits 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    size = 4 if dtype == torch.float32 else 1
    flat = torch.full((n + 16,), float("nan") if dtype == torch.float32 else 255, dtype=dtype, device="cuda")
    off = 4 // size if misalign else 0
    t = flat[off:off + n]
    assert t.data_ptr() % 16 == (4 if misalign else 0)
    return t.view(shape)


def _np(t):
    return t.cpu().numpy()


def _note(key, frac):
    WORST[key] = max(WORST.get(key, 0.0), frac)


def _padded_masks(masks, ldm):
    G, H, W = masks.shape
    full = torch.full((G, H, ldm), 0xA5, dtype=torch.uint8, device="cuda")     # padding bytes are non-zero: reading one shows
    full[:, :, :W] = _dev(masks)
    return full[:, :, :W]


def target_kernel(hip, c, soft, ldm=None):
    masks = _padded_masks(c["masks"], ldm) if ldm else _dev(c["masks"])
    rois, rows, M = _dev(c["rois"]), _dev(c["gt_rows"]), c["M"]
    runs = []
    for _ in range(2):
        out = _poison((len(c["rois"]), M, M), torch.float32 if soft else torch.uint8)
        runs.append(_np(hip.mask_target(rois, rows, masks, M, soft=soft, out=out)))
    assert R.same_bits(runs[0], runs[1]), "two calls, different targets"
    return runs[0]


# ------------------------------------------------------------------------------------------------ targets
def test_target_known_answers_bit_for_bit(hip):
    masks = R.blob_masks(1, 60, 60, 9, noise=0.2)
    c = dict(masks=masks, rois=np.array([[0, 0, 0, 28, 28], [0, 0, 0, 56, 56]], np.float32), gt_rows=np.zeros(2, np.int32), M=28)
    corner = (masks[0, :28, :28] != 0)
    quads = (masks[0, :56, :56] != 0).reshape(28, 2, 28, 2).sum(axis=(1, 3)) / 4.0
    assert (quads == 0.5).any()
    soft, hard = target_kernel(hip, c, True), target_kernel(hip, c, False)
    assert R.same_bits(soft[0], corner.astype(np.float32)) and R.same_bits(soft[1], quads.astype(np.float32))
    assert R.same_bits(hard[0], corner.astype(np.uint8)) and R.same_bits(hard[1], (quads >= 0.5).astype(np.uint8))     # a tie gives 1


@pytest.mark.parametrize("M", [4, 14])
def test_target_dyadic_boxes_bit_for_bit(hip, M):
    c = R.dyadic_case(M)
    assert c["ref"]["exact"]                                   # checked on the float64 terms: every partial sum is an fp32 number
    assert R.same_bits(target_kernel(hip, c, True), c["ref"]["t"].astype(np.float32))
    assert (c["ref"]["t"] == 0.5).any() and R.binary_target_ok(c["ref"], target_kernel(hip, c, False))      # ties at 1/2 give 1


@pytest.mark.parametrize("name,ldm", [("small", 64), ("large", None)])
def test_target_random_inside_the_bound(hip, name, ldm):
    c = R.target_case(name)
    soft = target_kernel(hip, c, True, ldm)
    ok, frac = R.inside(soft, c["ref"]["t"], c["ref"]["bound"])
    print(name, "soft target: worst fraction of the bound", frac)
    assert ok
    _note("target " + name, frac)
    ok, band = R.binary_check(target_kernel(hip, c, False, ldm), c["ref"]["t"], c["ref"]["bound"], 0.5)
    print(name, "binary target: in the band", band, "of", soft.size)
    assert ok


def test_target_m64_and_m1(hip):
    base = R.target_case("large")
    for M in (64, 1):                                          # four rows per chunk / one bin over the whole box: a grid of up to 128
        c = dict(base, M=M, ref=R.target_vec(base["rois"], base["gt_rows"], base["masks"], M))
        ok, frac = R.inside(target_kernel(hip, c, True), c["ref"]["t"], c["ref"]["bound"])
        print("M", M, "worst fraction of the bound", frac)
        assert ok
        _note(f"target M={M}", frac)


# ------------------------------------------------------------------------------------------------ loss
def loss_kernel(hip, c, grad=True, misalign=False):
    pred, labels, targets, w = _dev(c["pred"]), _dev(c["labels"]), _dev(c["targets"]), _dev(c["w"])
    runs = []
    for _ in range(2):
        out = (_poison((2,), torch.float32), _poison(c["pred"].shape, torch.float32, misalign) if grad else None)
        o2, dp = hip.mask_loss(pred, labels, targets, w, grad=grad, out=out)
        runs.append((_np(o2), _np(dp) if grad else None))
    assert np.array_equal(_np(pred), c["pred"], equal_nan=True), "the predictions were written"
    assert R.same_bits(runs[0][0], runs[1][0]), "two calls, different losses"
    if grad:
        assert R.same_bits(runs[0][1], runs[1][1]), "two calls, different gradients"
    return runs[0]


@pytest.mark.parametrize("name", sorted(R.LOSS_CASES))
def test_loss_and_gradient_inside_the_bounds(hip, name):
    c = R.loss_case(name)
    want = R.loss_ref(c)
    out2, dpred = loss_kernel(hip, c)
    print(name, "out", out2, "want", want["out"], "bound", want["out_bound"])
    assert np.isfinite(out2).all() and float(out2[1]) == want["out"][1]
    ok, frac = R.inside(out2[0], want["out"][0], want["out_bound"][0])
    assert ok, frac
    _note("loss", frac)
    ok, frac = R.inside(dpred, want["dpred"], want["dpred_bound"])
    print(name, "dpred: worst fraction of the bound", frac)
    assert ok
    _note("dpred", frac)
    fwd, _ = loss_kernel(hip, c, grad=False)
    assert R.same_bits(fwd, out2), "a forward-only call gives other bits"


@pytest.mark.parametrize("name", ["R7_C1", "C3_odd", "M64"])
def test_loss_misaligned_gradient_gives_the_same_bits(hip, name):
    c = R.loss_case(name)
    a, b = loss_kernel(hip, c), loss_kernel(hip, c, misalign=True)
    assert R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1])


def test_loss_zero_logits_known_answer(hip):
    """M = 16, four counted rows of five, zero logits: den = 1024, loss = ln 2 within its bound, gradients (0.5 - t) / 1024 bit for bit."""
    rng = np.random.default_rng(3)
    c = dict(R=5, C=1, M=16, pred=np.zeros((5, 1, 16, 16), np.float32), labels=None, targets=(rng.random((5, 16, 16)) < 0.5).astype(np.uint8),
             w=np.array([1, 1, 0, 1, 1], np.float32))
    want = R.loss_ref(c)
    out2, dpred = loss_kernel(hip, c)
    assert float(out2[1]) == 4.0 and abs(want["out"][0] - np.log(2.0)) < 1e-15
    ok, frac = R.inside(out2[0], want["out"][0], want["out_bound"][0])
    print("loss", out2[0], "ln 2", np.log(2.0), "fraction of the bound", frac)
    assert ok
    g = ((0.5 - c["targets"].astype(np.float32)) / np.float32(1024.0)) * c["w"][:, None, None]
    assert R.same_bits(dpred[:, 0], g.astype(np.float32) + np.float32(0))      # + 0: the zero rows are +0, as the kernel writes them


def test_loss_autograd_is_the_kernels_gradient_times_the_upstream(hip):
    from clipself_amd import det_masks as DM
    c = R.loss_case("C3_labels")
    _, dpred = loss_kernel(hip, c)
    pred = _dev(c["pred"]).requires_grad_(True)
    out = DM.mask_loss(pred, _dev(c["targets"]), _dev(c["labels"]), _dev(c["w"]), class_agnostic=False,
                       loss_mask=dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0), ops=hip, fused=True)
    (out["loss_mask"] * 0.75).backward()
    assert R.same_bits(_np(pred.grad), dpred * np.float32(0.75))


# ------------------------------------------------------------------------------------------------ paste
def paste_kernel(hip, logits, labels, boxes, img_h, img_w, thr=0.5):
    lg, lb, bx = _dev(logits), _dev(labels), _dev(boxes)
    runs = []
    for with_soft in (True, True, False):
        out = _poison((len(boxes), img_h, img_w), torch.uint8)
        soft = _poison((len(boxes), img_h, img_w), torch.float32) if with_soft else None
        hip.paste_masks(lg, lb, bx, img_h, img_w, thr, out=out, soft=soft)
        runs.append((_np(out), _np(soft) if with_soft else None))
    assert R.same_bits(runs[0][0], runs[1][0]) and R.same_bits(runs[0][1], runs[1][1]), "two calls, different masks"
    assert R.same_bits(runs[0][0], runs[2][0]), "soft = NULL gives other bytes"
    return runs[0]


@pytest.mark.parametrize("M", [4, 16])
def test_paste_known_answers_bit_for_bit(hip, M):
    rng = np.random.default_rng(5)
    logits = rng.choice([-np.inf, 0.0, np.inf], size=(2, 1, M, M)).astype(np.float32)
    p = np.where(logits[:, 0] > 0, 1.0, np.where(logits[:, 0] < 0, 0.0, 0.5))
    out, soft = paste_kernel(hip, logits, None, np.array([[0, 0, M, M]] * 2, np.float32), M, M)
    assert R.same_bits(soft, p.astype(np.float32)) and R.same_bits(out, (p >= 0.5).astype(np.uint8))      # the identity; a tie gives 1
    boxes2 = np.array([[0, 0, 2 * M, 2 * M]] * 2, np.float32)
    ref2 = R.paste_ref(logits, None, boxes2, 2 * M, 2 * M)
    assert (p == 0.5).any() and (ref2["v"] * 32 == np.round(ref2["v"] * 32)).all()                        # ties above; quarter weights: exact
    out2, soft2 = paste_kernel(hip, logits, None, boxes2, 2 * M, 2 * M)
    assert R.same_bits(soft2, ref2["v"].astype(np.float32)) and R.same_bits(out2, (ref2["v"] >= 0.5).astype(np.uint8))


@pytest.mark.parametrize("name", R.PASTE_RANDOM)
def test_paste_random_inside_the_bound(hip, name):
    c = R.paste_case(name)
    out, soft = paste_kernel(hip, c["logits"], c["labels"], c["boxes"], c["img_h"], c["img_w"], c["thr"])
    ok, frac = R.inside(soft, c["ref"]["v"], c["ref"]["bound"])
    print(name, "soft paste: worst fraction of the bound", frac)
    assert ok
    _note("paste " + name, frac)
    ok, band = R.binary_check(out, c["ref"]["v"], c["ref"]["bound"], c["thr"])
    print(name, "binary paste: in the band", band, "of", out.size)
    assert ok
    assert out[c["zero"]].max() == 0 and out[c["live"]].max() == 1      # bad label, outside, zero extent, NaN; the live box


def test_arguments_outside_the_limits_are_refused(hip):
    c = R.paste_case("m4")
    with pytest.raises(RuntimeError):
        hip.paste_masks(_dev(c["logits"]), _dev(c["labels"]), _dev(c["boxes"]), 40, 56, -1.0)
    with pytest.raises(ValueError):
        hip.mask_target(_dev(np.zeros((1, 5), np.float32)), _dev(np.zeros(1, np.int32)), torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), 65)


# ------------------------------------------------------------------------------------------------ extents
def _extent_cases():
    tc, lc, pc = R.target_case("small"), R.loss_case("C3_odd"), R.paste_case("m4")
    G, H, W = tc["masks"].shape

    def target(soft):
        def fn(ops, a):
            m2 = a.inp(torch.from_numpy(tc["masks"].reshape(G * H, W)).to(a.dev), a.ld(W))          # the padded ldm in the halo run
            masks = m2.unflatten(0, (G, H))
            out = a.out((len(tc["rois"]), tc["M"], tc["M"]), torch.float32 if soft else torch.uint8)
            ops.mask_target(a.inp(torch.from_numpy(tc["rois"]).to(a.dev)), a.inp(torch.from_numpy(tc["gt_rows"]).to(a.dev)), masks, tc["M"],
                            soft=soft, out=out)
            return {"targets": out}
        return fn

    def loss(grad):
        def fn(ops, a):
            out2 = a.out((2,), torch.float32)
            dpred = a.out(lc["pred"].shape, torch.float32) if grad else None
            ws = a.ws(ops.mask_workspace(lc["R"]))
            ops.mask_loss(a.inp(torch.from_numpy(lc["pred"]).to(a.dev)), a.inp(torch.from_numpy(lc["labels"]).to(a.dev)),
                          a.inp(torch.from_numpy(lc["targets"]).to(a.dev)), a.inp(torch.from_numpy(lc["w"]).to(a.dev)), grad=grad,
                          out=(out2, dpred), workspace=ws)
            return {"out": out2, "dpred": dpred} if grad else {"out": out2}
        return fn

    def paste(with_soft):
        def fn(ops, a):
            shape = (len(pc["boxes"]), pc["img_h"], pc["img_w"])
            out = a.out(shape, torch.uint8)
            soft = a.out(shape, torch.float32) if with_soft else None
            ops.paste_masks(a.inp(torch.from_numpy(pc["logits"]).to(a.dev)), a.inp(torch.from_numpy(pc["labels"]).to(a.dev)),
                            a.inp(torch.from_numpy(pc["boxes"]).to(a.dev)), pc["img_h"], pc["img_w"], pc["thr"], out=out, soft=soft)
            return {"out": out, "soft": soft} if with_soft else {"out": out}
        return fn

    return {"mask_target.u8": target(False), "mask_target.soft": target(True), "mask_loss.grad": loss(True), "mask_loss.fwd": loss(False),
            "paste_masks": paste(False), "paste_masks.soft": paste(True)}


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("name", ["mask_target.u8", "mask_target.soft", "mask_loss.grad", "mask_loss.fwd", "paste_masks", "paste_masks.soft"])
def test_extents_poisoned_halo(hip, name, pad):
    from _extents import run_case
    problems = run_case(hip, _extent_cases()[name], "cuda", pad, key="det_masks." + name)
    assert not problems, problems
