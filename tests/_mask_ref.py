"""TEST INFRASTRUCTURE -- restatements of the mask-branch contract (include/clipself_mask.h), tested against each other on the CPU
(tests/test_det_masks_cpu.py), and the bounds the GPU tests use (tests/test_gpu_det_masks.py).

What is restated, by the published function names (mmdet 2.28.1 / mmcv 1.x; neither package is available to this project, so this
boundary is parity-unpinned in the sense of DESIGN.md §3.13 - §3.17: the restatement follows the published sources as read):

  mask_target_single / BitmapMasks.crop_and_resize -> mmcv roi_align(aligned=True, spatial_scale=1, sampling_ratio=0, 'avg') on the one
      ground-truth plane, after np.clip of the box                                              -> target_loops, target_vec
  mask_cross_entropy: F.binary_cross_entropy_with_logits(pred[arange, labels], target, reduction='mean') on the positive rows
      (a) torch float64 with autograd -> loss_mmdet;  (b) closed form numpy float64 with the header's departures -> loss_ref
  _do_paste_mask(skip_empty=False): F.grid_sample(masks, grid, align_corners=False) of the sigmoid, torch float64 on the CPU; the
      normalised coordinates gx, gy are computed in np.float32 exactly as the header says and handed over as fixed numbers -> paste_ref

Coordinates and axis weights of the target are np.float32, one operation at a time (the helpers of tests/_roi_extract_ref.py); they are
then fixed numbers, the weight of a tap is the exact product of its two axis weights, and the sums are float64.

Bounds.  u = 2^-24 is the fp32 unit roundoff; a sum of n non-negative fp32 terms in ANY order errs by at most (n - 1) u relative; the
device library documents expf and log1pf at 1 ulp = 2u relative.  Nothing below is tuned to a measurement.

  Target, bin (ph, pw) of a box with grids gh, gw; all terms are >= 0, so S = t itself.  In the kernel's stated (separable) order:
    Wx[x]: at most 2 gw tap weights added                          (2 gw - 1) u        Wy[y] likewise            (2 gh - 1) u
    row[y] = sum_x Wx[x] m: at most gw + 2 pixels, products with 0 / 1 exact                                    (gw + 1) u
    Wy[y] * row[y]: one product                                                                                  u
    the sum over at most gh + 2 rows, in any grouping                                                            (gh + 1) u
    the division by count                                                                                        u
    total 3 (gw + gh) + 2; one more u covers an implementation that rounds the product of the two axis weights per tap (mmcv's
    order), and (1 + u)^n - 1 <= (n + 1) u for n <= 4000 (asserted):        |t - T| <= (3 (gw + gh) + 6) u T     [two units to spare]
    A bin with T = 0 has bound 0: it must be exactly zero.  On the dyadic cases every term is a multiple of 2^-10 and the sums stay
    below 2^14, so every partial sum in any order is an fp32 number: the comparison is bit for bit and `exact` records that this was
    checked on the float64 terms, not assumed.
  Loss, element of a counted row, x the logit, t the target in [0, 1], w the row weight, den = fl(n * M * M) (the same fp32 number on
  both sides: no error).  a = max(x, 0) - x t >= 0: the product u |x t|, the subtraction u a.  e = expf(-|x|): 2u.  l = log1pf(e): the
  true log1p changes by at most the relative change of e, plus its own 2u: 4u l.  fl(a + l): u (a + l); times w: u.
                       |term - TERM| <= |w| (u |x t| + u a + 4u l + u (a + l)) + 2u |TERM|
    sigmoid: fl(1 + e): 3u (1 + e); the division u; for x < 0 the numerator adds 2u: relative 6u.  fl(sig - t): u |sig - t|; times w
    and / den: 2u.     |g - G| <= (|w| / den) (6u SIG + u |SIG - t|) + 3u |G|
    A sum of n non-zero terms in any order: n u sum |TERM|; the division and one u of slack:
                       |loss - LOSS| <= (sum term bounds + n u sum |TERM|) / den + 2u |LOSS| + (n + 1) TINY
    TINY = 2^-100 per term covers a flushed subnormal expf (logits of +-100).
  Paste, pixel of a live detection.  gx is the same fp32 number on both sides.  ix = fl(fl(fl(gx + 1) M) - 1) / 2: with b = (gx + 1) M,
    |b| <= 2 M + 1 on a pixel with a tap inside the mask, the three roundings give |ix - IX| <= (2u |b| + u |b - 1|) / 2 <= 3u (M + 1);
    the same in y.  Bilinear interpolation with zero padding is continuous and its slope along an axis is at most
    L = the largest difference of two neighbouring values of the zero-padded p, so the coordinates cost 6u (M + 1) L.  With the
    coordinate fixed: p = sigmoid: 6u; the two weights u each (ix - fx is exact or one rounding), their product u, times p u, three
    additions 3u: 13u of sum w p <= Pmax.  With slack:
                       |v - V| <= 6u (M + 1) L + 16u Pmax + TINY
  The two thresholded outputs: a bin or pixel whose float64 value lies within its bound of the threshold is UNDECIDED and may come out
  either way; everywhere else the byte must be equal.  Band caps, asserted from the reference alone (test_det_masks_cpu.py): at most 2 %
  of any one case's outputs and at most 0.1 % of all outputs of the random cases together; seeds are chosen to meet them.

CASES are generated from seeds; nothing is read from outside the repository.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _roi_extract_ref import _axis_sample_scalar, axis_samples

U = 2.0 ** -24
TINY = 2.0 ** -100
F32 = np.float32
_f = np.float32
QUANTUM = 2.0 ** 10


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def inside(got, want, bound):
    """Element by element |got - want| <= bound, NaN-free; a zero bound asks for equality.  -> (ok, worst fraction of the bound)."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    if got.shape != want.shape or not np.all(np.isfinite(got)):
        return False, float("inf")
    if got.size == 0:
        return True, 0.0
    diff = np.abs(got - want)
    frac = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))
    return bool(np.all(frac <= 1.0)), float(frac.max())


def binary_check(got, value, bound, thr):
    """A thresholded output against the float64 value: equal outside the undecided band.  -> (ok, number of elements in the band)."""
    got = np.asarray(got)
    band = np.abs(value - thr) <= bound
    want = (value >= thr).astype(got.dtype)
    ok = got.shape == want.shape and bool(np.all((got == want) | band)) and bool(np.all(got <= 1))
    return ok, int(band.sum())


# ================================================================================================ target
def _clip_geometry(roi, H, W, M):
    """-> None (non-finite box) or (sx, sy, bw, bh, gw, gh), np.float32 op by op: mmdet's np.clip, then the geometry with s = 1, P = M."""
    x0, y0, x1, y1 = (_f(v) for v in roi[1:5])
    if not np.all(np.isfinite([x0, y0, x1, y1])):
        return None
    x0, x1 = np.clip(x0, _f(0), _f(W)), np.clip(x1, _f(0), _f(W))
    y0, y1 = np.clip(y0, _f(0), _f(H)), np.clip(y1, _f(0), _f(H))
    sx, sy = _f(x0 - _f(0.5)), _f(y0 - _f(0.5))
    bw, bh = _f(_f(_f(x1 - _f(0.5)) - sx) / _f(M)), _f(_f(_f(y1 - _f(0.5)) - sy) / _f(M))
    return sx, sy, bw, bh, int(np.ceil(bw)), int(np.ceil(bh))


def target_loops(rois, gt_rows, masks, M):
    """The line-by-line restatement: mmcv's loop over bins and samples.  -> t [R, M, M] float64."""
    Gtot, H, W = masks.shape
    out = np.zeros((len(rois), M, M))
    for r in range(len(rois)):
        g = int(gt_rows[r])
        geo = _clip_geometry(rois[r], H, W, M)
        if not (0 <= g < Gtot) or geo is None:
            continue
        sx, sy, bw, bh, gw, gh = geo
        if gw <= 0 or gh <= 0:
            continue
        m = (masks[g] != 0).astype(np.float64)
        count = float(max(gh * gw, 1))
        for ph in range(M):
            for pw in range(M):
                acc = 0.0
                for iy in range(gh):
                    ys = _axis_sample_scalar(sy, bh, gh, ph, iy, H)
                    for ix in range(gw):
                        xs = _axis_sample_scalar(sx, bw, gw, pw, ix, W)
                        if ys is None or xs is None:
                            continue
                        (yl, yh, hy, ly), (xl, xh, hx, lx) = ys, xs
                        acc += float(hy) * float(hx) * m[yl, xl] + float(hy) * float(lx) * m[yl, xh] \
                            + float(ly) * float(hx) * m[yh, xl] + float(ly) * float(lx) * m[yh, xh]
                out[r, ph, pw] = acc / count
    return out


def _axis_matrix(start, binsz, grid, M, size):
    """A [M, size] float64: the exact sums of the fp32 tap weights of bin p that land on pixel x."""
    valid, lo, hi, w_lo, w_hi = axis_samples(start, binsz, grid, M, size)
    A = np.zeros((M, size))
    p = np.repeat(np.arange(M), grid)
    np.add.at(A, (p[valid], lo[valid]), w_lo[valid].astype(np.float64))
    np.add.at(A, (p[valid], hi[valid]), w_hi[valid].astype(np.float64))
    return A


def target_vec(rois, gt_rows, masks, M, plant=None):
    """-> dict(t, bound [R, M, M] float64, grids [R, 2], exact bool): the separable form in float64; bound = (3 (gw + gh) + 6) u t.
    plant: 'neighbour_plane' samples the plane of ground truth g + 1 (mod Gtot)."""
    Gtot, H, W = masks.shape
    R = len(rois)
    t, bound, grids = np.zeros((R, M, M)), np.zeros((R, M, M)), np.zeros((R, 2), np.int64)
    exact = True
    for r in range(R):
        g = int(gt_rows[r])
        geo = _clip_geometry(rois[r], H, W, M)
        if not (0 <= g < Gtot) or geo is None:
            continue
        sx, sy, bw, bh, gw, gh = geo
        if gw <= 0 or gh <= 0:
            continue
        if plant == "neighbour_plane":
            g = (g + 1) % Gtot
        m = (masks[g] != 0).astype(np.float64)
        Ax, Ay = _axis_matrix(sx, bw, gw, M, W), _axis_matrix(sy, bh, gh, M, H)
        # axis weights on multiples of 2^-5 (terms on 2^-10), a power-of-two count: the sums and the division are exact in fp32
        exact = exact and bool((Ax * 32 == np.round(Ax * 32)).all() and (Ay * 32 == np.round(Ay * 32)).all()) \
            and gh * gw <= 16 and (gh * gw) & (gh * gw - 1) == 0
        n = 3 * (gw + gh) + 5
        assert n <= 4000
        t[r] = Ay @ m @ Ax.T / float(max(gh * gw, 1))
        bound[r] = (n + 1) * U * t[r]
        grids[r] = gh, gw
    exact = exact and bool((t * QUANTUM == np.round(t * QUANTUM)).all())
    return dict(t=t, bound=bound, grids=grids, exact=exact)


def binary_target_ok(ref, got):
    """The binary target against target_vec's record: on an exact case (every partial sum an fp32 number, so no rounding can move a value
    across the threshold) bit for bit, a tie at 1/2 giving 1; otherwise equal outside the undecided band."""
    if ref["exact"]:
        return same_bits(np.asarray(got, np.uint8), binarize(ref["t"]))
    return binary_check(got, ref["t"], ref["bound"], 0.5)[0]


def binarize(t, tie_to_one=True):
    return (t >= 0.5).astype(np.uint8) if tie_to_one else (t > 0.5).astype(np.uint8)


def blob_masks(G, H, W, seed, noise=0.03):
    """G binary planes: a few ellipses each, with salt-and-pepper noise; values 0 / 1 / 255 (a byte != 0 counts as 1)."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((G, H, W), np.uint8)
    for g in range(G):
        m = np.zeros((H, W), bool)
        for _ in range(3):
            cy, cx, ry, rx = r.rand() * H, r.rand() * W, (0.08 + 0.3 * r.rand()) * H, (0.08 + 0.3 * r.rand()) * W
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        m ^= r.rand(H, W) < noise
        out[g] = np.where(m, np.where(r.rand(H, W) < 0.5, 1, 255), 0)
    return out


def random_boxes(R, H, W, seed, smin=2.0, smax=None):
    r = np.random.RandomState(seed)
    smax = smax or min(H, W) - 3.0
    w, h = smin + (smax - smin) * r.rand(R), smin + (smax - smin) * r.rand(R)
    x0, y0 = r.rand(R) * (W - w), r.rand(R) * (H - h)
    return np.stack([np.zeros(R), x0, y0, x0 + w, y0 + h], 1).astype(np.float32)


def target_case(name):
    """-> dict(masks [G, H, W] uint8, rois [R, 5], gt_rows [R] int32, M, ref=target_vec(...)); computed once, read-only."""
    if name in _memo:
        return _memo[name]
    if name == "small":                                        # 37 x 53, Gtot = 5, R = 9: the departures and the plane's edges
        H, W, G = 37, 53, 5
        masks = blob_masks(G, H, W, 1)
        rois = random_boxes(9, H, W, 2)
        rows = np.array([0, 1, 2, 3, 4, 2, 1, 0, 3], np.int32)
        rows[1], rows[2] = -1, G                               # not a positive slot / out of range
        rois[3, 1:] = [-7.5, -3.25, 20.5, 18.0]                # partly outside the plane before the clip
        rois[4, 1:] = [11.0, 5.0, 11.0, 30.0]                  # zero width
        rois[5, 1:] = [30.25, 20.5, 53.0, 37.0]                # ends on the last row and column
        rois[6, 1:] = [np.nan, 2.0, 20.0, 30.0]                # a NaN coordinate
        rois[7, 1:] = [40.0, 30.0, 70.0, 50.0]                 # hangs over the far corner
        M = 28
    elif name == "large":                                      # 96 x 128 with boxes up to the full plane: grids of 4 and 5
        H, W, G = 96, 128, 3
        masks = blob_masks(G, H, W, 3)
        rois = random_boxes(6, H, W, 4, smin=20.0)
        rows = np.array([0, 1, 2, 0, 1, 2], np.int32)
        rois[0, 1:] = [0.0, 0.0, 128.0, 96.0]
        rois[1, 1:] = [3.3, 1.7, 126.1, 95.2]
        M = 28
    elif name.startswith("rand"):                              # the CPU band statistics: blob and noise masks at 96 x 128, boxes 2 - 125 px
        seed = int(name[4:])
        H, W, G = 96, 128, 2
        masks = blob_masks(G, H, W, 100 + seed, noise=0.0 if seed % 2 else 0.05)
        rois = random_boxes(4, H, W, 200 + seed, smin=2.0, smax=93.0)
        rois[:, 3] = np.minimum(rois[:, 1] + (rois[:, 3] - rois[:, 1]) * 125.0 / 93.0, 128.0)
        rows = np.array([0, 1, 0, 1], np.int32)
        M = 28
    else:
        raise KeyError(name)
    c = dict(name=name, masks=masks, rois=rois, gt_rows=rows, M=M, ref=target_vec(rois, rows, masks, M))
    _memo[name] = c
    return c


def dyadic_case(M):
    """Boxes whose samples fall on quarter-pixel offsets with grid 2: every weight is a multiple of 1/4, every term of 2^-10."""
    H = W = 4 * M + 8
    masks = blob_masks(2, H, W, 50 + M, noise=0.2)
    side = 2.0 * M
    rois = np.array([[0, 0.5, 0.5, 0.5 + side, 0.5 + side], [0, 0.25, 1.75, 0.25 + side, 1.75 + side], [0, 3.0, 2.5, 3.0 + side, 2.5 + side],
                     [0, 2 * M + 0.75, 2 * M + 0.5, 2 * M + 0.75 + side, 2 * M + 0.5 + side]], np.float32)
    rows = np.array([0, 1, 1, 0], np.int32)
    ref = target_vec(rois, rows, masks, M)
    return dict(name=f"dyadic{M}", masks=masks, rois=rois, gt_rows=rows, M=M, ref=ref)


TARGET_RANDOM = ["small", "large"]
_memo = {}


# ================================================================================================ loss
def den_f32(n, M):
    return float(F32(n) * F32(M * M))


def loss_case(name):
    """-> dict(pred [R, C, M, M], labels [R] int32 or None, targets [R, M, M] uint8 / fp32, w [R], plain bool)."""
    spec = LOSS_CASES[name]
    R, C, M, kind = spec["R"], spec["C"], spec["M"], spec["kind"]
    rng = np.random.default_rng(spec["seed"])
    pred = rng.normal(0, 3, (R, C, M, M)).astype(F32)
    targets = (rng.random((R, M, M)) < 0.4).astype(np.uint8)
    w = (rng.random(R) < 0.6).astype(F32)
    if R:
        w[0] = 1
    labels = None if C == 1 and kind != "labels" else rng.integers(0, C, R).astype(np.int32)
    plain = True
    if kind == "allzero":
        w[:] = 0
    if kind == "labels":
        labels[1] = C                                          # out of range: not counted
        labels[2] = -1
        w[1] = w[2] = 1
        plain = False
    if kind == "soft":
        targets = rng.random((R, M, M)).astype(F32)
    if kind == "big":
        pred = np.where(rng.random(pred.shape) < 0.5, F32(100), F32(-100)).astype(F32)
    if kind == "nan_row":
        w[1] = 0
        pred[1] = np.nan
        pred[2, 0, 0, 0] = np.inf
        w[2] = 0
        plain = False
    if kind == "weights":
        w = np.where(w > 0, rng.choice([0.5, 2.0, 1.0], R), 0).astype(F32)
        w[-1] = -1.0                                           # negative: not counted
        plain = False
    return dict(name=name, R=R, C=C, M=M, pred=pred, labels=labels, targets=targets, w=w, plain=plain, kind=kind)


LOSS_CASES = {
    "R0": dict(R=0, C=1, M=28, kind="random", seed=1),
    "allzero": dict(R=5, C=1, M=28, kind="allzero", seed=2),
    "R7_C1": dict(R=7, C=1, M=28, kind="random", seed=3),
    "C3_labels": dict(R=9, C=3, M=28, kind="labels", seed=4),
    "C3_odd": dict(R=6, C=3, M=7, kind="random", seed=5),          # M * M = 49: planes that start off a 16-byte boundary, a ragged last group
    "soft": dict(R=7, C=1, M=28, kind="soft", seed=6),
    "big": dict(R=5, C=1, M=14, kind="big", seed=7),
    "nan_row": dict(R=6, C=2, M=14, kind="nan_row", seed=8),
    "weights": dict(R=8, C=1, M=14, kind="weights", seed=9),
    "M64": dict(R=3, C=2, M=64, kind="random", seed=10),           # 4096 cells: four groups per thread
}


def loss_ref(c, plant=None):
    """(b) closed form -> dict(out [2] = (loss, n), dpred, out_bound, dpred_bound), float64.
    plant: 'row_count' divides by the number of counted rows instead of n * M * M."""
    R, C, M = c["R"], c["C"], c["M"]
    lab = np.zeros(R, np.int64) if c["labels"] is None else c["labels"].astype(np.int64)
    w = c["w"].astype(np.float64)
    counted = (c["w"] > 0) & (lab >= 0) & (lab < C)
    n = max(int(counted.sum()), 1)
    den = den_f32(n, M) if plant != "row_count" else float(n)
    dpred, db = np.zeros((R, C, M, M)), np.zeros((R, C, M, M))
    terms, tb = [], []
    for r in np.nonzero(counted)[0]:
        x = c["pred"][r, lab[r]].astype(np.float64)
        t = c["targets"][r].astype(np.float64) if c["targets"].dtype == F32 else (c["targets"][r] != 0).astype(np.float64)
        with np.errstate(all="ignore"):
            e = np.exp(-np.abs(x))
            a, l = np.maximum(x, 0) - x * t, np.log1p(e)
            term = w[r] * (a + l)
            sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
            g = w[r] * (sig - t) / den
        terms.append(term)
        tb.append(abs(w[r]) * (U * np.abs(x * t) + U * a + 4 * U * l + U * (a + l)) + 2 * U * np.abs(term))
        dpred[r, lab[r]] = g
        db[r, lab[r]] = abs(w[r]) / den * (6 * U * sig + U * np.abs(sig - t)) + 3 * U * np.abs(g) + TINY
    terms = np.array(terms).reshape(-1)
    tb = np.array(tb).reshape(-1)
    loss = terms.sum() / den
    nt = int(np.count_nonzero(terms))
    lb = (tb.sum() + nt * U * np.abs(terms).sum()) / den + 2 * U * abs(loss) + (nt + 1) * TINY
    return dict(out=np.array([loss, float(n)]), out_bound=np.array([lb, 0.0]), dpred=dpred, dpred_bound=db)


def loss_mmdet(c):
    """(a) mmdet's mask_cross_entropy in torch float64 on the counted rows (mmdet passes the positive rows only), gradient by autograd,
    scattered back to [R, C, M, M].  For cases where no departure applies and the weights are 0 / 1."""
    R, C, M = c["R"], c["C"], c["M"]
    pred = torch.tensor(c["pred"], dtype=torch.float64, requires_grad=True)
    pos = torch.tensor(c["w"] > 0)
    mask_pred = pred[pos]
    label = torch.zeros(int(pos.sum()), dtype=torch.long) if c["labels"] is None else torch.tensor(c["labels"].astype(np.int64))[pos]
    target = torch.tensor(c["targets"].astype(np.float64))[pos] if c["targets"].dtype == F32 else torch.tensor((c["targets"] != 0).astype(np.float64))[pos]
    if mask_pred.size(0) == 0:
        loss = mask_pred.sum()
    else:
        num_rois = mask_pred.size()[0]
        inds = torch.arange(0, num_rois, dtype=torch.long)
        pred_slice = mask_pred[inds, label].squeeze(1)
        loss = F.binary_cross_entropy_with_logits(pred_slice, target, weight=None, reduction="mean")
    loss.backward()
    return float(loss.detach()), pred.grad.numpy()


# ================================================================================================ paste
def paste_grid(boxes, img_h, img_w):
    """The header's normalised coordinates in np.float32, op by op -> gx [N, img_w], gy [N, img_h] (NaN / inf where the box is bad)."""
    b = np.asarray(boxes, F32)
    X, Y = (np.arange(img_w, dtype=F32) + _f(0.5))[None, :], (np.arange(img_h, dtype=F32) + _f(0.5))[None, :]
    with np.errstate(all="ignore"):
        gx = (X - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * _f(2) - _f(1)
        gy = (Y - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * _f(2) - _f(1)
    assert gx.dtype == F32 and gy.dtype == F32
    return gx, gy


def paste_ok(boxes, labels, C):
    b = np.asarray(boxes, F32)
    with np.errstate(all="ignore"):
        dx, dy = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        ok = np.isfinite(b).all(1) & np.isfinite(dx) & np.isfinite(dy) & (dx > 0) & (dy > 0)
    lab = np.zeros(len(b), np.int64) if labels is None else np.asarray(labels, np.int64)
    return ok & (lab >= 0) & (lab < C), lab


def paste_ref(logits, labels, boxes, img_h, img_w, plant=None):
    """-> dict(v, bound [N, img_h, img_w] float64): _do_paste_mask on F.grid_sample in float64.
    plant: 'no_half' leaves the + 0.5 pixel-centre offset out of the coordinates."""
    N, C, M, _ = logits.shape
    ok, lab = paste_ok(boxes, labels, C)
    if plant == "no_half":
        b = np.asarray(boxes, F32).copy()
        b[:, [0, 2]] += _f(0.5)
        b[:, [1, 3]] += _f(0.5)                                # (X - (x0 + .5)) / (x1 - x0): the offset is gone
        gx, gy = paste_grid(b, img_h, img_w)
    else:
        gx, gy = paste_grid(boxes, img_h, img_w)
    v, bound = np.zeros((N, img_h, img_w)), np.zeros((N, img_h, img_w))
    for n in range(N):
        if not ok[n]:
            continue
        with np.errstate(all="ignore"):
            p = torch.sigmoid(torch.tensor(logits[n, lab[n]].astype(np.float64)))
        grid = torch.stack([torch.tensor(gx[n].astype(np.float64))[None, :].expand(img_h, img_w),
                            torch.tensor(gy[n].astype(np.float64))[:, None].expand(img_h, img_w)], dim=2)[None]
        v[n] = F.grid_sample(p[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0].numpy()
        pp = np.pad(p.numpy(), 1)
        L = max(np.abs(np.diff(pp, axis=0)).max(), np.abs(np.diff(pp, axis=1)).max())
        bound[n] = 6 * U * (M + 1) * L + 16 * U * pp.max() + TINY
    return dict(v=v, bound=bound)


def paste_case(name):
    """-> dict(logits [N, C, M, M], labels or None, boxes [N, 4], img_h, img_w, ref); computed once, read-only."""
    if name in _memo:
        return _memo[name]
    M = {"m28": 28, "m4": 4}[name]
    rng = np.random.default_rng(70 + M)
    img_h, img_w, C = 40, 56, 2
    boxes = np.array([[10.3, 5.2, 41.7, 33.9],                 # inside the image
                      [-9.5, -6.25, 70.1, 47.3],               # overhangs every edge
                      [60.0, 45.0, 90.0, 80.0],                # wholly outside
                      [20.0, 10.0, 20.0, 30.0],                # zero extent
                      [np.nan, 1.0, 30.0, 20.0]], F32)         # a NaN coordinate
    N = len(boxes)
    logits = rng.normal(0, 2.5, (N, C, M, M)).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    bad = 0 if M == 28 else 1                                  # the bad label sits on a box that would be live: the inside one / the overhanging one
    labels[bad] = C
    c_live = 1 - bad
    c = dict(name=name, logits=logits, labels=labels, boxes=boxes, img_h=img_h, img_w=img_w, M=M, C=C, thr=0.5, live=c_live,
             zero=[bad, 2, 3, 4], ref=paste_ref(logits, labels, boxes, img_h, img_w))
    _memo[name] = c
    return c


PASTE_RANDOM = ["m28", "m4"]
