"""TEST INFRASTRUCTURE -- numpy restatement of the detector's RoI extractor (include/clipself_roi.h), forward and backward.

What is restated, by the published function names (mmcv 1.x / mmdet 2.x; neither package nor its source is available to this project,
so this boundary is parity-unpinned in the sense of DESIGN.md §3.14: the restatement follows the published sources as read, it was not
run against them):

  mmdet.models.roi_heads.roi_extractors.SingleRoIExtractor.map_roi_levels:  scale = sqrt((x1 - x0) * (y1 - y0)),
      floor(log2(scale / finest_scale + 1e-6)) clamped to [0, num_levels - 1]                                           -> roi_levels
  mmcv.ops.roi_align, `roi_align_forward_cuda_kernel` (aligned=True, pool_mode='avg'): start = x0 * spatial_scale - 0.5, bin = extent / P,
      grid = sampling_ratio or ceil(extent / P), sample = start + ph * bin + (iy + .5) * bin / grid, count = max(grid_h * grid_w, 1)
      and `bilinear_interpolate` (outside [-1, size]: nothing; clamp at 0 and at the last cell; weights hy * hx, hy * lx, ly * hx, ly * lx)
                                                                                                                        -> box_geometry, axis_samples, forward_*
  mmcv.ops.roi_align, `roi_align_backward_cuda_kernel`: every tap adds weight * grad / count to its cell (there with atomicAdd, here as
      the ordered gather of the header)                                                                                 -> backward_*

Coordinates, weights and the level are computed in np.float32, one operation at a time, exactly as the header prescribes; numpy
evaluates every float32 product, quotient and sum as an operation of its own.  The weights are then fixed numbers, and the sums over
taps are accumulated in float64.  Each function comes as scalar loops (`*_loops`, the line-by-line restatement, small cases) and
vectorised per box (`*_vec`); test_roi_extract_cpu.py cross-checks them.

The bound an fp32 implementation is held to.  With the weights fixed by the contract the only freedom is the order of the sum.  Let
u = 2^-24, T the number of taps of the element, and S = sum |w_t f_t| / count taken from the float64 values.
  forward:  out = fl(fl-sum_t(fl(w_t f_t)) / count).  A term passes one rounding as a product (none when the implementation fuses it
      into an fma) and takes part in at most T - 1 additions, whatever the order or the tree; the division adds one rounding.  Every term
      therefore carries a factor (1 + d)^(T + 1), |d| <= u:  |out - exact| <= ((1 + u)^(T + 1) - 1) S.
  backward: cell += sum_t fl(w_t fl(g_t / count)): the division and the product round once each, at most T - 1 additions, and one more
      for the addition onto the map:  |cell - exact| <= ((1 + u)^(T + 2) - 1) S   (for a map that held zeros, as in the tests).
  (1 + u)^n - 1 <= n u / (1 - n u) <= (n + 1) u  while n (n + 1) u <= 1, i.e. n <= 4000.  With n = T + 2 this gives
      bound = (T + 4) u S   with one unit to spare for the forward, none tuned, asserted for T + 3 <= 4000 only.
The float64 accumulation of the reference itself errs by T 2^-53 S, nine orders of magnitude below.  An element with S = 0 has bound 0:
it must be exactly zero.  On the lattice cases (lattice_case) every term is a multiple of 2^-10 and S < 2^14, so every partial sum is an
fp32 number: the bound is not used there and the comparison is bit for bit; `exact` in the returned records states that this was
checked on the float64 terms, not assumed.
"""
import numpy as np

U = 2.0 ** -24
C_BOUND = 4
_f = np.float32
QUANTUM = 2.0 ** 10


# ================================================================================================ level and geometry, np.float32
def roi_levels(rois, L, finest_scale):
    """[K] int: the header's level rule, fp32 op by op; NaN -> 0."""
    r = np.asarray(rois, np.float32)
    with np.errstate(all="ignore"):
        area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
        t = np.floor(np.log2(np.sqrt(area) / _f(finest_scale) + _f(1e-6)))
    t = np.where(t >= 1, np.minimum(t, _f(L - 1)), _f(0))
    return t.astype(np.int64)


def level_margin(rois, finest_scale):
    """Relative distance of scale / finest_scale from the nearest power of two (float64): the random cases keep it above 1e-4."""
    r = np.asarray(rois, np.float64)
    v = np.sqrt(np.abs((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))) / finest_scale
    e = np.log2(np.maximum(v, 1e-300))
    return np.abs(2.0 ** (e - np.round(e)) - 1.0)


def spatial_scale(stride):
    return _f(1.0 / float(stride))


def box_geometry(roi, s, h, w, B, P, sampling_ratio):
    """-> None (the box pools to zeros) or dict(b, sy, sx, bh, bw, gh, gw, count); s = spatial_scale of the box's level (np.float32)."""
    bf, x0, y0, x1, y1 = (_f(v) for v in roi)
    with np.errstate(all="ignore"):
        sx, sy = _f(_f(x0 * s) - _f(0.5)), _f(_f(y0 * s) - _f(0.5))
        rw, rh = _f(_f(_f(x1 * s) - _f(0.5)) - sx), _f(_f(_f(y1 * s) - _f(0.5)) - sy)
        bw, bh = _f(rw / _f(P)), _f(rh / _f(P))
        ok = bool(bf >= 0) and bool(bf < B) and bool(np.abs(rw) <= _f(2 * w)) and bool(np.abs(rh) <= _f(2 * h))
    if not ok:
        return None
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bw))
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bh))
    if gw <= 0 or gh <= 0:
        return None
    return dict(b=int(bf), sy=sy, sx=sx, bh=bh, bw=bw, gh=gh, gw=gw, count=float(max(gh * gw, 1)))


def axis_samples(start, binsz, grid, P, size):
    """The P * grid samples of one axis in ascending (p, i) -> valid [n] bool, lo, hi [n] int, w_lo, w_hi [n] np.float32."""
    p = np.repeat(np.arange(P, dtype=np.float32), grid)
    i = np.tile(np.arange(grid, dtype=np.float32), P)
    with np.errstate(all="ignore"):
        c = (start + p * binsz) + ((i + _f(0.5)) * binsz) / _f(grid)
    assert c.dtype == np.float32
    valid = (c >= -1) & (c <= size)
    c = np.where(valid & (c > 0), c, _f(0))
    lo = c.astype(np.int64)
    edge = lo >= size - 1
    lo = np.where(edge, size - 1, lo)
    hi = np.where(edge, lo, lo + 1)
    c = np.where(edge, lo.astype(np.float32), c)
    w_hi = (c - lo.astype(np.float32)).astype(np.float32)
    w_lo = (_f(1) - w_hi).astype(np.float32)
    return valid, lo, hi, w_lo, w_hi


def _axis_sample_scalar(start, binsz, grid, p, i, size):
    """One sample, as mmcv's kernel walks it: -> None or (lo, hi, w_lo, w_hi)."""
    c = _f(_f(start + _f(_f(p) * binsz)) + _f(_f(_f(_f(i) + _f(0.5)) * binsz) / _f(grid)))
    if c < -1.0 or c > size:
        return None
    if c <= 0:
        c = _f(0)
    lo = int(c)
    if lo >= size - 1:
        hi = lo = size - 1
        c = _f(lo)
    else:
        hi = lo + 1
    l = _f(c - _f(lo))
    return lo, hi, _f(_f(1) - l), l


def _prep(maps_or_grids, rois, strides, P, sampling_ratio, finest_scale, B):
    grids = [(m.shape[1], m.shape[2]) if hasattr(m, "shape") else tuple(m) for m in maps_or_grids]
    lv = roi_levels(rois, len(grids), finest_scale)
    geos = []
    for k in range(len(rois)):
        h, w = grids[lv[k]]
        geos.append(box_geometry(rois[k], spatial_scale(strides[lv[k]]), h, w, B, P, sampling_ratio))
    return grids, lv, geos


# ================================================================================================ scalar loops
def forward_loops(maps, rois, strides, P, sampling_ratio=0, finest_scale=56):
    """maps: L arrays [B, h, w, C] -> out [K, P, P, C] float64."""
    B, C = maps[0].shape[0], maps[0].shape[3]
    grids, lv, geos = _prep(maps, rois, strides, P, sampling_ratio, finest_scale, B)
    out = np.zeros((len(rois), P, P, C))
    for k, g in enumerate(geos):
        if g is None:
            continue
        m = maps[lv[k]][g["b"]].astype(np.float64)
        h, w = grids[lv[k]]
        for ph in range(P):
            for pw in range(P):
                acc = np.zeros(C)
                for iy in range(g["gh"]):
                    ys = _axis_sample_scalar(g["sy"], g["bh"], g["gh"], ph, iy, h)
                    for ix in range(g["gw"]):
                        xs = _axis_sample_scalar(g["sx"], g["bw"], g["gw"], pw, ix, w)
                        if ys is None or xs is None:
                            continue
                        (yl, yh, hy, ly), (xl, xh, hx, lx) = ys, xs
                        acc += float(_f(hy * hx)) * m[yl, xl] + float(_f(hy * lx)) * m[yl, xh] + float(_f(ly * hx)) * m[yh, xl] \
                            + float(_f(ly * lx)) * m[yh, xh]
                out[k, ph, pw] = acc / g["count"]
    return out


def backward_loops(dout, rois, grids, strides, B, P, sampling_ratio=0, finest_scale=56):
    """dout [K, P, P, C] -> L arrays [B, h, w, C] float64 (added onto zeros)."""
    C = dout.shape[3]
    grids, lv, geos = _prep(grids, rois, strides, P, sampling_ratio, finest_scale, B)
    dmaps = [np.zeros((B, h, w, C)) for h, w in grids]
    for k, g in enumerate(geos):
        if g is None:
            continue
        d = dmaps[lv[k]][g["b"]]
        h, w = grids[lv[k]]
        for ph in range(P):
            for pw in range(P):
                gv = dout[k, ph, pw].astype(np.float64) / g["count"]
                for iy in range(g["gh"]):
                    ys = _axis_sample_scalar(g["sy"], g["bh"], g["gh"], ph, iy, h)
                    for ix in range(g["gw"]):
                        xs = _axis_sample_scalar(g["sx"], g["bw"], g["gw"], pw, ix, w)
                        if ys is None or xs is None:
                            continue
                        (yl, yh, hy, ly), (xl, xh, hx, lx) = ys, xs
                        d[yl, xl] += float(_f(hy * hx)) * gv
                        d[yl, xh] += float(_f(hy * lx)) * gv
                        d[yh, xl] += float(_f(ly * hx)) * gv
                        d[yh, xh] += float(_f(ly * lx)) * gv
    return dmaps


# ================================================================================================ vectorised per box, with the bound
def _box_taps(g, h, w, P):
    """-> (mask [ny, nx], four (yi [ny], xi [nx], weight [ny, nx] float64)) for one box."""
    vy, ylo, yhi, hy, ly = axis_samples(g["sy"], g["bh"], g["gh"], P, h)
    vx, xlo, xhi, hx, lx = axis_samples(g["sx"], g["bw"], g["gw"], P, w)
    mask = vy[:, None] & vx[None, :]
    prod = lambda a, b: np.where(mask, (a[:, None] * b[None, :]).astype(np.float32), _f(0)).astype(np.float64)     # fp32 product, rounded once
    return mask, [(ylo, xlo, prod(hy, hx)), (ylo, xhi, prod(hy, lx)), (yhi, xlo, prod(ly, hx)), (yhi, xhi, prod(ly, lx))]


def forward_vec(maps, rois, strides, P, sampling_ratio=0, finest_scale=56):
    """-> dict(out, bound [K, P, P, C] float64, levels [K], exact bool): bound = (T + C_BOUND) u sum |w f| / count."""
    B, C = maps[0].shape[0], maps[0].shape[3]
    grids, lv, geos = _prep(maps, rois, strides, P, sampling_ratio, finest_scale, B)
    K = len(rois)
    out, bound = np.zeros((K, P, P, C)), np.zeros((K, P, P, C))
    exact = True
    for k, g in enumerate(geos):
        if g is None:
            continue
        h, w = grids[lv[k]]
        m = maps[lv[k]][g["b"]].astype(np.float64)
        mask, taps = _box_taps(g, h, w, P)
        tot, mag = 0.0, 0.0
        for yi, xi, wt in taps:
            term = wt[..., None] * m[yi][:, xi]
            exact = exact and bool((term * QUANTUM == np.round(term * QUANTUM)).all())
            tot, mag = tot + term, mag + np.abs(term)
        bins = lambda a: a.reshape(P, g["gh"], P, g["gw"], -1).sum(axis=(1, 3))
        T = 4 * bins(mask.astype(np.float64)[..., None])
        assert T.max() + C_BOUND - 1 <= 4000
        mag = bins(mag)
        exact = exact and bool(mag.max() < 2.0 ** 14)
        out[k] = bins(tot) / g["count"]
        bound[k] = (T + C_BOUND) * U * mag / g["count"]
    return dict(out=out, bound=bound, levels=lv, exact=exact)


def backward_vec(dout, rois, grids, strides, B, P, sampling_ratio=0, finest_scale=56):
    """-> dict(dmaps, bounds: L arrays [B, h, w, C] float64, exact bool)."""
    C = dout.shape[3]
    grids, lv, geos = _prep(grids, rois, strides, P, sampling_ratio, finest_scale, B)
    dm = [np.zeros((B, h, w, C)) for h, w in grids]
    mag = [np.zeros((B, h, w, C)) for h, w in grids]
    cnt = [np.zeros((B, h, w)) for h, w in grids]
    exact = True
    for k, g in enumerate(geos):
        if g is None:
            continue
        l = lv[k]
        h, w = grids[l]
        mask, taps = _box_taps(g, h, w, P)
        ny, nx = mask.shape
        gv = dout[k].astype(np.float64) / g["count"]                                   # [P, P, C]
        gs = gv[np.arange(ny)[:, None] // g["gh"], np.arange(nx)[None, :] // g["gw"]]  # [ny, nx, C]: the bin of every sample
        r0, r1, c0, c1 = taps[0][0].min(), taps[3][0].max() + 1, taps[0][1].min(), taps[3][1].max() + 1      # the cells the box can touch
        for yi, xi, wt in taps:
            term = wt[..., None] * gs                                                  # zero where the sample is outside
            exact = exact and bool((term * QUANTUM == np.round(term * QUANTUM)).all())
            # scatter by one-hot matrices: the products with 0 and 1 are exact, the sums are float64.  Value, magnitude and tap count
            # ride along as 2 C + 1 columns
            yoh = (yi[None, :] == np.arange(r0, r1)[:, None]).astype(np.float64)       # [rows, ny]
            xoh = (xi[None, :] == np.arange(c0, c1)[:, None]).astype(np.float64)       # [cols, nx]
            a = np.concatenate([term, np.abs(term), mask[..., None].astype(np.float64)], axis=2)
            s = np.matmul(xoh[None], (yoh @ a.reshape(ny, -1)).reshape(r1 - r0, nx, 2 * C + 1))      # [rows, cols, 2 C + 1]
            dm[l][g["b"], r0:r1, c0:c1] += s[..., :C]
            mag[l][g["b"], r0:r1, c0:c1] += s[..., C:2 * C]
            cnt[l][g["b"], r0:r1, c0:c1] += s[..., 2 * C]
    bounds = []
    for l in range(len(grids)):
        assert cnt[l].max(initial=0) + C_BOUND - 1 <= 4000
        exact = exact and bool(mag[l].max(initial=0) < 2.0 ** 14)
        bounds.append((cnt[l][..., None] + C_BOUND) * U * mag[l])
    return dict(dmaps=dm, bounds=bounds, exact=exact)


# ================================================================================================ cases
def image_grids(img_h, img_w, strides):
    return [(int(round(img_h / s)), int(round(img_w / s))) for s in strides]


def lattice_rois(K, B, img_h, img_w, strides, finest_scale, L, seed, empty_image=None):
    """Sides 7 * 2^m px, m = 0..5, the two sides drawn independently; origins on multiples of a quarter of the stride of the box's own
    level (all of them multiples of a quarter of the finest stride), up to half a box outside the image; rows shuffled; image
    `empty_image` gets no box.  Perfect-square areas sit exactly on the level boundaries, where the + 1e-6 decides."""
    r = np.random.RandomState(seed)
    side_w, side_h = 7.0 * 2.0 ** r.randint(0, 6, K), 7.0 * 2.0 ** r.randint(0, 6, K)
    imgs = [b for b in range(B) if b != empty_image]
    rois = np.zeros((K, 5), np.float32)
    rois[:, 0] = np.array(imgs)[r.randint(0, len(imgs), K)]
    rois[:, 3], rois[:, 4] = side_w, side_h
    lv = roi_levels(rois, L, finest_scale)
    q = np.array([strides[l] for l in lv]) / 4.0
    x0 = np.round((r.rand(K) * (img_w + side_w / 2) - side_w / 2) / q) * q
    y0 = np.round((r.rand(K) * (img_h + side_h / 2) - side_h / 2) / q) * q
    rois[:, 1], rois[:, 2], rois[:, 3], rois[:, 4] = x0, y0, x0 + side_w, y0 + side_h
    assert (roi_levels(rois, L, finest_scale) == lv).all()
    return rois[r.permutation(K)]


def random_rois(K, B, img_h, img_w, seed, smin=4.0, smax=None, empty_image=None):
    r = np.random.RandomState(seed)
    smax = smax or 1.2 * max(img_h, img_w)
    w, h = smin * (smax / smin) ** r.rand(K), smin * (smax / smin) ** r.rand(K)
    imgs = [b for b in range(B) if b != empty_image]
    x0, y0 = r.rand(K) * (img_w + w / 2) - w / 2, r.rand(K) * (img_h + h / 2) - h / 2
    b = np.array(imgs)[r.randint(0, len(imgs), K)]
    return np.stack([b, x0, y0, x0 + w, y0 + h], 1).astype(np.float32)


#              name: lattice, (img_h, img_w), strides, B, C, P, K, sampling_ratio, finest_scale, seed
CASES = {
    "lattice_big":    (True, (128, 128), [4, 8, 16, 32], 3, 260, 7, 300, 0, 14, 1),       # the extents test runs on this one
    "lattice_wide":   (True, (96, 160), [4, 8, 16, 32], 1, 4, 14, 5, 0, 14, 2),
    "lattice_fs56":   (True, (96, 160), [4, 8, 16, 32], 3, 64, 7, 300, 0, 56, 3),
    "lattice_one":    (True, (128, 128), [4], 3, 64, 7, 5, 0, 14, 4),                      # L = 1: bins of up to 8 cells, 8 x 8 samples
    "lattice_single": (True, (128, 128), [4, 8, 16, 32], 1, 64, 14, 1, 0, 14, 5),
    "random_big":     (False, (128, 128), [4, 8, 16, 32], 3, 64, 7, 300, 0, 14, 11),
    "random_l14":     (False, (112, 112), [3.5, 7, 14, 28], 3, 260, 7, 5, 2, 14, 12),
    "random_wide":    (False, (96, 160), [4, 8, 16, 32], 1, 4, 14, 300, 2, 14, 13),
    "random_p1":      (False, (128, 128), [4], 3, 64, 1, 5, 0, 14, 14),
    "random_l14_p1":  (False, (112, 112), [3.5, 7, 14, 28], 1, 4, 1, 300, 0, 56, 15),
}
LATTICE = [n for n, c in CASES.items() if c[0]]
RANDOM = [n for n, c in CASES.items() if not c[0]]
_memo = {}


def build_case(name):
    """Inputs and the float64 reference of one case, computed once per process and shared: treat every array as read-only."""
    if name in _memo:
        return _memo[name]
    lattice, (ih, iw), strides, B, C, P, K, sr, fs, seed = CASES[name]
    grids = image_grids(ih, iw, strides)
    r = np.random.RandomState(seed + 100)
    empty = 1 if B > 1 else None
    if lattice:
        rois = lattice_rois(K, B, ih, iw, strides, fs, len(strides), seed, empty)
        maps = [r.randint(-8, 9, (B, h, w, C)).astype(np.float32) for h, w in grids]
        dout = r.randint(-8, 9, (K, P, P, C)).astype(np.float32)
    else:
        rois = random_rois(K, B, ih, iw, seed, empty_image=empty)
        maps = [r.randn(B, h, w, C).astype(np.float32) for h, w in grids]
        dout = r.randn(K, P, P, C).astype(np.float32)
    c = dict(name=name, lattice=lattice, strides=strides, grids=grids, B=B, C=C, P=P, K=K, sampling_ratio=sr, finest_scale=fs, rois=rois,
             maps=maps, dout=dout, empty_image=empty)
    c["fwd"] = forward_vec(maps, rois, strides, P, sr, fs)
    c["bwd"] = backward_vec(dout, rois, grids, strides, B, P, sr, fs)
    _memo[name] = c
    return c


def check(c, out, dmaps, who):
    """out [K, P, P, C], dmaps: L arrays [B, h, w, C] (numpy) against the case's reference: bit for bit on a lattice case, inside the
    derived bound otherwise.  -> (worst forward, worst backward) fraction of the bound (0 on a lattice case)."""
    fwd, bwd = c["fwd"], c["bwd"]
    worst = [0.0, 0.0]
    pairs = [("out", out, fwd["out"], fwd["bound"], 0)] + [(f"dmaps[{l}]", d, bwd["dmaps"][l], bwd["bounds"][l], 1) for l, d in enumerate(dmaps)]
    for what, got, want, bound, slot in pairs:
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape, (who, what, got.shape, want.shape)
        assert np.isfinite(got).all(), (who, what)
        if c["lattice"]:
            bad = got != want
            assert not bad.any(), f"{who} {c['name']} {what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, first at {np.argwhere(bad)[0].tolist()}"
        else:
            err = np.abs(got - want)
            frac = float((err / np.maximum(bound, 1e-300)).max(initial=0)) if bool((bound > 0).any()) else 0.0
            zero_ok = bool((err[bound == 0] == 0).all())
            worst[slot] = max(worst[slot], frac if zero_ok else float("inf"))
            print(f"{who} {c['name']} {what}: worst err / bound {frac:.3f}")
            assert zero_ok and (err <= bound).all(), f"{who} {c['name']} {what}: worst err / bound {frac:.3f}"
    return tuple(worst)
