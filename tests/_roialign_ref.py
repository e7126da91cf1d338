"""TEST INFRASTRUCTURE -- numpy restatement of the distillation head's RoIAlign (cs_roialign_fwd's plain pooling form and cs_roialign_bwd,
clipself_amd/csrc/roialign_loss.hip), forward and backward, with a per-element error bound and the case list of tests/test_gpu_roialign.py.

What is restated.  A box is (image, x0, y0, x1, y1) with corners normalised to [0, 1].  Its map coordinate is v * s - 0.5 with s the grid
side of that axis, and the kernels' source writes it as __fsub_rn(__fmul_rn(v, s), 0.5f), which the compiler may or may not contract into
one fma.  Both outcomes are restated (`map_coord`):
    rounded   fl32(fl32(v * s) - 0.5)       the product is rounded first: what oracle/roi_align_ref.py (`_box_f32` on the boxes
                                            RefOps._rois_pixels scaled in fp32) computes
    fused     fl32(v * s - 0.5)             one rounding: v * s is exact in float64 (24 x 8 bits) and so is the subtraction
On a power-of-two grid the product is exact and the two are the same float; `geometry_both` asserts that.  Everything after the
coordinate follows `axis_weights` of the kernel file, which oracle/roi_align_ref.py (`_sample_points`, `_axis_weights`) restates too,
in np.float32 one operation at a time: extent = c1 - c0, grid = ceil(extent), count = max(gh * gw, 1), sample i of an axis at
c = start + ((i + 0.5) * extent) / grid; a sample outside [-1, size] is dropped (but counted); c <= 0 -> 0; lo >= size - 1 -> lo = hi =
size - 1 and c = lo; l = c - lo; w[lo] += 1 - l, then w[hi] += l, in sample order.  The per-axis weights Wy [grid_h], Wx [grid_w] are
then fixed fp32 numbers, and
    forward    pooled[k, :]      = sum_{r, c} Wy_k[r] Wx_k[c] F[b_k, r, c, :] / count_k
    backward   dfeat[b, r, c, :] += sum_{k of image b} Wy_k[r] Wx_k[c] dP[k, :] / count_k
are summed in float64 with the exact products Wy * Wx (48 bits).  A box with gh <= 0 or gw <= 0 pools to zeros and sends nothing.

The bound an element is held to.  u = 2^-24; n = the number of non-zero terms w f of the element (cells of the box for the forward,
boxes on the cell for the backward; a zero weight is skipped by the kernels, and a zero f gives an exact zero product whose addition
changes nothing: neither rounds); S = sum |w f| / count over those terms from the float64 values.  Counting the kernels' own roundings, each a factor (1 + d), |d| <= u, on the term:
  forward (roialign_fwd_kernel, pool_cells):
      w = wy * Wx[c]                           1    the product of the two axis weights is rounded to fp32
      acc += w * v                             1    the product, when it is not fused into the addition
                                               n    additions at the most: a term enters acc once and is carried through the later ones
      inv_count = 1.f / (float)count           1    the reciprocal (exact only for a power of two)
      acc * inv_count                          1    its multiplication
    n + 4 factors:  |out - exact| <= ((1 + u)^(n + 4) - 1) S <= (n + 5) u S,
    by (1 + u)^m - 1 <= m u / (1 - m u) <= (m + 1) u while m (m + 1) u <= 1, i.e. m <= 4000 (asserted).          C_FWD = 5
  backward (roialign_bwd_gather_kernel):
      inv_count                                1
      gv = dP * inv_count                      1
      w = wy * Wxs[c]                          1
      acc += w * gv                            1    the product, when not fused
                                               n    additions at the most
    n + 4 factors: |acc - exact| <= (n + 5) u S.  Then cell += acc rounds once more, on the whole sum:
      out = (prefill + acc)(1 + d)  ->  |out - (prefill + exact)| <= (1 + u)(n + 5) u S + u |prefill + exact|
                                                                 <= (n + 6) u S + u |result|.                     C_BWD = 6
    A second launch onto that output (`second_bound`) adds the same once more: with b1 the bound above and e = (n + 5) u S,
      |out2 - (prefill + 2 exact)| <= (1 + u)(b1 + e) + u |prefill + 2 exact|.
An element with S = 0 has no term: the forward writes an exact zero, the backward must leave the prefill's bits alone.  The float64
sums of the reference err by n 2^-53 S, nine orders of magnitude below.  None of the constants was fitted to what a kernel returns.

Lattice cases (power-of-two grids only: 8 x 8, 16 x 16, 8 x 16, 16 x 8): map-space origins on quarter cells, sides in {1, 2, 4, 8} cells,
integer features, gradients and prefill in [-8, 8].  The normalised corner (q / 4 + 0.5) / 2^m is an fp32 number, count is a power of
two, every weight is a multiple of 1/4, every term w f / count a multiple of 2^-10, and every magnitude sum (prefill included) is below
2^14: each partial sum in any order is an fp32 number.  The builder checks this on the float64 terms (`exact`) and also evaluates both
directions once in np.float32 and requires the same bits; the expected output is then a bit pattern.  The first boxes of every lattice
case hang over each of the four borders by more than one cell (samples dropped below -1 / above size, samples clamped between).

Random cases: real-valued corners in about [-0.3, 1.3]: plain, tiny, near-whole-map, zero-size and inverted boxes (`KINDS`).  The
generator is deterministic and re-draws a box while (`violates`)
    the two coordinate forms give a different gh or gw, or
    a sample of either form lies within 1e-3 of -1 or of size, or
    an extent of either form lies within 1e-3 of an integer (the exact 0 of a zero-size box, whose two corners are one float, apart),
so that no decision of the algorithm (ceil, drop, clamp) hangs on the last bits of a coordinate; `violations(case)` counts the boxes
that still do, and every test requires 0.  That is a condition on the inputs, not a tolerance on the outputs.  Where the two forms
differ (`forms_differ`), the case also proves that they can be told apart: some element of each direction has references further apart
than the two bounds together.  Maps, gradients and the prefill are normal draws; three of every four channels of each are sparse (an
element is non-zero with probability 0.5, 0.12, 0.03; channels 0, 4, 8, .. are dense), so that some outputs consist of one or two terms
only: there S is that term alone, the bound is a few u of it, and an ulp of the box's coordinate in its weight is not hidden under the
other cells, boxes or the prefill.

Cases and the path of the kernels each one reaches (RB_CELLS = 16 cells per workgroup of the backward, 256 boxes per compaction chunk,
1024 channels per channel chunk of the backward and per trip of the forward's channel loop).  tok_off = 1 cases carry 3 tokens after
the grid and tok_off = 0 cases 2: both the CLS row and the trailing tokens must keep their prefill.  Image 1 has no box wherever
B > 1; image indices are drawn at random, so unsorted; in cases with K >= 256 the image `spread` owns boxes in every 64-box wave slot of
every chunk (asserted).
    lat_8x8_one       8 x 8    E 4     K 1     B 1   off 0    one float4, one box, one image
    lat_8x8_none      8 x 8    E 4     K 0     B 2   off 1    no boxes: nothing launched, every bit of the prefill kept
    lat_16x16_257     16 x 16  E 1028  K 257   B 3   off 1    exactly one cell group; second chunk of one box; ragged second channel chunk
    lat_8x16_600      8 x 16   E 260   K 600   B 4   off 1    h != w; three chunks; j = 1 of the channel loop partly filled
    lat_16x8_256      16 x 8   E 1024  K 256   B 3   off 0    w != h the other way, half a cell group; one full chunk, four full waves; one channel chunk exactly
    lat_8x16_b70      8 x 16   E 4     K 12    B 70  off 0    70 images, a dozen boxes: most workgroups find no box
    rnd_5x7           5 x 7    E 260   K 40    B 3   off 1    the swap pair: grid_w < 16, h != w
    rnd_7x5           7 x 5    ...                            rnd_5x7 transposed (map and boxes), built from it
    rnd_3x16          3 x 16   E 1024  K 256   B 3   off 0    exactly one cell group
    rnd_4x17          4 x 17   E 1028  K 257   B 3   off 1    a second cell group of one cell (the Wxs tail and the column guard)
    rnd_14x14_600     14 x 14  E 260   K 600   B 4   off 1    grid of the training recipe, not a power of two; three chunks
    rnd_24x24         24 x 24  E 260   K 200   B 2   off 0    two cell groups, the second half full; not a power of two
    rnd_16x8          16 x 8   E 260   K 257   B 3   off 0    random boxes where both coordinate forms are one float
    rnd_8x8_one       8 x 8    E 4     K 1     B 1   off 1    one random box
    rnd_14x14_b70     14 x 14  E 260   K 12    B 70  off 1    70 images
"""
import numpy as np

U = 2.0 ** -24
C_FWD, C_BWD = 5, 6
QUANTUM = 2.0 ** 10
FORMS = ("rounded", "fused")
MARGIN = 1e-3
DENSITY = (1.0, 0.5, 0.12, 0.03)
_f = np.float32


# ================================================================================================ coordinates and axis weights, np.float32
def map_coord(v, s, form):
    """v [..] normalised corners (np.float32), s the grid side -> the map coordinate in np.float32, in one of the two FORMS."""
    v = np.asarray(v, np.float32)
    if form == "rounded":
        p = (v * _f(s)).astype(np.float32)
        return (p - _f(0.5)).astype(np.float32)
    assert form == "fused"
    p = v.astype(np.float64) * float(s)                                       # exact: 24 bits times at most 8
    assert ((p == 0) | (np.abs(p) >= 2.0 ** -20)).all(), "v * s - 0.5 would not be exact in float64"
    return (p - 0.5).astype(np.float32)                                       # the one rounding


def axis_weights(start, extent, grid, size):
    """The kernel file's axis_weights(), scalar and in sample order -> (w [size] np.float32, the samples' coordinates before the clamp)."""
    w = np.zeros(size, np.float32)
    cs = []
    for i in range(max(grid, 0)):
        c = _f(start + _f(_f(_f(_f(i) + _f(0.5)) * extent) / _f(grid)))
        cs.append(float(c))
        if c < -1.0 or c > size:
            continue
        if c <= 0:
            c = _f(0)
        lo = int(c)
        if lo >= size - 1:
            hi = lo = size - 1
            c = _f(lo)
        else:
            hi = lo + 1
        l = _f(c - _f(lo))
        w[lo] = _f(w[lo] + _f(_f(1) - l))
        w[hi] = _f(w[hi] + l)
    return w, cs


def geometry(rois, h, w, form):
    """-> dict(b, gh, gw [K] int, count [K] float, Wy [K, h], Wx [K, w] np.float32, rh, rw [K] np.float32, ys, xs: K lists of samples)."""
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    K = len(rois)
    x0, y0 = map_coord(rois[:, 1], w, form), map_coord(rois[:, 2], h, form)
    x1, y1 = map_coord(rois[:, 3], w, form), map_coord(rois[:, 4], h, form)
    rw, rh = (x1 - x0).astype(np.float32), (y1 - y0).astype(np.float32)
    gh, gw = np.ceil(rh).astype(np.int64), np.ceil(rw).astype(np.int64)
    Wy, Wx = np.zeros((K, h), np.float32), np.zeros((K, w), np.float32)
    ys, xs = [], []
    for k in range(K):
        Wy[k], cy = axis_weights(y0[k], rh[k], int(gh[k]), h)
        Wx[k], cx = axis_weights(x0[k], rw[k], int(gw[k]), w)
        ys.append(cy)
        xs.append(cx)
    return dict(b=rois[:, 0].astype(np.int64), gh=gh, gw=gw, count=np.maximum(gh * gw, 1).astype(np.float64), Wy=Wy, Wx=Wx, rh=rh, rw=rw,
                ys=ys, xs=xs, form=form)


def _pow2(n):
    return n & (n - 1) == 0


def geometry_both(rois, h, w):
    """{form: geometry}.  Where both grid sides are powers of two the two forms must be the same floats: one geometry, twice."""
    g = {f: geometry(rois, h, w, f) for f in FORMS}
    if _pow2(h) and _pow2(w):
        a, b = g["rounded"], g["fused"]
        assert np.array_equal(a["Wy"].view(np.int32), b["Wy"].view(np.int32)) and np.array_equal(a["Wx"].view(np.int32), b["Wx"].view(np.int32))
        assert np.array_equal(a["rh"].view(np.int32), b["rh"].view(np.int32)) and np.array_equal(a["rw"].view(np.int32), b["rw"].view(np.int32))
        g["fused"] = g["rounded"]
    return g


def forms_differ(geos):
    return geos["fused"] is not geos["rounded"]


# ================================================================================================ the re-draw rule
def violates(roi, h, w):
    """The generator's rule for one box (module docstring) -> a word naming the first condition it breaks, or None."""
    g = [geometry(roi, h, w, f) for f in FORMS]
    if int(g[0]["gh"][0]) != int(g[1]["gh"][0]) or int(g[0]["gw"][0]) != int(g[1]["gw"][0]):
        return "grid"
    roi = np.asarray(roi, np.float32).reshape(5)
    for a in g:
        for cs, size in ((a["ys"][0], h), (a["xs"][0], w)):
            for c in cs:
                if abs(c + 1.0) < MARGIN or abs(c - size) < MARGIN:
                    return "sample"
        for ext, same in ((float(a["rh"][0]), roi[2] == roi[4]), (float(a["rw"][0]), roi[1] == roi[3])):
            if same and ext == 0.0:
                continue                                                       # a zero-size box: both corners are one float, the extent is an exact 0 in both forms
            if abs(ext - round(ext)) < MARGIN:
                return "extent"
    return None


def violations(c):
    """Number of boxes of a case that break the rule."""
    return sum(violates(r, c["h"], c["w"]) is not None for r in c["rois"])


KINDS = ("plain", "tiny", "whole", "zero", "inverted")


def _draw(r, kind):
    """One box (x0, y0, x1, y1) of a kind, normalised."""
    if kind == "plain":
        x0, y0 = r.uniform(-0.3, 1.0, 2)
        ew, eh = r.uniform(0.03, 0.7, 2)
        return [x0, y0, min(x0 + ew, 1.3), min(y0 + eh, 1.3)]
    if kind == "tiny":
        x0, y0 = r.uniform(-0.05, 1.05, 2)
        ew, eh = r.uniform(1e-4, 0.02, 2)
        return [x0, y0, x0 + ew, y0 + eh]
    if kind == "whole":
        a = r.uniform(0.001, 0.03, 4)
        return [a[0], a[1], 1.0 - a[2], 1.0 - a[3]]
    x0, y0 = r.uniform(0.0, 0.8, 2)
    ew, eh = r.uniform(0.05, 0.4, 2)
    which = r.randint(0, 3)                                                    # x, y or both
    if kind == "zero":
        return [x0, y0, x0 if which != 1 else x0 + ew, y0 if which != 0 else y0 + eh]
    assert kind == "inverted"
    return [x0, y0, x0 - ew if which != 1 else x0 + ew, y0 - eh if which != 0 else y0 + eh]


def box_kinds(K):
    """The kind of every box: boxes 1, 2, 3 and 5 of every 16 are tiny, near-whole-map, zero-size and inverted, the others plain."""
    special = {1: "tiny", 2: "whole", 3: "zero", 5: "inverted"}
    return [special.get(k % 16, "plain") for k in range(K)]


def image_indices(r, K, B, empty):
    imgs = np.array([b for b in range(B) if b not in empty])
    return imgs[r.randint(0, len(imgs), K)]


def random_rois(K, B, h, w, seed, empty=()):
    """[K, 5] np.float32 -- deterministic; every box re-drawn until it meets the rule."""
    r = np.random.RandomState(seed)
    rois = np.zeros((K, 5), np.float32)
    rois[:, 0] = image_indices(r, K, B, empty)
    for k, kind in enumerate(box_kinds(K)):
        for _ in range(1000):
            rois[k, 1:] = _draw(r, kind)
            if violates(rois[k], h, w) is None:
                break
        else:
            raise AssertionError(f"box {k} ({kind}) found no draw that meets the rule")
    return rois


def lattice_rois(K, B, h, w, seed, empty=()):
    """[K, 5] np.float32: map-space origins q / 4 (q integer) from a box's own side + 2 cells before the map to 2 cells past it, sides in
    {1, 2, 4, 8} cells drawn per axis; the first boxes hang over the left, right, top and bottom border by more than a cell."""
    r = np.random.RandomState(seed)
    sw, sh = 2 ** r.randint(0, 4, K), 2 ** r.randint(0, 4, K)
    qx = np.array([r.randint(-4 * (s + 2), 4 * (w + 2) + 1) for s in sw])
    qy = np.array([r.randint(-4 * (s + 2), 4 * (h + 2) + 1) for s in sh])
    over = [(4, 4, -9, -10), (4, 2, 4 * w - 7, 3), (2, 4, 5, -10), (8, 4, 2, 4 * h - 5), (8, 8, -13, -11), (4, 4, 4 * w - 6, 4 * h - 5)]
    for k, (a, b, x, y) in enumerate(over[:K]):
        sw[k], sh[k], qx[k], qy[k] = a, b, x, y
    rois = np.zeros((K, 5), np.float32)
    rois[:, 0] = image_indices(r, K, B, empty)
    rois[:, 1], rois[:, 2] = (qx / 4.0 + 0.5) / w, (qy / 4.0 + 0.5) / h
    rois[:, 3], rois[:, 4] = (qx / 4.0 + sw + 0.5) / w, (qy / 4.0 + sh + 0.5) / h
    g = geometry(rois, h, w, "rounded")                                        # the draw is what it says: exact sides, exact quarter-cell weights
    assert (g["rw"] == sw).all() and (g["rh"] == sh).all() and (g["gw"] == sw).all() and (g["gh"] == sh).all()
    assert (g["Wy"] * 4 == np.round(g["Wy"] * 4)).all() and (g["Wx"] * 4 == np.round(g["Wx"] * 4)).all()
    return rois


# ================================================================================================ float64 references with the bound
def _rect(wy, wx):
    r, c = np.nonzero(wy)[0], np.nonzero(wx)[0]
    if len(r) == 0 or len(c) == 0:
        return None
    return slice(r[0], r[-1] + 1), slice(c[0], c[-1] + 1)


def forward_ref(fmap, geo, fp32_too=False):
    """fmap [B, h, w, E] -> dict(out, mag, n, bound [K, E] float64, exact bool); mag = sum |w f| / count, bound = (n + C_FWD) u mag."""
    K, E = len(geo["b"]), fmap.shape[-1]
    out, mag, n = np.zeros((K, E)), np.zeros((K, E)), np.zeros((K, E))
    exact = True
    for k in range(K):
        if geo["gh"][k] <= 0 or geo["gw"][k] <= 0:
            continue
        rc = _rect(geo["Wy"][k], geo["Wx"][k])
        if rc is None:
            continue
        W = np.multiply.outer(geo["Wy"][k][rc[0]].astype(np.float64), geo["Wx"][k][rc[1]].astype(np.float64))
        F = fmap[geo["b"][k]][rc].astype(np.float64)
        term = W[..., None] * F / geo["count"][k]
        out[k], mag[k], n[k] = term.sum((0, 1)), np.abs(term).sum((0, 1)), (term != 0).sum((0, 1))
        exact = exact and bool((term * QUANTUM == np.round(term * QUANTUM)).all())
        if fp32_too:                                                           # the same sum in np.float32, as a kernel would: the same bits
            W32 = np.multiply.outer(geo["Wy"][k][rc[0]], geo["Wx"][k][rc[1]]).astype(np.float32)
            acc = (W32[..., None] * fmap[geo["b"][k]][rc]).astype(np.float32).reshape(-1, E)
            s = np.zeros(E, np.float32)
            for row in acc:
                s = (s + row).astype(np.float32)
            s = (s * (_f(1) / _f(geo["count"][k]))).astype(np.float32)
            exact = exact and bool((s.astype(np.float64) == out[k]).all())
    assert n.max(initial=0) + C_FWD - 1 <= 4000
    exact = exact and bool(mag.max(initial=0) < 2.0 ** 14)
    return dict(out=out, mag=mag, n=n, bound=(n + C_FWD) * U * mag, exact=exact)


def backward_ref(dP, geo, B, h, w, fp32_too=False):
    """dP [K, E] -> dict(d, mag, n [B, h, w, E] float64, acc_bound = (n + C_BWD - 1) u mag, bound0 = (n + C_BWD) u mag, exact);
    the bound of an output is bound0 + u |prefill + d| (`backward_bound`)."""
    K, E = dP.shape
    d, mag, n = np.zeros((B, h, w, E)), np.zeros((B, h, w, E)), np.zeros((B, h, w, E))
    d32 = np.zeros((B, h, w, E), np.float32) if fp32_too else None
    exact = True
    for k in range(K):
        if geo["gh"][k] <= 0 or geo["gw"][k] <= 0:
            continue
        rc = _rect(geo["Wy"][k], geo["Wx"][k])
        if rc is None:
            continue
        b = geo["b"][k]
        W = np.multiply.outer(geo["Wy"][k][rc[0]].astype(np.float64), geo["Wx"][k][rc[1]].astype(np.float64))
        term = W[..., None] * (dP[k].astype(np.float64) / geo["count"][k])
        d[b][rc] += term
        mag[b][rc] += np.abs(term)
        n[b][rc] += term != 0
        exact = exact and bool((term * QUANTUM == np.round(term * QUANTUM)).all())
        if fp32_too:
            W32 = np.multiply.outer(geo["Wy"][k][rc[0]], geo["Wx"][k][rc[1]]).astype(np.float32)
            gv = (dP[k] * (_f(1) / _f(geo["count"][k]))).astype(np.float32)
            d32[b][rc] = (d32[b][rc] + (W32[..., None] * gv).astype(np.float32)).astype(np.float32)
    assert n.max(initial=0) + C_BWD - 1 <= 4000
    exact = exact and bool(mag.max(initial=0) < 2.0 ** 14)
    if fp32_too:
        exact = exact and bool((d32.astype(np.float64) == d).all())
    return dict(d=d, mag=mag, n=n, acc_bound=(n + C_BWD - 1) * U * mag, bound0=(n + C_BWD) * U * mag, exact=exact)


def backward_bound(bwd, prefill_grid):
    """Bound of dfeat after one launch onto prefill_grid [B, h, w, E]."""
    return bwd["bound0"] + U * np.abs(prefill_grid.astype(np.float64) + bwd["d"])


def second_bound(bwd, prefill_grid):
    """Bound of dfeat after a second launch onto the first one's output, against prefill + 2 d."""
    p = prefill_grid.astype(np.float64)
    return (1 + U) * (backward_bound(bwd, prefill_grid) + bwd["acc_bound"]) + U * np.abs(p + 2 * bwd["d"])


# ================================================================================================ cases
#   name: (lattice, (h, w), E, K, B, tok_off, seed)
CASES = {
    "lat_8x8_one":    (True, (8, 8), 4, 1, 1, 0, 1),
    "lat_8x8_none":   (True, (8, 8), 4, 0, 2, 1, 2),
    "lat_16x16_257":  (True, (16, 16), 1028, 257, 3, 1, 3),
    "lat_8x16_600":   (True, (8, 16), 260, 600, 4, 1, 4),
    "lat_16x8_256":   (True, (16, 8), 1024, 256, 3, 0, 5),
    "lat_8x16_b70":   (True, (8, 16), 4, 12, 70, 0, 6),
    "rnd_5x7":        (False, (5, 7), 260, 40, 3, 1, 11),
    "rnd_7x5":        (False, (7, 5), 260, 40, 3, 1, 11),                      # rnd_5x7 transposed
    "rnd_3x16":       (False, (3, 16), 1024, 256, 3, 0, 13),
    "rnd_4x17":       (False, (4, 17), 1028, 257, 3, 1, 14),
    "rnd_14x14_600":  (False, (14, 14), 260, 600, 4, 1, 15),
    "rnd_24x24":      (False, (24, 24), 260, 200, 2, 0, 16),
    "rnd_16x8":       (False, (16, 8), 260, 257, 3, 0, 17),
    "rnd_8x8_one":    (False, (8, 8), 4, 1, 1, 1, 18),
    "rnd_14x14_b70":  (False, (14, 14), 260, 12, 70, 1, 19),
}
LATTICE = [n for n, c in CASES.items() if c[0]]
RANDOM = [n for n, c in CASES.items() if not c[0]]
RANDOM_POW2 = [n for n in RANDOM if _pow2(CASES[n][1][0]) and _pow2(CASES[n][1][1])]
RANDOM_OTHER = [n for n in RANDOM if n not in RANDOM_POW2]
SWAP_PAIR = ("rnd_5x7", "rnd_7x5")
MANY_BOXES = ("lat_8x16_600", "rnd_14x14_600")
_memo = {}


def tail_tokens(tok_off):
    return 3 if tok_off else 2


def grid_of(c, tokens):
    """[B, Ntok, E] -> the grid's tokens as [B, h, w, E] (a view)."""
    return tokens[:, c["tok_off"]:c["tok_off"] + c["h"] * c["w"]].reshape(c["B"], c["h"], c["w"], c["E"])


def transpose_case_inputs(c):
    """Inputs of the transposed problem: the map's rows become columns, the boxes' x becomes y; gradient, prefill tokens outside the grid,
    image indices and box order stay."""
    t = dict(h=c["w"], w=c["h"], E=c["E"], K=c["K"], B=c["B"], tok_off=c["tok_off"], Ntok=c["Ntok"], empty=c["empty"], spread=c["spread"])
    t["rois"] = np.ascontiguousarray(c["rois"][:, [0, 2, 1, 4, 3]])
    for key in ("feat", "prefill"):
        a = c[key].copy()
        grid_of(t, a)[...] = grid_of(c, c[key]).transpose(0, 2, 1, 3)
        t[key] = a
    t["dP"] = c["dP"]
    return t


def _inputs(name):
    lattice, (h, w), E, K, B, tok_off, seed = CASES[name]
    empty = (1,) if B > 1 else ()
    Ntok = tok_off + h * w + tail_tokens(tok_off)
    r = np.random.RandomState(seed + 100)
    c = dict(h=h, w=w, E=E, K=K, B=B, tok_off=tok_off, Ntok=Ntok, empty=empty, spread=None)
    if lattice:
        c["rois"] = lattice_rois(K, B, h, w, seed, empty)
        draw = lambda *s: r.randint(-8, 9, s).astype(np.float32)
    else:
        c["rois"] = random_rois(K, B, h, w, seed, empty)
        draw = lambda *s: r.randn(*s).astype(np.float32)
    c["feat"], c["dP"], c["prefill"] = draw(B, Ntok, E), draw(K, E), draw(B, Ntok, E)
    if not lattice:                                                            # channel e keeps a cell with probability DENSITY[e % 4]: see the docstring
        c["feat"] *= r.rand(B, Ntok, E) < np.array(DENSITY)[np.arange(E) % 4]
        c["dP"] *= r.rand(K, E) < np.array(DENSITY)[np.arange(E) % 4]
        c["prefill"] *= r.rand(B, Ntok, E) < np.array(DENSITY)[np.arange(E) % 4]
    if K >= 256:                                                               # one image with boxes in every wave slot of every chunk
        img = c["rois"][:, 0].astype(np.int64)
        c["spread"] = int(np.bincount(img).argmax())
        c["rois"][K - 1, 0] = c["spread"]                                      # K = 257: the one box of the second chunk
        img = c["rois"][:, 0].astype(np.int64)
        for s in range(0, K, 64):
            assert (img[s:s + 64] == c["spread"]).any(), (name, s)
        assert (np.diff(img) < 0).any() and (np.diff(img) > 0).any()           # unsorted
    return c


def build_case(name):
    """Inputs and the float64 references of one case, computed once per process and shared: treat every array as read-only.
    c["ref"][form] = dict(geo, fwd, bwd); both forms are one object on a power-of-two grid."""
    if name in _memo:
        return _memo[name]
    lattice = CASES[name][0]
    c = transpose_case_inputs(build_case(SWAP_PAIR[0])) if name == SWAP_PAIR[1] else _inputs(name)
    c.update(name=name, lattice=lattice, pow2=_pow2(c["h"]) and _pow2(c["w"]))
    assert (c["h"], c["w"], c["E"], c["K"], c["B"], c["tok_off"]) == (CASES[name][1] + CASES[name][2:6])
    img = c["rois"][:, 0]
    assert ((img >= 0) & (img < c["B"])).all() and not np.isin(img, c["empty"]).any()      # the plain launch does not check image indices
    geos = geometry_both(c["rois"], c["h"], c["w"])
    assert lattice <= c["pow2"] and forms_differ(geos) == (not c["pow2"])
    fmap = grid_of(c, c["feat"])
    ref = {}
    for form in FORMS:
        if form == "fused" and not forms_differ(geos):
            ref[form] = ref["rounded"]
            continue
        ref[form] = dict(geo=geos[form], fwd=forward_ref(fmap, geos[form], fp32_too=lattice),
                         bwd=backward_ref(c["dP"], geos[form], c["B"], c["h"], c["w"], fp32_too=lattice))
    c["ref"] = ref
    if lattice:
        pre = np.abs(grid_of(c, c["prefill"]).astype(np.float64))
        c["exact"] = ref["rounded"]["fwd"]["exact"] and ref["rounded"]["bwd"]["exact"] and bool((2 * ref["rounded"]["bwd"]["mag"] + pre).max(initial=0) < 2.0 ** 14)
    _memo[name] = c
    return c


def distinguishable(c):
    """(forward, backward): does some element have the two forms' references further apart than their two bounds together?  Then at most
    one form can hold a whole launch inside its bound."""
    a, b = c["ref"]["rounded"], c["ref"]["fused"]
    pre = grid_of(c, c["prefill"])
    f = np.abs(a["fwd"]["out"] - b["fwd"]["out"]) > a["fwd"]["bound"] + b["fwd"]["bound"]
    g = np.abs(a["bwd"]["d"] - b["bwd"]["d"]) > backward_bound(a["bwd"], pre) + backward_bound(b["bwd"], pre)
    return bool(f.any()), bool(g.any())


# ================================================================================================ comparisons
def expected_tokens(c, form, times=1):
    """prefill + times * gradient as [B, Ntok, E] float64: the prefill everywhere outside the grid."""
    want = c["prefill"].astype(np.float64)
    grid_of(c, want)[...] += times * c["ref"][form]["bwd"]["d"]
    return want


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(got, want64, what):
    """got (np.float32) holds exactly the numbers want64 (float64), signed zeros included where want64 came from fp32 values."""
    want = want64.astype(np.float32)
    assert (want.astype(np.float64) == want64).all(), f"{what}: the expected values are not fp32 numbers"
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, first at {np.argwhere(bad)[0].tolist()}"


def fraction(got, want, bound):
    """-> worst |got - want| / bound over the elements with a bound (inf if an element without one is off at all)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    if not np.isfinite(err).all() or (err[bound == 0] != 0).any():
        return float("inf")
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def forward_fraction(c, form, pooled):
    f = c["ref"][form]["fwd"]
    return fraction(pooled, f["out"], f["bound"])


def backward_fraction(c, form, dfeat, prefill=None, times=1):
    """dfeat [B, Ntok, E] np.float32 after `times` (1 or 2) launches onto prefill (the case's own by default): the worst fraction of the
    bound over the grid; inf if a token outside the grid, or a cell no box reaches, lost a bit of its prefill."""
    prefill = c["prefill"] if prefill is None else prefill
    b = c["ref"][form]["bwd"]
    pg = grid_of(c, prefill)
    untouched = np.ones(prefill.shape, bool)
    grid_of(c, untouched)[...] = b["mag"] == 0
    if (_bits(dfeat)[untouched] != _bits(prefill)[untouched]).any():
        return float("inf")
    bound = backward_bound(b, pg) if times == 1 else second_bound(b, pg)
    return fraction(grid_of(c, dfeat), pg.astype(np.float64) + times * b["d"], np.where(b["mag"] == 0, 0.0, bound))
