"""TEST INFRASTRUCTURE -- float64 restatement of the reference's open-vocabulary scoring tail and the bound its fp32 evaluations are held to
(clipself_amd/ov_head.py, cs_roialign_fwd's scoring form).

Restated lines (F-ViT/models/fvit_head.py):
  :276      vlm_roi_extractor([vlm_feat], rois)[..., 0, 0]: RoIAlign 1x1, aligned, adaptive, spatial_scale = 1 / 16 -- pooled here through
            oracle.roi_align_ref.roi_align_1x1 on box coordinates scaled in float32, np.float32(x) * np.float32(scale), as torchvision's
            T = float does;
  :68       F.normalize(vlm_box_feats, dim=-1, p=2)                (eps 1e-12);
  :112-114  cls_score.softmax(-1);  (normalized @ all_embed * vlm_temperature).softmax(-1);
  :116-119  cls_score[:, idx] ** (1 - p) * vlm_score[:, idx] ** p  with p = alpha on base and beta on novel classes -- the literal
            softmax() ** p product, on a per-class exponent vector;
  :337-345  the transfer head: the same with one exponent.
VLM-only scores (cls_score None) are :113-114 alone.  Boxes the kernel contract scores as EMPTY -- image index outside [0, B), extent on
the map not in (0, 2 * grid side] on an axis, non-finite coordinates -- pool to 0 here as well, so their VLM distribution is uniform
(F.normalize of a zero vector is zero); that rule is the project's, not the reference's.

THE BOUND, per element, on log out.  u = 2^-24.  An fp32 accumulation of n terms in any order, fused or not, errs by at most
n * u * sum|terms| to first order (Higham, Accuracy and Stability of Numerical Algorithms, §3.1); as in tests/_neck_ref.py a factor 2
covers the higher orders.  Inputs (map, boxes, embeddings, detector logits, exponents) are the same fp32 values on both sides, and the
per-sample bilinear weights are computed by the same un-contracted fp32 steps on both sides, so errors start at the first sum.

  pooling   v_e = sum over touched cells of Wy[r] * Wx[c] * F[r, c, e] / count.  Wy[r] (Wx[c]) is an fp32 sum of at most gh (gw) sample
            weights, the product Wy * Wx, 1 / count and the final multiplication are one rounding each, and the cell sum has
            cells <= min(h, gh + 1) * min(w, gw + 1) terms:      dv_e = 2 * (gh + gw + cells + 4) * u * sum|terms|_e,
            sum|terms|_e = the same pooling of |F|.  (The fallback route of ov_head.py pools sample by sample -- four products per
            sample, each weight product, the division by count and the multiplication one rounding -- so there the term count is
            4 * gh * gw + 3: `pool_terms="samples"`.)
  norm      n = sqrt(sum v_e^2): the sum of E non-negative terms has relative error E * u, the square root halves it and adds u, the
            perturbation of v moves n by at most |dv|_2:         dn / n = |dv|_2 / n + 2 * (E + 2) * u
            v^_e = v_e / n, one more rounding:                   dv^_e = dv_e / n + |v^_e| * (dn / n + 2 * u)
  logit     z_c = T * sum_e v^_e * A[c, e], E terms, then one rounding for T:
                                                                 dz_c = T * (sum_e dv^_e |A_ce| + 2 * E * u * sum_e |v^_e A_ce|) + 2 * u * |z_c|
  softmax   |d log softmax(z)_c| <= 2 * max_c dz_c for a perturbation of z (the logit moves by at most max dz, the log-sum-exp by at most
            max dz).  Evaluating log softmax in fp32 from exact z, with Z = max|z|: the argument z - max is rounded (u * 2Z, which the
            exponential turns into a relative error), expf is good to 1 ulp (2u), the sum of C positive terms adds C * u, logf of a sum
            in [1, C] is good to 1 ulp (2u * log C), max + log and z - lse are one rounding each (u * (Z + log C), u * (2Z + log C)):
                                                                 tls(Z, C) = 2 * u * (5 * Z + C + 2 + 4 * log C)
            (fp32 softmax as p = exp(z - max) / sum followed by a log has the same terms and one division, inside the factor 2).
  blend     with ld = log softmax(det), lv = log softmax(z) and exponent w:  log out = (1 - w) * ld + w * lv.  Log-domain form: 1 - w and
            the two products and the sum are roundings of terms no larger than (1 - w)|ld| + w|lv|, expf is 1 ulp.  Product form
            (softmax() ** p in fp32): two powf at 1 ulp, two divisions, one multiplication = 7 u, 1 - w one rounding.  Both inside
                                                                 tb = 2 * u * (3 * ((1 - w)|ld| + w|lv|) + 7)
  total     bound(log out) = (1 - w) * 2 * dd + w * 2 * dv_max + tau, with the detector's logits exact inputs, so that
            2 * dd = tls(max|det|, C) is the whole detector term, dv_max = max_c dz_c, and tau = w * tls(max|z|, C) + tb.
            VLM-only scores are the case w = 1.

A score below the fp32 minimum normal 2^-126 has no fp32 logarithm to speak of (it is subnormal or zero): such elements compare
absolutely, |got - want| <= 2^-126.  No constant above is tuned to a measurement."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.roi_align_ref import _box_f32, roi_align_1x1

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def scale_rois(rois, scale):
    """Pixel rois [K, 5] -> map coordinates, the product rounded to float32 like torchvision's T = float."""
    r = np.asarray(rois, dtype=np.float32).copy()
    r[:, 1:] = r[:, 1:] * np.float32(scale)
    return r


def box_geometry(scaled, B, h, w):
    """Per box: (walk, gh, gw, cells) by the kernel contract's rule, in float32 like the kernel."""
    out = []
    for row in scaled:
        _, _, rw, rh = _box_f32([float(v) for v in row])
        b = float(row[0])
        walk = (0 <= b < B) and (0 < rh <= 2 * h) and (0 < rw <= 2 * w)                # NaN compares false
        gh, gw = (math.ceil(rh), math.ceil(rw)) if walk else (0, 0)
        out.append((walk, gh, gw, min(h, gh + 1) * min(w, gw + 1)))
    return out


class Reference:
    pass


def tls(Z, C):
    return 2.0 * U * (5.0 * Z + C + 2.0 + 4.0 * math.log(C))


def reference(feat, rois, scale, embed, vlm_temp, det=None, expo=None, pool_terms="cells"):
    """feat [B, h, w, E] fp32 map, rois [K, 5] pixel boxes, embed [C, E] fp32 class rows, det [K, C] fp32 logits | None, expo [C] fp32.
    pool_terms: the form of the pooling sum under test -- "cells" (the kernels: folded axis weights, one term per touched cell) or
    "samples" (roi_align_1x1 in fp32, the fallback route: four terms per sample).
    -> Reference with pooled, dpool [K, E], z, dz, out, log_out, bound [K, C] (float64)."""
    B, h, w, E = feat.shape
    C, K = embed.shape[0], len(rois)
    scaled = scale_rois(rois, scale)
    geo = box_geometry(scaled, B, h, w)
    f64 = feat.double()
    pooled, apooled, npool = torch.zeros(K, E, dtype=F64), torch.zeros(K, E, dtype=F64), torch.zeros(K, dtype=F64)
    idx = [k for k in range(K) if geo[k][0]]
    if idx:
        r = torch.from_numpy(scaled[idx]).double()
        pooled[idx] = roi_align_1x1(f64, r)                                            # :276
        apooled[idx] = roi_align_1x1(f64.abs(), r)
        npool[idx] = torch.tensor([geo[k][1] + geo[k][2] + geo[k][3] + 4.0 if pool_terms == "cells" else 4.0 * geo[k][1] * geo[k][2] + 3.0
                                   for k in idx], dtype=F64)
    ref = Reference()
    ref.pooled, ref.dpool = pooled, 2.0 * npool[:, None] * U * apooled
    A = embed.double()
    n = pooled.norm(dim=1, keepdim=True).clamp_min(1e-12)
    vh = pooled / n                                                                    # :68
    dn = ref.dpool.norm(dim=1, keepdim=True) / n + 2.0 * (E + 2) * U
    dvh = ref.dpool / n + vh.abs() * (dn + 2.0 * U)
    z = vh @ A.t() * vlm_temp                                                          # :113
    ref.z = z
    ref.dz = vlm_temp * (dvh @ A.abs().t() + 2.0 * E * U * (vh.abs() @ A.abs().t())) + 2.0 * U * z.abs()
    vlm = z.softmax(dim=-1)                                                            # :114
    lv = vlm.log()
    dvmax = ref.dz.max(dim=1, keepdim=True).values
    tv = torch.tensor([tls(float(z[k].abs().max()), C) for k in range(K)], dtype=F64)[:, None] if K else torch.zeros(0, 1, dtype=F64)
    if det is None:
        ref.out = vlm
        ref.log_out = lv
        ref.bound = 2.0 * dvmax + tv + 2.0 * U * (3.0 * lv.abs() + 7.0)
        return ref
    d64, wv = det.double(), expo.double()[None, :]
    sm = d64.softmax(dim=-1)                                                           # :112
    ld = sm.log()
    ref.out = sm ** (1 - wv) * vlm ** wv                                               # :116-119 / :345
    ref.log_out = ref.out.log()
    td = torch.tensor([tls(float(d64[k].abs().max()), C) for k in range(K)], dtype=F64)[:, None] if K else torch.zeros(0, 1, dtype=F64)
    tb = 2.0 * U * (3.0 * ((1 - wv) * ld.abs() + wv * lv.abs()) + 7.0)
    ref.bound = (1 - wv) * td + wv * (2.0 * dvmax + tv) + tb
    return ref


def worst_ratio(got, ref):
    """-> (worst |log got - log want| / bound over the normal-range elements, count of elements past their bound), subnormal-range
    elements compared absolutely and counted as ratio |got - want| / 2^-126."""
    got = got.detach().double().cpu()
    assert got.shape == ref.out.shape, (got.shape, ref.out.shape)
    if got.numel() == 0:
        return 0.0, 0
    small = ref.out < FLT_MIN
    with np.errstate(all="ignore"):
        rlog = (got.log() - ref.log_out).abs() / ref.bound
    rabs = (got - ref.out).abs() / FLT_MIN
    ratio = torch.where(small, rabs, rlog)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()), int((ratio > 1.0).sum())


def check(name, got, ref):
    worst, bad = worst_ratio(got, ref)
    print(f"OV SCORES {name}: worst err / bound {worst:.4f} over {ref.out.numel()} scores")
    assert bad == 0, f"{name}: {bad} of {ref.out.numel()} scores past the bound, worst ratio {worst:.3f}"
    return worst


def check_pooled(name, got, ref):
    err = (got.detach().double().cpu() - ref.pooled).abs()
    tol = ref.dpool + 2.0 * U * ref.pooled.abs()                                        # the stored value's own rounding
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"OV SCORES {name} pooled: worst err / bound {worst:.4f}")
    assert bool((err <= tol).all()), f"{name}: pooled features past the bound, worst ratio {worst:.3f}"


# ------------------------------------------------------------------------------------------------ seeded cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_boxes(B, K, h, w, stride, gen, lattice=None):
    """[K, 5] pixel boxes, images interleaved (k % B): centres anywhere on (and a little beyond) the image, sides from a few pixels to
    most of it.  lattice: snap coordinates to multiples of it."""
    W, H = w * stride, h * stride
    c = torch.rand(K, 2, generator=gen) * torch.tensor([W * 1.2, H * 1.2]) - torch.tensor([W * 0.1, H * 0.1])
    s = (torch.rand(K, 2, generator=gen) ** 2 * 0.9 + 0.02) * torch.tensor([float(W), float(H)])
    box = torch.cat([c - s / 2, c + s / 2], dim=1)
    if lattice:
        box = (box / lattice).round() * lattice
        box[:, 2:] = torch.maximum(box[:, 2:], box[:, :2] + lattice)
    return torch.cat([(torch.arange(K) % B).float()[:, None], box], dim=1).contiguous()


def make_case(B, h, w, E, C, K, seed, stride=16, lattice=None):
    """-> feat [B, h, w, E] (unit rows, like the tower's dense map), rois [K, 5], embed [C, E] (unit rows), det [K, C]."""
    g = _gen(seed)
    feat = F.normalize(torch.randn(B, h, w, E, generator=g), dim=-1)
    embed = F.normalize(torch.randn(C, E, generator=g), dim=-1)
    rois = make_boxes(B, K, h, w, stride, g, lattice)
    det = torch.randn(K, C, generator=g) * 4.0
    return feat, rois, embed, det


def split_exponents(C, alpha, beta, every=3):
    """alpha on base classes, beta on every `every`-th class (novel); the last class (background) is base."""
    w = torch.full((C,), alpha, dtype=F32)
    w[1:C - 1:every] = beta
    return w


def needle_case(B, h, w, E):
    """Background direction e_0 everywhere, the needle direction e_1 in rows 2-3 x columns 4-5 of image 1; class rows e_0, e_1, e_2; boxes
    (stride 16) on the needle, beside it, and at its place in the other image."""
    feat = torch.zeros(B, h, w, E)
    feat[..., 0] = 1.0
    feat[1, 2:4, 4:6, 0] = 0.0
    feat[1, 2:4, 4:6, 1] = 1.0
    rois = torch.tensor([[1.0, 64, 32, 96, 64], [1.0, 0, 32, 32, 64], [0.0, 64, 32, 96, 64]])
    return feat, rois, torch.eye(E)[:3].contiguous()
