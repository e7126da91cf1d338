"""Two statements of the detector-loss contract (include/clipself_loss.h), tested against each other on the CPU
(tests/test_det_losses_cpu.py), and the bounds the GPU tests use (tests/test_gpu_det_losses.py).

(a) `rpn_mmdet` / `head_mmdet`: mmdet 2.28.1's expressions transcribed in torch float64 with autograd -- permute / reshape of the
    predictions, _expand_onehot_labels + F.binary_cross_entropy_with_logits, the reference's cross_entropy (F.cross_entropy(weight=) on
    a copy whose masked columns hold -inf), L1 on the positive rows, weight_reduce_loss with its eps, accuracy through topk.  They run
    on inputs where the header's departures do not apply (finite predictions, labels in range and unmasked, no tied maximum).
(b) `rpn_ref` / `head_ref`: closed-form numpy float64 losses and gradients; they also state the departures (the zero-weight rule, labels
    outside their range, masked labels, ties to the lowest index) and return, next to every value, the bound below.

Bounds.  u = 2^-24 is the fp32 unit roundoff: one rounded operation errs by at most u |result|.  The device library documents expf, logf
and log1pf at 1 ulp, i.e. a relative error of at most 2u.  den = fl(avg + 2^-23) is the same fp32 number on both sides (one rounding of an
exact sum), so it carries no error; (a) is compared with (b) at the unrounded den (den_exact=True).  Second-order terms are covered by one
extra u on the last factor of each bound; TINY = 2^-100 per term covers a flushed subnormal expf.

  RPN objectness, t in {0, 1}:  a = max(x, 0) - x t is exact (it is x, -x or 0).  e = expf(-|x|): relative 2u.  l = log1pf(e): the true
    log1p changes by at most the relative change of e (e / ((1 + e) log1p(e)) <= 1), plus its own 2u: relative 4u.  fl(a + l): u (a + l);
    times lw: u.       |term - TERM| <= 7u |TERM|                                                              [4u l + 2u (a + l) <= 6u, + u]
    sigmoid: fl(1 + e) errs by 2u e + u (1 + e) <= 3u (1 + e); the division u; for x < 0 the numerator e adds 2u: relative 6u.
    fl(sig - t): 6u sig + u |sig - t|; times lw and / den: 2u.
                       |g - G| <= (|lw| / den) (6u SIG + u |SIG - t|) + 3u |G|
  L1: d = fl(pred - target): u |d|; times bw: u.          |term - TERM| <= 3u |TERM|.
    The sign of d is exact, bw * (+-1) is exact, so the gradient is ONE rounded division:      |g - G| <= u |G|   (no slack: this
    is what separates avg + eps from avg at avg = 1, a difference of 2u).
  A sum of n non-zero fp32 terms in any order (zeros add exactly): n u sum |terms|; the division by den and one u of slack: 2u |LOSS|.
                       |loss - LOSS| <= (sum term bounds + n u sum |TERM|) / den + 2u |LOSS| + n TINY
  Softmax row over the n unmasked classes, z_c = x_c - m, Z = max |z_c|:  fl(x - m): u |z|, which expf turns into a relative u |z|, plus
    its own 2u; the sum of n positive terms: (n - 1) u.   relative error of s: rs = (Z + 2 + n) u
    logf(s): rs + 2u |log s|;  fl(z_y): u |z_y|;  the subtraction: u |z_y - log s|;  times cw_y, times lw: 2u.
                       |term_r - TERM_r| <= |lw| cw_y (u |z_y| + rs + 2u |log s| + u |z_y - log s|) + 3u |TERM_r|
    p_c = e_c / s: rp = (|z_c| + 2) u + rs + u.  coef = fl(fl(lw cw_y) / den): 2u.
                       |g - G| <= |coef| (P rp + u |P - [c == y]|) + 3u |G|
  acc = fl(fl(100 hits) / R) is the same fp32 expression on both sides: equal bits.  out[3] (avg) is an integer or the caller's value: equal.
The not-vacuous test plants four errors in (b) and requires these bounds to reject each.

CASES are generated from seeds; nothing is read from outside the repository.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 2.0 ** -23
TINY = 2.0 ** -100
F32 = np.float32


def same_float_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def den_f32(avg):
    return float(F32(avg) + F32(EPS))


def level_sizes(side, strides=(4, 8, 16, 32, 64)):
    """(h, w) of the five levels of a side x side image: ceil(side / stride)."""
    return [(-(-side // s), -(-side // s)) for s in strides]


# ================================================================================================ cases
def rpn_case(name):
    """-> dict(levels [(h, w)], A, B, N, cls [L arrays B,A,h,w], reg [L arrays B,4A,h,w], labels, lw [B,N], bt, bw [B,N,4], avg)."""
    spec = RPN_CASES[name]
    levels, A, B, kind = spec["levels"], spec["A"], spec["B"], spec["kind"]
    rng = np.random.default_rng(spec["seed"])
    N = sum(h * w * A for h, w in levels)
    labels = np.ones((B, N), np.int32)
    lw, bt, bw = np.zeros((B, N), F32), np.zeros((B, N, 4), F32), np.zeros((B, N, 4), F32)
    dy = kind == "dyadic"
    q = (lambda shape: (rng.integers(-16, 17, shape) / 8.0).astype(F32)) if dy else (lambda shape: rng.normal(0, 1, shape).astype(F32))
    cls = [np.zeros((B, A, h, w), F32) if dy else (rng.normal(0, 3, (B, A, h, w))).astype(F32) for h, w in levels]
    reg = [q((B, 4 * A, h, w)) for h, w in levels]
    if kind == "edges":                                        # one weighted anchor at the first and at the last index of each level
        off = 0
        for h, w in levels:
            n = h * w * A
            for b in range(B):
                for i, pos in ((off, True), (off + n - 1, False)):
                    lw[b, i] = 1
                    labels[b, i] = 0 if pos else 1
                    if pos:
                        bw[b, i] = 1
                        bt[b, i] = q((4,))
            off += n
    elif kind != "zero":
        for b in range(B):
            pick = rng.choice(N, size=min(N, spec.get("sampled", 24)), replace=False)
            lw[b, pick] = 1 if not dy else rng.choice([1.0, 0.5], size=pick.size)
            posn = pick[: max(1, pick.size // 2)]
            labels[b, posn] = 0
            bw[b, posn] = 1 if not dy else rng.choice([1.0, 0.5], size=(posn.size, 1))
            bt[b, posn] = q((posn.size, 4))
    if dy:                                                     # some exact zeros of pred - target: sign(0) = 0
        off = 0
        for l, (h, w) in enumerate(levels):
            view = reg[l].reshape(B, A, 4, h, w)
            for b in range(B):
                for n in np.nonzero(bw[b, off:off + h * w * A, 0])[0][::2]:
                    p, a = divmod(int(n), A)
                    view[b, a, :2, p // w, p % w] = bt[b, off + n, :2]
            off += h * w * A
    if kind == "big":                                          # |x| up to 1e4: no overflow in exp, and lw * bce stays finite
        for c in cls:
            c *= F32(1e4 / 9.0)
            np.clip(c, -1e4, 1e4, out=c)
    if kind == "nonfinite":                                    # NaN / inf predictions wherever the weight is zero
        off = 0
        for l, (h, w) in enumerate(levels):
            n = h * w * A
            z = (lw[:, off:off + n] == 0).reshape(B, h, w, A).transpose(0, 3, 1, 2)
            bad = rng.choice([np.nan, np.inf, -np.inf], size=z.shape).astype(F32)
            cls[l] = np.where(z, bad, cls[l])
            zb = (bw[:, off:off + n] == 0).reshape(B, h, w, 4 * A).transpose(0, 3, 1, 2)
            reg[l] = np.where(zb, np.resize(bad, zb.shape), reg[l])
            bt[:, off:off + n] = np.where(bw[:, off:off + n] == 0, F32(np.nan), bt[:, off:off + n])
            off += n
    if kind == "hostile":                                      # weighted anchors whose labels are outside {0, 1}: they count as weight 0
        for b in range(B):
            on = np.nonzero(lw[b])[0]
            labels[b, on[::3]] = rng.choice([-1, 2, -100, 2 ** 31 - 1, -2 ** 31], size=on[::3].size)
    avg = spec.get("avg", float(max(int((lw > 0).sum()), 1)))
    return dict(levels=levels, A=A, B=B, N=N, cls=cls, reg=reg, labels=labels, lw=lw, bt=bt, bw=bw, avg=float(avg), kind=kind)


FIVE = level_sizes(64)                                         # 16, 8, 4, 2, 1: N = 3 * 341 = 1023 for A = 3
RPN_CASES = {
    "five_A3_B3": dict(levels=FIVE, A=3, B=3, kind="random", seed=1),
    "five_A1_B1": dict(levels=FIVE, A=1, B=1, kind="random", seed=2),
    "one_5x7_A3_B1": dict(levels=[(5, 7)], A=3, B=1, kind="random", seed=3),
    "one_5x7_A1_B3": dict(levels=[(5, 7)], A=1, B=3, kind="random", seed=4),
    "zero": dict(levels=FIVE, A=3, B=1, kind="zero", seed=5),
    "edges": dict(levels=FIVE, A=3, B=3, kind="edges", seed=6),
    "big": dict(levels=FIVE, A=3, B=1, kind="big", seed=7, sampled=200),
    "nonfinite": dict(levels=FIVE, A=3, B=3, kind="nonfinite", seed=8),
    "hostile": dict(levels=[(5, 7), (3, 4)], A=3, B=3, kind="hostile", seed=9),
    "dyadic": dict(levels=FIVE, A=3, B=3, kind="dyadic", seed=10, avg=64.0),
    "dyadic_5x7": dict(levels=[(5, 7)], A=3, B=1, kind="dyadic", seed=11, avg=1.0),
}
RPN_PLAIN = ["five_A3_B3", "five_A1_B1", "one_5x7_A3_B1", "one_5x7_A1_B3", "edges", "big", "dyadic", "dyadic_5x7"]      # no departure applies
RPN_EXACT = ["dyadic", "dyadic_5x7"]


def head_case(name):
    """-> dict(R, C1, pad, x [R, C1 + pad] (columns past C1 are padding), labels, lw [R], cw [C1] or None, bp, bt, bw [R, 4], bg, avg)."""
    spec = HEAD_CASES[name]
    R, C1, kind, pad = spec["R"], spec["C1"], spec["kind"], spec.get("pad", 0)
    rng = np.random.default_rng(spec["seed"])
    bg = C1 - 1
    uni = kind == "uniform"
    x = np.zeros((R, C1), F32) if uni else rng.normal(0, 3, (R, C1)).astype(F32)
    q = (lambda shape: (rng.integers(-16, 17, shape) / 8.0).astype(F32)) if uni else (lambda shape: rng.normal(0, 1, shape).astype(F32))
    labels = np.full(R, bg, np.int32)
    npos = 0 if kind == "nopos" or C1 == 1 else (R + 3) // 4
    labels[:npos] = rng.integers(0, max(bg, 1), npos)
    lw = np.ones(R, F32)
    lw[R - R // 8:] = 0                                        # padding slots of the sampler
    if uni:
        lw[::2] = 0.5
    bp, bt = q((R, 4)), q((R, 4))
    bw = np.zeros((R, 4), F32)
    bw[:npos] = 1
    if uni:
        bt[:npos:2, :2] = bp[:npos:2, :2]                      # exact zeros of pred - target
    cw = None
    if kind in ("masked", "departures") or spec.get("cw"):
        cw = np.ones(C1, F32)
        if C1 > 2:
            cw[rng.choice(C1 - 1, size=max(1, (C1 - 1) // 3), replace=False)] = 0
        cw[-1] = F32(0.9)
        live = np.nonzero(cw[:bg] >= 1e-5)[0] if bg else np.array([0])
        labels[:npos] = rng.choice(live, npos) if live.size else bg
        big = np.nonzero(cw < 1e-5)[0]
        x[:, big] += 50                                        # a masked class holds every row's largest logit: it must not win
    if kind == "departures" and R >= 8:
        labels[0], labels[1], labels[2], labels[3] = -100, C1, -1, 2 ** 31 - 1
        masked = np.nonzero(cw < 1e-5)[0]
        if masked.size:
            labels[4] = masked[0]                              # a row whose own label is masked
        x[R - 1, :] = np.nan                                   # a zero-weight row with non-finite logits
        bp[R - 1, :] = np.inf
    if kind == "ties":
        x = np.round(x)                                        # many tied maxima
        x[0, :] = 1.0
    xp = np.full((R, C1 + pad), F32(777.0), F32)
    xp[:, :C1] = x
    return dict(R=R, C1=C1, pad=pad, x=xp, labels=labels, lw=lw, cw=cw, bp=bp, bt=bt, bw=bw, bg=bg, avg=spec.get("avg"), kind=kind)


HEAD_CASES = {}
for _i, _c in enumerate((1, 2, 63, 64, 65, 66, 81, 257, 1204, 4096)):
    HEAD_CASES[f"C{_c}"] = dict(R=9, C1=_c, kind="random", seed=100 + _i)
for _i, _r in enumerate((0, 1, 63, 64, 65, 513)):
    HEAD_CASES[f"R{_r}"] = dict(R=_r, C1=66, kind="random", seed=200 + _i)
HEAD_CASES.update({
    "padded": dict(R=65, C1=66, pad=6, kind="random", seed=300),
    "padded_masked": dict(R=65, C1=81, pad=3, kind="masked", seed=301),
    "masked_1204": dict(R=33, C1=1204, kind="masked", seed=302),
    "departures": dict(R=65, C1=66, kind="departures", seed=303),
    "avg_given": dict(R=65, C1=66, kind="random", seed=304, avg=37.0),
    "avg_given_masked": dict(R=64, C1=66, kind="masked", seed=305, avg=512.0),
    "nopos": dict(R=65, C1=66, kind="nopos", seed=306),
    "ties": dict(R=65, C1=66, kind="ties", seed=307),
    "uniform": dict(R=64, C1=64, kind="uniform", seed=308, avg=32.0),
    "uniform_avg1": dict(R=16, C1=128, kind="uniform", seed=309, avg=1.0),
})
HEAD_PLAIN = [k for k, v in HEAD_CASES.items() if v["kind"] in ("random", "masked", "nopos") and v["R"] > 0]            # no departure applies
HEAD_EXACT = ["uniform", "uniform_avg1"]


# ================================================================================================ (b) closed form, float64
def _dense(t, B, h, w, C):
    """[B, n (* 4)] targets of one level in the predictions' layout [B, C, h, w]."""
    return t.reshape(B, h, w, C).transpose(0, 3, 1, 2)


def _sum_bound(terms, tb, den, loss):
    n = int(np.count_nonzero(terms))
    return (tb.sum() + n * U * np.abs(terms).sum()) / den + 2 * U * abs(loss) + (n + 1) * TINY


def rpn_ref(c, den_exact=False, plant=None):
    """-> dict(losses [L, 2], dcls, dreg (lists) and losses_bound, dcls_bound, dreg_bound), float64.
    plant: 'shift_anchor' reads anchor (x, a) as (x, a + 1) in one cell; 'sign0' takes sign(0) as 1; 'no_eps' leaves the eps out of den."""
    B, A = c["B"], c["A"]
    den = c["avg"] + EPS if den_exact else den_f32(c["avg"])
    if plant == "no_eps":
        den = float(c["avg"])
    out = dict(losses=[], losses_bound=[], dcls=[], dreg=[], dcls_bound=[], dreg_bound=[])
    off = 0
    for l, (h, w) in enumerate(c["levels"]):
        n = h * w * A
        lab, lw = c["labels"][:, off:off + n].astype(np.int64), c["lw"][:, off:off + n].astype(np.float64)
        if plant == "shift_anchor" and l == 0:
            hit = int(np.nonzero(lw[0])[0][0])                 # the first weighted anchor of image 0 moves to the next base anchor
            lab, lw = lab.copy(), lw.copy()
            lab[0, [hit, hit + 1]], lw[0, [hit, hit + 1]] = lab[0, [hit + 1, hit]], lw[0, [hit + 1, hit]]
        lab, lw = _dense(lab, B, h, w, A), _dense(lw, B, h, w, A)
        bt = _dense(c["bt"][:, off:off + n].astype(np.float64), B, h, w, 4 * A)
        bw = _dense(c["bw"][:, off:off + n].astype(np.float64), B, h, w, 4 * A)
        off += n
        on = (lw != 0) & ((lab == 0) | (lab == 1))
        with np.errstate(all="ignore"):
            x = np.where(on, c["cls"][l].astype(np.float64), 0.0)
            t = (lab == 0).astype(np.float64)
            e = np.exp(-np.abs(x))
            terms = np.where(on, lw * ((np.maximum(x, 0) - x * t) + np.log1p(e)), 0.0)
            sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
            g = np.where(on, lw * (sig - t) / den, 0.0)
            gb = np.where(on, np.abs(lw) / den * (6 * U * sig + U * np.abs(sig - t)), 0.0) + 3 * U * np.abs(g) + TINY
            lc = terms.sum() / den
            lcb = _sum_bound(terms, 7 * U * np.abs(terms), den, lc)
            bon = bw != 0
            d = np.where(bon, c["reg"][l].astype(np.float64), 0.0) - np.where(bon, bt, 0.0)
            bterms = np.where(bon, bw * np.abs(d), 0.0)
            sg = np.sign(d) if plant != "sign0" else np.where(d >= 0, 1.0, -1.0)
            gr = np.where(bon, bw * sg / den, 0.0)
            lb = bterms.sum() / den
            lbb = _sum_bound(bterms, 3 * U * np.abs(bterms), den, lb)
        out["losses"].append([lc, lb])
        out["losses_bound"].append([lcb, lbb])
        out["dcls"].append(g)
        out["dcls_bound"].append(gb)
        out["dreg"].append(gr)
        out["dreg_bound"].append(U * np.abs(gr) + TINY)
    out["losses"], out["losses_bound"] = np.array(out["losses"]), np.array(out["losses_bound"])
    return out


def head_ref(c, den_exact=False, plant=None):
    """-> dict(out [4], dcls [R, C1], dbbox [R, 4] and out_bound [4], dcls_bound, dbbox_bound), float64.
    plant: 'drop_class' leaves one class out of one row's softmax denominator; 'sign0'; 'no_eps'."""
    R, C1, bg = c["R"], c["C1"], c["bg"]
    x = c["x"][:, :C1].astype(np.float64)
    lw, y = c["lw"].astype(np.float64), c["labels"].astype(np.int64)
    cw = np.ones(C1) if c["cw"] is None else c["cw"].astype(np.float64)
    live = ~((np.ones(C1, F32) if c["cw"] is None else c["cw"]) < F32(1e-5))
    avg = float(c["avg"]) if c["avg"] is not None else float(max(int((c["lw"] > 0).sum()), 1))
    den = avg + EPS if den_exact else den_f32(avg)
    rden = R + EPS if den_exact else den_f32(R)
    if plant == "no_eps":
        den, rden = avg, float(R)
    dcls, dclsb = np.zeros((R, C1)), np.full((R, C1), TINY)
    terms, tb = np.zeros(R), np.zeros(R)
    hits = 0
    first_valid = True
    for r in range(R):
        xs = np.where(live & ~np.isnan(x[r]), x[r], -np.inf)
        arg = int(np.argmax(xs)) if np.any(live & ~np.isnan(x[r])) else -1          # numpy's argmax: the lowest index of the maximum
        y_in = 0 <= y[r] < C1
        hits += int(y_in and arg == y[r])
        if not (lw[r] != 0 and y_in and live[y[r]]):
            continue
        with np.errstate(all="ignore"):
            m = xs.max()
            z = np.where(live, x[r] - m, 0.0)
            e = np.where(live, np.exp(z), 0.0)
            s = e.sum()
            if plant == "drop_class" and first_valid:
                s -= e[[k for k in np.nonzero(live)[0] if k != y[r]][0]]
                first_valid = False
            n, Z = int(live.sum()), float(np.abs(z[live]).max())
            rs = (Z + 2 + n) * U
            ly = z[y[r]] - np.log(s)
            terms[r] = lw[r] * (-cw[y[r]] * ly)
            tb[r] = abs(lw[r]) * cw[y[r]] * (U * abs(z[y[r]]) + rs + 2 * U * abs(np.log(s)) + U * abs(ly)) + 3 * U * abs(terms[r])
            coef = lw[r] * cw[y[r]] / den
            p = e / s
            onehot = (np.arange(C1) == y[r]).astype(np.float64)
            dcls[r] = np.where(live, coef * (p - onehot), 0.0)
            rp = (np.abs(z) + 2) * U + rs + U
            dclsb[r] = np.where(live, abs(coef) * (p * rp + U * np.abs(p - onehot)) + 3 * U * np.abs(dcls[r]), 0.0) + TINY
    loss_cls = terms.sum() / den
    pos = (y >= 0) & (y < bg)
    bon = pos[:, None] & (c["bw"] != 0)
    with np.errstate(all="ignore"):
        d = np.where(bon, c["bp"].astype(np.float64), 0.0) - np.where(bon, c["bt"].astype(np.float64), 0.0)
        bterms = np.where(bon, c["bw"].astype(np.float64) * np.abs(d), 0.0)
        sg = np.sign(d) if plant != "sign0" else np.where(d >= 0, 1.0, -1.0)
        dbbox = np.where(bon, c["bw"].astype(np.float64) * sg / rden, 0.0)
    loss_bbox = bterms.sum() / rden
    acc = float(F32(F32(100) * F32(hits)) / F32(R)) if R else 0.0
    out = np.array([loss_cls, acc, loss_bbox, avg])
    ob = np.array([_sum_bound(terms, tb, den, loss_cls), 0.0, _sum_bound(bterms, 3 * U * np.abs(bterms), rden, loss_bbox), 0.0])
    return dict(out=out, out_bound=ob, dcls=dcls, dcls_bound=dclsb, dbbox=dbbox, dbbox_bound=U * np.abs(dbbox) + TINY)


def inside(got, want, bound):
    """Element by element |got - want| <= bound, NaN-free; -> (ok, worst fraction of the bound)."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    if got.shape != want.shape or not np.all(np.isfinite(got)):
        return False, float("inf")
    if got.size == 0:
        return True, 0.0
    diff = np.abs(got - want)
    frac = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))       # a zero bound asks for equality
    return bool(np.all(frac <= 1.0)), float(frac.max())


# ================================================================================================ (a) mmdet 2.28.1 as read, torch float64
def _weight_reduce_loss(loss, weight, avg_factor):
    """mmdet 2.28.1 weight_reduce_loss, reduction='mean' with an avg_factor."""
    if weight is not None:
        loss = loss * weight
    eps = torch.finfo(torch.float32).eps
    return loss.sum() / (avg_factor + eps)


def _expand_onehot_labels(labels, label_weights, label_channels, ignore_index):
    bin_labels = labels.new_full((labels.size(0), label_channels), 0)
    valid_mask = (labels >= 0) & (labels != ignore_index)
    inds = torch.nonzero(valid_mask & (labels < label_channels), as_tuple=False)
    if inds.numel() > 0:
        bin_labels[inds, labels[inds]] = 1
    valid_mask = valid_mask.view(-1, 1).expand(labels.size(0), label_channels).float()
    bin_label_weights = valid_mask if label_weights is None else label_weights.view(-1, 1).repeat(1, label_channels) * valid_mask
    return bin_labels, bin_label_weights, valid_mask


def rpn_mmdet(c, dtype=torch.float64):
    """RPNHead.loss -> (losses [L, 2], dcls list, dreg list): loss_single per level, gradients of the sum by autograd."""
    B, A = c["B"], c["A"]
    cls = [torch.tensor(v, dtype=dtype, requires_grad=True) for v in c["cls"]]
    reg = [torch.tensor(v, dtype=dtype, requires_grad=True) for v in c["reg"]]
    losses, off = [], 0
    for l, (h, w) in enumerate(c["levels"]):
        n = h * w * A
        labels = torch.tensor(c["labels"][:, off:off + n].astype(np.int64)).reshape(-1)
        label_weights = torch.tensor(c["lw"][:, off:off + n], dtype=dtype).reshape(-1)
        bbox_targets = torch.tensor(c["bt"][:, off:off + n], dtype=dtype).reshape(-1, 4)
        bbox_weights = torch.tensor(c["bw"][:, off:off + n], dtype=dtype).reshape(-1, 4)
        off += n
        cls_score = cls[l].permute(0, 2, 3, 1).reshape(-1, 1)
        bin_labels, weight, _ = _expand_onehot_labels(labels, label_weights.float(), 1, -100)
        loss = F.binary_cross_entropy_with_logits(cls_score, bin_labels.to(dtype), reduction="none")
        loss_cls = _weight_reduce_loss(loss, weight.to(dtype), c["avg"])
        bbox_pred = reg[l].permute(0, 2, 3, 1).reshape(-1, 4)
        loss_bbox = _weight_reduce_loss(torch.abs(bbox_pred - bbox_targets), bbox_weights, c["avg"])
        losses.append(torch.stack([loss_cls, loss_bbox]))
    losses = torch.stack(losses)
    losses.sum().backward()
    return losses.detach().numpy(), [t.grad.numpy() for t in cls], [t.grad.numpy() for t in reg]


def head_mmdet(c, dtype=torch.float64):
    """BBoxHead.loss (reg_class_agnostic) with the reference's cross_entropy -> (out [4], dcls, dbbox)."""
    R, C1, bg = c["R"], c["C1"], c["bg"]
    cls_score = torch.tensor(c["x"][:, :C1], dtype=dtype, requires_grad=True)
    bbox_pred = torch.tensor(c["bp"], dtype=dtype, requires_grad=True)
    labels = torch.tensor(c["labels"].astype(np.int64))
    label_weights = torch.tensor(c["lw"], dtype=dtype)
    bbox_targets, bbox_weights = torch.tensor(c["bt"], dtype=dtype), torch.tensor(c["bw"], dtype=dtype)
    avg_factor = max(torch.sum(label_weights > 0).float().item(), 1.) if c["avg"] is None else c["avg"]
    pred = cls_score.clone()
    class_weight = None
    if c["cw"] is not None:
        class_weight = torch.tensor(c["cw"], dtype=dtype)
        mask_out = torch.tensor(c["cw"]) < 0.00001
        pred[:, mask_out] = -float("inf")                      # the reference writes into its argument; here into the clone
    loss = F.cross_entropy(pred, labels, weight=class_weight, reduction="none", ignore_index=-100)
    loss_cls = _weight_reduce_loss(loss, label_weights, avg_factor)
    _, pred_label = pred.detach().topk(1, dim=1)
    acc = pred_label.t().eq(labels.view(1, -1)).reshape(-1).float().sum() * (100.0 / R)
    pos_inds = (labels >= 0) & (labels < bg)
    if pos_inds.any():
        loss_bbox = _weight_reduce_loss(torch.abs(bbox_pred[pos_inds] - bbox_targets[pos_inds]), bbox_weights[pos_inds], bbox_targets.size(0))
    else:
        loss_bbox = bbox_pred[pos_inds].sum()
    (loss_cls + loss_bbox).backward()
    out = np.array([loss_cls.item(), acc.item(), loss_bbox.item(), float(avg_factor)])
    return out, cls_score.grad.numpy(), bbox_pred.grad.numpy()
