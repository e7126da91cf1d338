"""TEST INFRASTRUCTURE -- batch norm (+ ReLU) on channel-last maps (clipself_amd/norm_act.py, include/clipself_bn.h).

* `RefOpsBN`: tests/_conv_ref.RefOpsConv plus the six batch-norm ops as torch expressions written from the header, and the BATCHNORM flag
  -- the CPU backend BatchNormAct2d's kernel route and its autograd function run on without a GPU.  `flaws` plants one error in a copy
  (what the checks must reject).
* `PartsBN`: BatchNormAct2d as rank r of R ranks without processes -- the other ranks' records and sums come from the same ops on their
  rows, through the two methods the layer reaches its collective by.
* Seeded operands: random (representable in the map's type) and exact (known answers, see `exact_case`).
* The reference: F.batch_norm(training=...) followed by F.relu under autograd in float64 -- torch's own layer, which the reference's
  SyncBN is; the multi-rank reference is the same call on the concatenation of all parts.
* The bounds, derived per element from named rounding terms, u = 2^-24, first order with a factor 2 on every accumulation for the
  higher orders (Higham, Accuracy and Stability of Numerical Algorithms, §3.1), as tests/_neck_ref.bound:

  input rounding   none: the operands are generated representable in the map's type (bf16 or fp32), and bf16 -> fp32 is exact.
  reduction        a sum of n fp32 terms in ANY order errs by at most (n - 1) u sum|terms|; the two levels (thread -> workgroup tree,
                   partials -> slices -> tree) are one such order.  `2 (n + 1) u sum|terms|` with n the part's rows covers both levels,
                   the rounding of each term (d = x - K, fmaf(d, d, .)) and the higher orders.
  statistics       a part's record is  mean = K + s1 / n,  M2 = s2 - s1 (s1 / n)  with the shifted sums s1 = sum d, s2 = sum d^2,
                   d = x - K, K = the part's first row:
                     e(s1)   = 2 (n + 1) u sum|d|
                     e(mean) = e(s1) / n + 2 u (sum|d| / n + |mean|)                      (the division and the final addition)
                     e(M2)   = 2 (n + 1) u sum d^2 + 2 (|s1| / n) e(s1) + 2 u s1^2 / n + u M2
                   The terms scale with sum d^2 = M2 + n (mean - K)^2, not with sum x^2: a map with mean 1000 and unit variance keeps
                   its variance to ~n u relative, where E[x^2] - E[x]^2 in fp32 errs by ~u mean^2 = 0.06 absolute (6 at mean 10 000).
  merge            R records merged by Chan's formula: mean = sum n_r mean_r / N and M2 = sum M2_r + sum n_r (mean_r - mean)^2 in exact
                   arithmetic; the means' errors enter the between-part term with 2 n_r |mean_r - mean| (e(mean_r) + e(mean)), and each
                   of the R - 1 merges rounds its few operations: 4 (R - 1) u on the quantities merged.
  rstd             var = M2 / N (+ u var); rstd = 1 / sqrt(var + eps): |d rstd / d var| = rstd^3 / 2, and the addition, the square root
                   and the division round once each: e(rstd) = rstd^3 e(var) / 2 + 3 u rstd.
  fmaf             scale = gamma rstd (+ u), shift = fmaf(-mean, scale, beta) (+ u), y = fmaf(x, scale, shift) (+ u |y|):
                     e(y) = |x| e(scale) + e(shift) + u |y|;  the ReLU is 1-Lipschitz and adds nothing.
  output rounding  a bf16 result adds half an ulp: 2^-8 (|reference| + bound).
  mask             where |fmaf(x, scale, shift)| <= e(y) the kernels' ReLU mask may differ from the reference's: such an element adds
                   |dy| to its own g and to the sums it enters.
  backward         xhat = (x - mean) rstd:  e(xhat) = (e(mean) + u |x - mean|) rstd + |x - mean| e(rstd) + u |xhat|;
                   sum g: 2 (n + R) u sum|g| + the mask term; sum g xhat: 2 (n + R + 1) u sum|g xhat| + sum|g| e(xhat) + the mask term;
                   dx = a (g - b - xhat c), a = gamma rstd, b = sum g / N, c = sum g xhat / N:
                     e(dx) = |a| (mask + e(b) + |c| e(xhat) + |xhat| e(c) + 2 u (|g| + |b| + |xhat c|)) + |g - b - xhat c| e(a) + u |dx|.
  Derived, not measured."""
import functools

import torch
import torch.nn.functional as F

from _conv_ref import RefOpsConv
from _neck_ref import BF, F32, F64, check_bound, rne_bf16  # noqa: F401

U = 2.0 ** -24
REC_EXTRA, ST_EXTRA = 4, 4
# (M, C) of the issue: the smallest | a partial thread row | one channel group of bf16 | odd rows, six groups | just past a power of two |
# the heads' width | 1089 = 33 * 33 rows, nine / eighteen groups (no power of two) | several workgroups with a remainder block, the neck's width
SHAPES = [(2, 8), (30, 16), (64, 8), (147, 48), (257, 64), (512, 256), (1089, 72), (5000, 768)]
SHAPE_IDS = [f"{m}x{c}" for m, c in SHAPES]
EXACT_SHAPES = [(2, 8), (64, 8), (128, 16), (512, 256)]                     # M a power of two
EXACT_IDS = [f"{m}x{c}" for m, c in EXACT_SHAPES]
EPS, MOMENTUM = 1e-5, 0.1
FLAWS = ("naive_var", "unbiased_norm", "biased_running", "mean_of_means", "no_mask", "no_xhat_term")


def fmaf(a, b, c):
    """fmaf of fp32 tensors: the product is exact in float64, one rounding to fp32 (a double rounding is possible and immaterial here)."""
    return (a.double() * b.double() + c.double()).to(F32)


# ------------------------------------------------------------------------------------------------ the ops, from the header's definition
class RefOpsBN(RefOpsConv):
    name = "ref+taps+neck+conv+bn"
    BATCHNORM = True
    flaws = ()

    def bn_workspace(self, M, C):
        return 2 * C * 4

    @staticmethod
    def _map(t):
        assert t.dim() == 2 and t.dtype in (F32, BF) and t.shape[1] % 8 == 0 and t.shape[0] >= 1, (t.dtype, tuple(t.shape))
        return t.shape

    def bn_stats(self, x, rec, ws=None):
        M, C = self._map(x)
        assert rec.dtype == F32 and rec.numel() == 2 * C + REC_EXTRA
        xf = x.to(F32)
        if "naive_var" in self.flaws:                                   # E[x^2] - E[x]^2 in fp32
            import numpy as np
            a = xf.numpy().astype(np.float32)
            mean = a.mean(0, dtype=np.float32)
            var = (a * a).mean(0, dtype=np.float32) - mean * mean
            mean, M2 = torch.from_numpy(mean), torch.from_numpy(np.maximum(var, 0) * np.float32(M))
        else:
            K = xf[0]
            d = xf - K
            s1, s2 = d.sum(0), (d * d).sum(0)
            q = s1 / float(M)
            mean, M2 = K + q, (s2 - s1 * q).clamp_min(0)
        rec[:C] = mean
        rec[C:2 * C] = M2
        rec[2 * C:] = 0
        rec[2 * C:2 * C + 1].view(torch.int32)[0] = M

    def bn_finalize(self, recs, C, gamma, beta, eps, momentum, running_mean, running_var, st):
        assert st.dtype == F32 and st.numel() == 4 * C + ST_EXTRA and C % 8 == 0
        if recs is not None:
            recs = recs.view(-1, 2 * C + REC_EXTRA)
            N, mean, M2 = 0, torch.zeros(C), torch.zeros(C)
            for rec in recs:
                cnt = int(rec[2 * C:2 * C + 1].view(torch.int32)[0])
                if cnt <= 0:
                    continue
                mb, M2b = rec[:C].clone(), rec[C:2 * C].clone()
                if N == 0:
                    mean, M2 = mb, M2b
                elif "mean_of_means" in self.flaws:                     # parts averaged without their counts
                    mean, M2 = (mean + mb) / 2, M2 + M2b
                else:
                    na, nb = torch.tensor(float(N)), torch.tensor(float(cnt))
                    w, d = nb / torch.tensor(float(N + cnt)), mb - mean
                    mean = mean + d * w
                    M2 = (M2 + M2b) + d * d * (na * w)
                N += cnt
            var = M2 / float(N)
            inv_n = 1.0 / float(N)
            unbiased = M2 / float(N - 1) if N > 1 else None
            if "biased_running" in self.flaws:
                unbiased = var
            if running_mean is not None:
                running_mean.copy_((1.0 - momentum) * running_mean + momentum * mean)
            if running_var is not None and unbiased is not None:
                running_var.copy_((1.0 - momentum) * running_var + momentum * unbiased)
            if "unbiased_norm" in self.flaws and N > 1:
                var = M2 / float(N - 1)
        else:
            assert running_mean is not None and running_var is not None
            mean, var, inv_n = running_mean.clone(), running_var.clone(), 0.0
        rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
        scale = gamma * rstd if gamma is not None else rstd
        shift = fmaf(-mean, scale, beta if beta is not None else torch.zeros(C))
        st[:C], st[C:2 * C], st[2 * C:3 * C], st[3 * C:4 * C] = mean, rstd, scale, shift
        st[4 * C:] = 0
        st[4 * C] = inv_n

    @staticmethod
    def _st(st, C):
        return st[:C], st[C:2 * C], st[2 * C:3 * C], st[3 * C:4 * C], float(st[4 * C])

    def bn_apply(self, x, st, act, y):
        M, C = self._map(x)
        assert tuple(y.shape) == (M, C) and y.dtype in (F32, BF) and act in (0, 1)
        _, _, scale, shift, _ = self._st(st, C)
        v = fmaf(x.to(F32), scale, shift)
        if act:
            v = torch.where((v > 0) | v.isnan(), v, torch.zeros(()))
        y.copy_(v.to(y.dtype))

    def _g_xhat(self, dy, x, st, act):
        M, C = self._map(x)
        assert tuple(dy.shape) == (M, C) and dy.dtype in (F32, BF) and act in (0, 1)
        mean, rstd, scale, shift, inv_n = self._st(st, C)
        xf, g = x.to(F32), dy.to(F32)
        if act and "no_mask" not in self.flaws:
            g = torch.where(fmaf(xf, scale, shift) > 0, g, torch.zeros(()))
        return g, (xf - mean) * rstd, rstd, inv_n

    def bn_bwd_reduce(self, dy, x, st, act, sums, ws=None):
        C = x.shape[1]
        assert sums.dtype == F32 and sums.numel() == 2 * C
        g, xh, _, _ = self._g_xhat(dy, x, st, act)
        sums[:C] = g.sum(0)
        sums[C:] = (g * xh).sum(0)

    def bn_bwd_apply(self, dy, x, st, act, sums, gamma, dx):
        M, C = self._map(x)
        assert tuple(dx.shape) == (M, C) and dx.dtype in (F32, BF)
        g, xh, rstd, inv_n = self._g_xhat(dy, x, st, act)
        a = gamma * rstd if gamma is not None else rstd
        if inv_n != 0.0:
            b, c = sums[:C] * inv_n, sums[C:] * inv_n
            t = g - b
            if "no_xhat_term" not in self.flaws:
                t = fmaf(-xh, c.expand_as(xh), t)
        else:
            t = g
        dx.copy_((a * t).to(dx.dtype))


def flawed(*flaws):
    ops = RefOpsBN()
    ops.flaws = tuple(flaws)
    return ops


# ------------------------------------------------------------------------------------------------ ranks without processes
def make_parts_bn():
    from clipself_amd.norm_act import BatchNormAct2d

    class PartsBN(BatchNormAct2d):
        """Rank `rank` of len(xs) ranks: xs / dys are every rank's input and output-gradient rows [n_r, C] on the ops' device."""

        def set_parts(self, xs, dys, rank):
            self.xs, self.dys, self.rank = xs, dys, rank

        def forward(self, x):
            self._k = self.kernel_backend(x)
            return super().forward(x)

        def _world(self):
            return len(self.xs) if self.training else 1

        def _gather_records(self, rec):
            C, k = self.num_features, self._k
            recs = []
            for r, x in enumerate(self.xs):
                if r == self.rank:
                    recs.append(rec)
                else:
                    other = k.empty((2 * C + REC_EXTRA,), F32)
                    k.bn_stats(x, other)
                    recs.append(other)
            self._recs = torch.stack(recs)
            return self._recs

        def _reduce_sums(self, sums):
            C, k = self.num_features, self._k
            st = k.empty((4 * C + ST_EXTRA,), F32)
            w = None if self.weight is None else self.weight.detach()
            b = None if self.bias is None else self.bias.detach()
            k.bn_finalize(self._recs, C, w, b, self.eps, 0.0, None, None, st)
            total = None
            for r, (x, dy) in enumerate(zip(self.xs, self.dys)):
                if r == self.rank:
                    s = sums.clone()
                else:
                    s = k.empty((2 * C,), F32)
                    k.bn_bwd_reduce(dy, x, st, 1 if self.act == "relu" else 0, s)
                total = s if total is None else total + s
            sums.copy_(total)                                            # in place, as all_reduce
            return sums
    return PartsBN


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_operands(M, C, dtype, seed):
    """x, dy [M, C] fp32 values representable in `dtype`, gamma, beta fp32 [C]; channel means in [-2, 2], spreads in [0.5, 2]."""
    g = _gen(seed)
    mu, sd = torch.rand(C, generator=g) * 4 - 2, torch.rand(C, generator=g) * 1.5 + 0.5
    x = (torch.randn(M, C, generator=g) * sd + mu).to(dtype).to(F32)
    dy = torch.randn(M, C, generator=g).to(dtype).to(F32)
    return x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5, dy


def offset_operands(M, C, seed=3):
    """An fp32 map with unit variance whose channel means are 1000 (even channels) and 10 000 (odd channels)."""
    g = _gen(seed)
    mu = torch.where(torch.arange(C) % 2 == 0, torch.tensor(1000.0), torch.tensor(10000.0))
    return (torch.randn(M, C, generator=g).double() + mu.double()).to(F32)


def exact_case(M, C, seed=0, splits=None):
    """Known answers.  Channel c holds +2^k and -2^k (k = k_c in -2..2) equally often -- in every part of `splits` rows, where given --
    gamma = 2^j (j in 0..3), beta an integer in [-2, 2], dy integers in [-4, 4], eps = 0.  Then mean = 0, M2 = M 4^k, rstd = 2^-k,
    scale = 2^(j-k), shift = beta, y = act(+-2^j + beta), and every sum and every dx is a dyadic number of a few bits: fp32 arithmetic in
    any order is exact (a part's shifted sums are s1 = -n K and s2 = 2 n K^2 with K = +-2^k, so s1 / n = -K exactly for any n)."""
    splits = [M] if splits is None else list(splits)
    assert sum(splits) == M and all(n % 2 == 0 for n in splits)
    g = _gen(seed + M + C)
    k = torch.randint(-2, 3, (C,), generator=g)
    j = torch.randint(0, 4, (C,), generator=g)
    sign = torch.ones(M, C)
    r0 = 0
    for n in splits:
        for c in range(C):
            sign[r0 + torch.randperm(n, generator=g)[:n // 2], c] = -1.0
        r0 += n
    x = sign * (2.0 ** k.float())
    gamma, beta = 2.0 ** j.float(), torch.randint(-2, 3, (C,), generator=g).float()
    dy = torch.randint(-4, 5, (M, C), generator=g).float()
    return x, gamma, beta, dy, k, j, sign


def exact_answers(M, C, act, seed=0, splits=None):
    """float64 answers of exact_case in closed form; sg / sgx are lists over the parts."""
    x, gamma, beta, dy, k, j, sign = exact_case(M, C, seed, splits)
    splits = [M] if splits is None else list(splits)
    s64, g64, b64 = sign.double(), gamma.double(), beta.double()
    rstd = 2.0 ** (-k.double())
    pre = s64 * g64 + b64
    mask = (pre > 0).double() if act else torch.ones_like(pre)
    g = dy.double() * mask
    sg, sgx = g.sum(0), (g * s64).sum(0)
    dx = g64 * rstd * (g - sg / M - s64 * sgx / M)
    edges = [0] + list(torch.tensor(splits).cumsum(0))
    parts = [slice(int(edges[r]), int(edges[r + 1])) for r in range(len(splits))]
    return dict(mean=torch.zeros(C, dtype=F64), M2=M * 4.0 ** k.double(), rstd=rstd, scale=g64 * rstd, shift=b64, inv_n=1.0 / M,
                y=pre * (pre > 0) if act else pre, dx=dx, sg=[g[p].sum(0) for p in parts], sgx=[(g * s64)[p].sum(0) for p in parts],
                unbiased=M * 4.0 ** k.double() / (M - 1), parts=parts)


# ------------------------------------------------------------------------------------------------ the reference and its bounds
def _part_record(x64):
    n = x64.shape[0]
    K = x64[0]
    d = x64 - K
    ad, s1, sd2 = d.abs().sum(0), d.sum(0), (d * d).sum(0)
    mu = x64.mean(0)
    M2 = ((x64 - mu) ** 2).sum(0)
    e_s1 = 2.0 * (n + 1) * U * ad
    e_mean = e_s1 / n + 2.0 * U * (ad / n + mu.abs())
    e_M2 = 2.0 * (n + 1) * U * sd2 + 2.0 * (s1.abs() / n) * e_s1 + 2.0 * U * s1 * s1 / n + U * M2
    return n, mu, M2, e_mean, e_M2


def reference(x, gamma, beta, dy, act, eps=EPS, splits=None, training=True, running=None, momentum=MOMENTUM, bf16_out=False):
    """The float64 reference of one training (or evaluation) step on the rows x [M, C] -- all parts concatenated; splits = the parts' row
    counts -- and the per-element bounds of everything the kernels produce.  -> (ref, tol): dicts over mean, M2, rstd, scale, shift, y,
    sg, sgx (lists per part), dx, dgamma, dbeta (lists per part), running_mean, running_var."""
    M, C = x.shape
    splits = [M] if splits is None else list(splits)
    R = len(splits)
    x64, dy64 = x.double(), dy.double()
    g64 = torch.ones(C, dtype=F64) if gamma is None else gamma.double()
    b64 = torch.zeros(C, dtype=F64) if beta is None else beta.double()
    xa, ga, ba = x64.clone().requires_grad_(True), g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    rm = None if running is None else running[0].double().clone()
    rv = None if running is None else running[1].double().clone()
    out = F.batch_norm(xa, rm, rv, ga, ba, training, momentum, eps)
    if act:
        out = F.relu(out)
    out.backward(dy64)
    ref = dict(y=out.detach(), dx=xa.grad, dgamma_total=ga.grad, dbeta_total=ba.grad, running_mean=rm, running_var=rv)

    bounds = [0] + list(torch.tensor(splits).cumsum(0))
    parts = [slice(int(bounds[r]), int(bounds[r + 1])) for r in range(R)]
    if training:
        recs = [_part_record(x64[p]) for p in parts]
        N = float(M)
        mu = sum(n * m for n, m, *_ in recs) / N
        between = sum(n * (m - mu) ** 2 for n, m, *_ in recs)
        M2 = sum(r[2] for r in recs) + between
        mergeU = 4.0 * (R - 1) * U
        e_mean = sum((n / N) * e for n, _, _, e, _ in recs) + mergeU * (torch.stack([r[1].abs() for r in recs]).max(0).values + mu.abs())
        e_M2 = sum(r[4] for r in recs) + sum(2.0 * n * (m - mu).abs() * (e + e_mean) for n, m, _, e, _ in recs) + mergeU * M2
        var = M2 / N
        e_var = e_M2 / N + U * var
        ref.update(M2=M2, unbiased=M2 / (N - 1) if M > 1 else None)
    else:
        mu, var = running[0].double(), running[1].double()
        e_mean, e_M2, e_var, N = torch.zeros(C, dtype=F64), None, torch.zeros(C, dtype=F64), float(M)
    rstd = (var + eps) ** -0.5
    e_rstd = 0.5 * rstd ** 3 * e_var + 3.0 * U * rstd
    scale = g64 * rstd
    e_scale = g64.abs() * e_rstd + U * scale.abs()
    shift = b64 - mu * scale
    e_shift = scale.abs() * e_mean + mu.abs() * e_scale + U * (shift.abs() + (mu * scale).abs())
    pre = x64 * scale + shift
    e_y = x64.abs() * e_scale + e_shift + U * pre.abs()
    ref.update(mean=mu, rstd=rstd, scale=scale, shift=shift)
    tol = dict(mean=e_mean, M2=e_M2, rstd=e_rstd, scale=e_scale, shift=e_shift)
    tol["y"] = e_y + 2.0 ** -8 * (ref["y"].abs() + e_y) if bf16_out else e_y

    flip = ((pre.abs() <= e_y) & bool(act)).double() * dy64.abs()                     # the mask term
    g = dy64 * ((pre > 0).double() if act else 1.0)
    xc = x64 - mu
    xh = xc * rstd
    e_xh = (e_mean + U * xc.abs()) * rstd + xc.abs() * e_rstd + U * xh.abs()
    ref["sg"], ref["sgx"], tol["sg"], tol["sgx"] = [], [], [], []
    for p in parts:
        n = p.stop - p.start
        ref["sg"].append(g[p].sum(0))
        ref["sgx"].append((g[p] * xh[p]).sum(0))
        tol["sg"].append(2.0 * (n + R) * U * g[p].abs().sum(0) + flip[p].sum(0))
        tol["sgx"].append(2.0 * (n + R + 1) * U * (g[p] * xh[p]).abs().sum(0) + (g[p].abs() * e_xh[p]).sum(0) + (flip[p] * xh[p].abs()).sum(0))
    ref["dbeta"], ref["dgamma"], tol["dbeta"], tol["dgamma"] = ref["sg"], ref["sgx"], tol["sg"], tol["sgx"]
    a, e_a = scale, e_scale
    if training:
        b, c = sum(ref["sg"]) / N, sum(ref["sgx"]) / N
        e_b = (sum(tol["sg"]) + 2.0 * R * U * g.abs().sum(0)) / N + 2.0 * U * b.abs()
        e_c = (sum(tol["sgx"]) + 2.0 * R * U * (g * xh).abs().sum(0)) / N + 2.0 * U * c.abs()
        t = g - b - xh * c
        e_t = flip + e_b + c.abs() * e_xh + xh.abs() * e_c + 2.0 * U * (g.abs() + b.abs() + (xh * c).abs())
    else:
        t, e_t = g, flip
    e_dx = a.abs() * e_t + t.abs() * e_a + U * ref["dx"].abs()
    tol["dx"] = e_dx + 2.0 ** -8 * (ref["dx"].abs() + e_dx) if bf16_out else e_dx
    if training and running is not None:
        tol["running_mean"] = momentum * e_mean + 3.0 * U * (running[0].double().abs() + mu.abs())
        tol["running_var"] = momentum * (e_M2 / max(N - 1, 1) + U * ref["unbiased"]) + 3.0 * U * (running[1].double().abs() + ref["unbiased"])
    ref["parts"] = parts
    return ref, tol


@functools.lru_cache(maxsize=None)
def case(shape, dtype, act, splits=None, seed=0):
    """(x, gamma, beta, dy, running, ref, tol) of a random case, computed once and shared (read-only) by the tests that need it."""
    M, C = shape
    x, gamma, beta, dy = random_operands(M, C, dtype, seed + M + C)
    g = _gen(seed + 7)
    running = (torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5)
    ref, tol = reference(x, gamma, beta, dy, act, splits=splits, running=running, bf16_out=dtype == BF)
    return x, gamma, beta, dy, running, ref, tol


def same_bits(got, want, what):
    it = {BF: torch.int16, F32: torch.int32}[got.dtype]
    assert want.dtype == got.dtype and tuple(want.shape) == tuple(got.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().contiguous().view(it), want.contiguous().view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


def image(t64, dtype):
    """The image of exactly fp32-representable float64 values in `dtype` (bf16: round to nearest even); -0 as +0."""
    return (t64 + 0.0).to(F32).to(dtype)


def run_ops(ops, x, gamma, beta, dy, act, dtype, splits=None, running=None, eps=EPS, momentum=MOMENTUM, dev="cpu", training=True, new=None):
    """The whole step through the six ops on rows, as the layer chains them, every part in turn.  -> dict(rec [R], st, y [R], sums [R],
    dx [R], running_mean, running_var).  `new(shape, dtype)` allocates an output (the GPU tests hand in NaN)."""
    M, C = x.shape
    new = new or (lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev))
    splits = [M] if splits is None else list(splits)
    edges = [0] + list(torch.tensor(splits).cumsum(0))
    xs = [x[int(edges[r]):int(edges[r + 1])].to(dtype).to(dev).contiguous() for r in range(len(splits))]
    dys = [dy[int(edges[r]):int(edges[r + 1])].to(dtype).to(dev).contiguous() for r in range(len(splits))]
    gm = None if gamma is None else gamma.to(dev)
    bt = None if beta is None else beta.to(dev)
    rm = None if running is None else running[0].clone().to(dev)
    rv = None if running is None else running[1].clone().to(dev)
    st = new((4 * C + ST_EXTRA,), F32)
    out = dict(rec=[], y=[], sums=[], dx=[])
    if training:
        for xr in xs:
            rec = new((2 * C + REC_EXTRA,), F32)
            ops.bn_stats(xr, rec)
            out["rec"].append(rec)
        ops.bn_finalize(torch.stack(out["rec"]), C, gm, bt, eps, momentum, rm, rv, st)
    else:
        ops.bn_finalize(None, C, gm, bt, eps, momentum, rm, rv, st)
    for xr, dyr in zip(xs, dys):
        y, sums = new(tuple(xr.shape), dtype), new((2 * C,), F32)
        ops.bn_apply(xr, st, act, y)
        ops.bn_bwd_reduce(dyr, xr, st, act, sums)
        out["y"].append(y)
        out["sums"].append(sums)
    total = torch.stack(out["sums"]).sum(0) if len(xs) > 1 else out["sums"][0]
    for xr, dyr in zip(xs, dys):
        dx = new(tuple(xr.shape), dtype)
        ops.bn_bwd_apply(dyr, xr, st, act, total, gm, dx)
        out["dx"].append(dx)
    out.update(st=st, running_mean=rm, running_var=rv)
    return out


def check_ops(tag, got, ref, tol, C, training=True, running=True):
    """Every quantity run_ops produced against the reference, inside its bound; prints worst error / bound per quantity."""
    st = got["st"].detach().cpu()
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        check_bound(f"{tag} {k}", st[i * C:(i + 1) * C], ref[k], tol[k])
    cat = lambda ts: torch.cat([t.detach().cpu().double() for t in ts])
    check_bound(f"{tag} y", cat(got["y"]), ref["y"], tol["y"])
    check_bound(f"{tag} dx", cat(got["dx"]), ref["dx"], tol["dx"])
    for r, s in enumerate(got["sums"]):
        check_bound(f"{tag} sum_g[{r}]", s[:C], ref["sg"][r], tol["sg"][r])
        check_bound(f"{tag} sum_gx[{r}]", s[C:], ref["sgx"][r], tol["sgx"][r])
    if training and running:
        check_bound(f"{tag} running_mean", got["running_mean"], ref["running_mean"], tol["running_mean"])
        check_bound(f"{tag} running_var", got["running_var"], ref["running_var"], tol["running_var"])


EXACT_MOMENTUM = 0.25
EXACT_PARTS = (2, 38, 88)                    # three parts of unequal size, each balanced: 128 rows


def exact_running(C):
    """Running statistics of the exact cases: small integers, so that (1 - 0.25) * running_mean + 0.25 * 0 is exact."""
    return (torch.arange(C).float() % 5 - 2) * 4, torch.arange(C).float() % 3 + 1


def run_exact(ops, M, C, act, dtype, splits=None, dev="cpu", balanced=None):
    """balanced: the parts inside which the signs are balanced, where they are not the parts the step is run on."""
    x, gamma, beta, dy, *_ = exact_case(M, C, splits=balanced or splits)
    return run_ops(ops, x, gamma, beta, dy, act, dtype, splits=splits, running=exact_running(C), eps=0.0, momentum=EXACT_MOMENTUM, dev=dev)


def check_exact(got, M, C, act, dtype, splits=None, balanced=None):
    """Every result of run_exact against the closed form, bit for bit (-0 counted as +0); running_var, which carries the non-dyadic
    n / (n - 1), inside 4 u (|running_var| + unbiased variance): one rounding each for the quotient, the two products and the sum."""
    ans = exact_answers(M, C, act, splits=balanced or splits)
    if balanced is not None and splits is None:
        ans.update(parts=[slice(0, M)], sg=[sum(ans["sg"])], sgx=[sum(ans["sgx"])])
    canon = lambda t: (t.detach().cpu().to(F32) + 0.0).to(t.dtype)
    st = canon(got["st"])
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        same_bits(st[i * C:(i + 1) * C], image(ans[k], F32), f"exact {k}")
    same_bits(st[4 * C:], torch.tensor([1.0 / M, 0, 0, 0]), "exact 1/N")
    k4 = ans["M2"] / M
    for r, p in enumerate(ans["parts"]):
        n = p.stop - p.start
        rec = got["rec"][r].detach().cpu()
        assert int(rec[2 * C:2 * C + 1].view(torch.int32)[0]) == n and not bool(rec[2 * C + 1:].any()), "the count is carried as integer bits"
        same_bits(canon(rec[:2 * C]), image(torch.cat([ans["mean"], n * k4]), F32), f"exact record {r}")
        same_bits(canon(got["y"][r]), image(ans["y"][p], dtype), f"exact y {r}")
        same_bits(canon(got["dx"][r]), image(ans["dx"][p], dtype), f"exact dx {r}")
        same_bits(canon(got["sums"][r]), image(torch.cat([ans["sg"][r], ans["sgx"][r]]), F32), f"exact sums {r}")
    rm0, rv0 = exact_running(C)
    same_bits(canon(got["running_mean"]), (1.0 - EXACT_MOMENTUM) * rm0, "exact running_mean")
    want = (1.0 - EXACT_MOMENTUM) * rv0.double() + EXACT_MOMENTUM * ans["unbiased"]
    check_bound("exact running_var", got["running_var"], want, 4.0 * U * (rv0.double() + ans["unbiased"]))


def all_bits(got):
    """Every tensor run_ops produced, as integers: what two runs on equal inputs must agree on."""
    flat = [got["st"], got["running_mean"], got["running_var"]] + got["rec"] + got["y"] + got["sums"] + got["dx"]
    return [t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]) for t in flat if t is not None]
