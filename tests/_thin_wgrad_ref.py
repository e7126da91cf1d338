"""TEST INFRASTRUCTURE -- epilogue 12 of cs_gemm_nt, the thin layers' weight and bias gradient (include/clipself_hip.h "THIN FORMS",
clipself_amd/csrc/thin.hip, HipOps.thin_wgrad, conv.thin_param_grads, linear.LinearThin).

* `RefOpsThinWgrad(RefOpsThin)`: the CPU backend of tests/_thin_ref plus `thin_wgrad` and `thin_wgrad_workspace` restated from the header's
  text in np.float32 with explicit indices: rows T[m * ld + n]; planes P1[((m / R) * s + n) * R + m % R] and
  P2[((m / R) * (N - s) + (n - s)) * R + m % R]; dY AND X rounded to bf16 (RNE); db the column sums of the rounded dY; dW overwritten;
  workspace[0 .. N) = db and [N .. 16) zeros.  `flaws` plants the errors the checks must reject (WGRAD_FLAWS).
* Exact operands: integers in [-8, 8], so that every product is exact; `bounds` asserts that every sum of |terms| stays below 2^24,
  where fp32 accumulation in any order is exact and the result equals the float64 one bit for bit.
* Random operands: the standard bound of recursive summation, which holds for ANY fixed order of M additions:
  2 * (M + 2) * 2^-24 * sum_m |terms|.  Derived, not measured.
"""
import functools

import numpy as np
import torch

from _thin_ref import BF, F32, TWO24, ExactnessError, RefOpsThin, _np32

U = 2.0 ** -24
REF_CUS = 256                                       # the CU count the CPU backend states the workspace rule with (MI355X)
STEP_ROWS, WG_ROWS, BLOCKS_PER_CU, HEAD = 32, 128, 2, 16       # the header's constants (hip.THIN_WGRAD_*)
WGRAD_FLAWS = ("wg_dy_not_rounded", "db_unrounded", "second_block_first_width", "ragged_tail_dropped", "dw_accumulated", "partial_dropped",
               "x_not_rounded")


class RefOpsThinWgrad(RefOpsThin):
    name = "ref+taps+neck+conv+bn+fc+fpn+thin+wgrad"
    THIN_WGRAD = True

    def __init__(self, flaws=()):
        super().__init__(tuple(f for f in flaws if f not in WGRAD_FLAWS))
        self.wflaws = tuple(f for f in flaws if f in WGRAD_FLAWS)

    def thin_wgrad_partials(self, M):
        return min(-(-M // WG_ROWS), BLOCKS_PER_CU * REF_CUS)

    def thin_wgrad_workspace(self, M, N, K):
        return HEAD + self.thin_wgrad_partials(M) * (N * K + HEAD)

    def thin_wgrad(self, dY, X, dW, db=None, R=0, dY2=None, workspace=None):
        M, K = X.shape
        assert dY.dtype == F32 and X.dtype in (F32, BF) and X.stride(1) == 1 and dW.dtype == F32 and dW.stride(1) == 1
        if R == 0:
            assert dY2 is None and dY.dim() == 2 and dY.shape[0] == M and dY.stride(1) == 1
            N = dY.shape[1]
            s = N
        else:
            N = (dY.numel() + (0 if dY2 is None else dY2.numel())) // M
            s = dY.numel() // M
        if N > 16 or N < 1 or K % 64 or K <= 0 or M <= 0:
            raise RuntimeError("cs_gemm_nt (thin weight gradient): 1 <= N <= 16, K a positive multiple of 64")
        if R < 0 or (R and M % R):
            raise RuntimeError("cs_gemm_nt (thin weight gradient): group is 0 or a divisor of M")
        if R and not 1 <= s <= N:
            raise RuntimeError("cs_gemm_nt (thin weight gradient): split outside [1, N]")
        assert dW.shape[0] >= N and dW.shape[1] >= K and (M == 1 or X.stride(0) >= K)
        need = self.thin_wgrad_workspace(M, N, K)
        if workspace is None:
            workspace = torch.empty(need, dtype=F32)
        elif workspace.dtype != F32 or not workspace.is_contiguous() or workspace.numel() < need:
            raise ValueError(f"thin_wgrad: a contiguous fp32 workspace of {need} floats is needed")
        # ---- dY[m, n] through its explicit index
        if R == 0:
            assert M == 1 or dY.stride(0) >= N
            dy = np.empty((M, N), np.float32)
            src = _np32(dY)
            for n in range(N):
                dy[:, n] = src[:, n]                                   # T[m * ld + n] (the tensor view carries ld)
        else:
            assert dY.is_contiguous() and dY.numel() == M * s and (dY2 is None) == (s == N)
            assert dY2 is None or (dY2.dtype == F32 and dY2.is_contiguous() and dY2.numel() == M * (N - s))
            p1 = _np32(dY).reshape(-1)
            p2 = _np32(dY2).reshape(-1) if dY2 is not None else np.zeros(1, np.float32)
            m = np.arange(M, dtype=np.int64)
            img, pix = m // R, m % R
            dy = np.empty((M, N), np.float32)
            for n in range(N):
                if n < s:
                    dy[:, n] = p1[(img * s + n) * R + pix]
                else:
                    width = s if "second_block_first_width" in self.wflaws else N - s
                    dy[:, n] = p2[np.minimum((img * width + (n - s)) * R + pix, p2.size - 1)]
        dyr = dy if "wg_dy_not_rounded" in self.wflaws else _np32(torch.from_numpy(dy).to(BF))
        x = _np32(X) if ("x_not_rounded" in self.wflaws) else _np32(X.to(BF))
        keep = np.ones(M, bool)
        if "ragged_tail_dropped" in self.wflaws:
            keep[M // STEP_ROWS * STEP_ROWS:] = False
        if "partial_dropped" in self.wflaws:                            # the last workgroup's row blocks: b, b + P, b + 2 P, ...
            P = self.thin_wgrad_partials(M)
            keep[(np.arange(M) // WG_ROWS) % P == P - 1] = False
        dw = (dyr[keep].T.astype(np.float32) @ x[keep]).astype(np.float32)
        dbv = (dy if "db_unrounded" in self.wflaws else dyr)[keep].sum(0, dtype=np.float32)
        out = torch.from_numpy(dw)
        if "dw_accumulated" in self.wflaws:
            dW[:N, :K] += out
        else:
            dW[:N, :K] = out
        workspace[:N] = torch.from_numpy(dbv)
        workspace[N:HEAD] = 0
        if db is not None:
            assert db.dtype == F32 and db.numel() == N
            db.view(-1).copy_(workspace[:N])
        return workspace


class Counting(RefOpsThinWgrad):
    """The backend with its parameter-gradient calls counted; direct=False hides THIN_WGRAD (today's backend, call for call)."""

    def __init__(self, direct=True):
        super().__init__()
        self.THIN_WGRAD = direct
        self.calls = {"colsum_bf16": 0, "gemm_wgrad_tn": 0, "gemm_wgrad": 0, "thin_wgrad": 0, "cast_f32_bf16": 0, "nchw_to_rows": 0}

    def _count(name):
        def f(self, *a, **k):
            self.calls[name] += 1
            return getattr(super(Counting, self), name)(*a, **k)
        return f

    colsum_bf16, gemm_wgrad_tn, gemm_wgrad = _count("colsum_bf16"), _count("gemm_wgrad_tn"), _count("gemm_wgrad")
    thin_wgrad, cast_f32_bf16, nchw_to_rows = _count("thin_wgrad"), _count("cast_f32_bf16"), _count("nchw_to_rows")


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def operands(M, N, K, kind):
    """(x fp32 [M, K], dy fp32 [M, N]) computed once, shared read-only.  exact: integers in [-8, 8]; random: fp32 values bf16 does NOT
    hold, so that both roundings act; ternary: {-1, 0, 1}."""
    g = torch.Generator().manual_seed(M * 7919 + N * 131 + K + 17 * len(kind))
    if kind == "exact":
        r = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)
    elif kind == "ternary":
        r = lambda *s: torch.randint(-1, 2, s, generator=g).to(F32)
    else:
        r = lambda *s: torch.randn(*s, generator=g)
    return r(M, K), r(M, N)


def rows_to_planes(rows, R, c0, c1):
    M = rows.shape[0]
    return rows[:, c0:c1].reshape(M // R, R, c1 - c0).permute(0, 2, 1).contiguous()


def dy_forms(dy, R, N):
    """[(name, R argument, dY, dY2)]: rows, planes in one block, and at N == 15 planes split at 3."""
    forms = [("rows", 0, dy.contiguous(), None), ("planes", R, rows_to_planes(dy, R, 0, N), None)]
    if N == 15:
        forms.append(("planes3", R, rows_to_planes(dy, R, 0, 3), rows_to_planes(dy, R, 3, N)))
    return forms


def reference(x, dy):
    """float64 results of the bf16-rounded operands and the per-element bounds: (dw64, db64, bound_dw, bound_db)."""
    M = x.shape[0]
    xb, dyb = x.to(BF).double(), dy.to(BF).double()
    dw, db = dyb.T @ xb, dyb.sum(0)
    adw, adb = dyb.abs().T @ xb.abs(), dyb.abs().sum(0)
    return dw, db, 2.0 * (M + 2) * U * adw, 2.0 * (M + 2) * U * adb, adw, adb


def assert_exact_sums(adw, adb):
    if not (float(adw.max()) < TWO24 and float(adb.max()) < TWO24):
        raise ExactnessError(f"a sum of |terms| reaches {max(float(adw.max()), float(adb.max()))} >= 2^24: the case, not a kernel, is wrong")


def check_result(dw, db, x, dy, kind, what):
    """dw [N, K], db [N] (fp32, on any device) against float64: bit for bit where kind is exact / ternary, inside the bound otherwise.
    -> the worst fraction of the bound (0 for exact kinds)."""
    dw64, db64, bdw, bdb, adw, adb = reference(x, dy)
    dw, db = dw.detach().cpu(), db.detach().cpu()
    assert dw.dtype == F32 and db.dtype == F32
    if kind != "random":
        assert_exact_sums(adw, adb)
        assert torch.equal(dw.double(), dw64), f"{what}: dW differs in {int((dw.double() != dw64).sum())} of {dw.numel()} elements"
        assert torch.equal(db.double(), db64), f"{what}: db differs in {int((db.double() != db64).sum())} of {db.numel()} elements"
        return 0.0
    worst = 0.0
    for name, got, want, bound in (("dW", dw, dw64, bdw), ("db", db, db64, bdb)):
        frac = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
        print(f"THIN WGRAD {what} {name}: worst {frac:.4f} of the bound")
        assert frac <= 1.0, f"{what}: {name} at {frac:.3f} x its bound"
        worst = max(worst, frac)
    return worst


def rounding_case():
    """dY of +-{257, 1027, 515, 2049, 3}: integers bf16 does not hold (the case of _thin_ref.check_dy_rounding), X exact."""
    M, N, K = 105, 15, 64
    x, _ = operands(M, N, K, "exact")
    g = torch.Generator().manual_seed(99)
    dy = (torch.randint(0, 2, (M, N), generator=g) * 2 - 1).to(F32) * torch.tensor([257.0, 1027.0, 515.0, 3.0, 2049.0])[torch.randint(0, 5, (M, N), generator=g)]
    assert not torch.equal(dy.to(BF).to(F32), dy)
    return x, dy


# ------------------------------------------------------------------------------------------------ LinearThin
def linear_thin(ops, weight, bias, device="cpu", fused=True):
    from clipself_amd.linear import LinearThin
    m = LinearThin(weight.shape[1], weight.shape[0], ops=ops, fused=fused)
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    return m.to(device)


def run_linear(m, x, dy, dtype=F32, shape=None):
    """One forward + backward of the layer on x [rows, in] (cast to dtype, viewed as `shape`) -> (y rows, dx rows, dw, db)."""
    dev = m.weight.device
    m.zero_grad()
    inp = x.detach().to(dev).to(dtype).clone()
    if shape is not None:
        inp = inp.view(*shape)
    inp.requires_grad_(True)
    y = m(inp)
    y.backward(dy.to(dev).to(y.dtype).view(y.shape))
    return y.detach().reshape(-1, y.shape[-1]), inp.grad.reshape(x.shape), m.weight.grad, m.bias.grad


def check_linear(ops, shape, kind, dtype=F32, device="cpu", view=None):
    """LinearThin on `ops` against float64 autograd (tests/_fc_ref.case without activation): exact bit for bit, random inside the bounds."""
    import _fc_ref
    from _thin_ref import same_bits
    x, w, b, dy, ref = _fc_ref.case(shape, kind, act=None)
    rows, inf, out = shape
    m = linear_thin(ops, w, b, device)
    y, dx, dw, db = run_linear(m, x, dy, dtype, view)
    assert y.dtype == F32 and dx.dtype == dtype and dw.dtype == F32 and db.dtype == F32
    if kind == "exact":
        for got, key in ((y, "y"), (dx, "dx"), (dw, "dw"), (db, "db")):
            same_bits(got, ref[key], f"LinearThin {shape} {dtype}: {key}")
        return
    _fc_ref.check_bound("y", y, ref["y"], _fc_ref.bound(ref["ay"], inf, 1))
    _fc_ref.check_bound("dx", dx, ref["dx"], _fc_ref.bound(ref["adx"], out, 1, ref["dx"], dtype == BF))
    _fc_ref.check_bound("dw", dw, ref["dw"], _fc_ref.bound(ref["adw"], rows))
    _fc_ref.check_bound("db", db, ref["db"], _fc_ref.bound(ref["adb"], rows))
