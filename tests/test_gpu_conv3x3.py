"""`-m gpu`: the detector heads' 3 x 3 convolutions as implicit GEMMs (include/clipself_conv.h, clipself_amd/conv.py) on the MI355X.

Kernels alone (HipOps.conv3x3, HipOps.im2col3x3): outputs are handed in as NaN, every call runs twice with equal bits.  Exact operands:
y, dx, dw, db bit for bit against float64 autograd on both routes, fp32 and bf16 outputs (bf16 = the round-to-nearest-even image of the
float64 result).  Random operands: inside the derived per-element bounds of tests/_conv_ref.py, the worst error / bound printed
(profiles/conv3x3_parity.md).  Padded row strides, non-channel-last inputs, the whole module under autograd, and the read / write
extents of both entry points inside the poisoned halos of tests/_extents.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _conv_ref import (BF, F32, ROUTES, SHAPE_IDS, SHAPES, bounds, case, check_bound, index_im2col, layer, map_of, rne_bf16,  # noqa: E402
                       rows_of, run_layer, same_bits)
from _extents import run_case  # noqa: E402
from clipself_amd.conv import pack_weights  # noqa: E402
from clipself_amd.det_layer import pad_cols  # noqa: E402

EPI = {BF: 0, F32: 1}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _twice(fn):
    """fn() -> output tensor(s), freshly NaN-filled inside; run twice, the same bits both times."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        it = {2: torch.int16, 4: torch.int32}[u.element_size()]
        assert torch.equal(u.view(it), v.view(it)), "two runs on equal inputs differ"
    return a


def _conv_rows(hip, route, X, Wm, bias, N, H, W, dtype):
    """One convolution of the rows X with packed weights Wm into a NaN-filled output, by the implicit kernel or by im2col + cs_gemm_nt
    (K padded with zero columns to a multiple of 64 where 9 * C is none)."""
    M, Ci = X.shape
    out = _nan((M, Wm.shape[0]), dtype)
    if route == "implicit":
        hip.conv3x3(X, Wm, out, bias, N, H, W)
        return out
    Wp = pad_cols(hip, Wm)
    cols = torch.zeros(M, Wp.shape[1], dtype=BF, device="cuda")
    cols[:, :9 * Ci] = float("nan")
    hip.im2col3x3(X, cols[:, :9 * Ci], N, H, W)
    hip.gemm_nt(cols, Wp, out, bias, epi=EPI[dtype])
    return out


def _results(hip, shape, kind, route, dtype):
    """y, dx (in `dtype`), dw, db (fp32) of a case from the kernels alone; dx takes `route` where the implicit kernel covers it."""
    N, H, W, Cin, Cout = shape
    x, w, b, dy, ref = case(shape, kind)
    Wg, WgT = (t.cuda() for t in pack_weights(w))
    X, dY, bias = rows_of(x).cuda(), rows_of(dy).cuda(), b.cuda()
    y = _twice(lambda: _conv_rows(hip, route, X, Wg, bias, N, H, W, dtype))
    dx = _twice(lambda: _conv_rows(hip, route if Cout % 64 == 0 else "im2col", dY, WgT, None, N, H, W, dtype))

    def grads():
        cols = _nan((N * H * W, 9 * Cin), BF)
        hip.im2col3x3(X, cols, N, H, W)
        dWg, db = torch.zeros(Cout, 9 * Cin, device="cuda"), torch.zeros(Cout, device="cuda")
        ws = torch.empty(hip.gemm_wgrad_tn_workspace(Cout, 9 * Cin, N * H * W), dtype=torch.uint8, device="cuda")
        hip.gemm_wgrad_tn(dY, cols, dWg, ws)
        hip.colsum_bf16(dY, db)
        return dWg, db
    dWg, db = _twice(grads)
    dw = dWg.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
    return dict(y=map_of(y, N, H, W).contiguous(), dx=map_of(dx, N, H, W).contiguous(), dw=dw, db=db), ref


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_exact_operands_bit_for_bit(hip, shape, route):
    assert hip.CONV3X3
    for dtype in (F32, BF):
        got, ref = _results(hip, shape, "exact", route, dtype)
        img = (lambda t: t.to(F32)) if dtype == F32 else rne_bf16
        same_bits(got["y"], img(ref["y"]), f"{route} {dtype} y")
        same_bits(got["dx"], img(ref["dx"]), f"{route} {dtype} dx")
        same_bits(got["dw"], ref["dw"].to(F32), f"{route} dw")
        same_bits(got["db"], ref["db"].to(F32), f"{route} db")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_random_operands_within_the_derived_bounds(hip, shape, route):
    for dtype in (F32, BF):
        got, ref = _results(hip, shape, "random", route, dtype)
        tol = bounds(ref, shape, bf16_out=dtype == BF)
        for k in ("y", "dx", "dw", "db"):
            check_bound(f"CONV PARITY {SHAPE_IDS[SHAPES.index(shape)]} {route} {str(dtype)[6:]} {k}", got[k], ref[k], tol[k])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_im2col_is_the_index_expression_bit_for_bit(hip, shape):
    """Pure data movement: every element of the explicit matrix, whole and as a chunk with row0 > 0, with padded row strides whose
    padding holds NaN (input) and must keep its fill (output)."""
    N, H, W, Cin, Cout = shape
    M = N * H * W
    x = case(shape, "random")[0]
    X = rows_of(x)
    want = index_im2col(X, N, H, W, 0, M)
    Xp = _nan((M, Cin + 8), BF)
    Xp[:, :Cin] = X.cuda()
    for row0 in sorted({0, M // 3}):
        rows = M - row0
        cols = torch.full((rows, 9 * Cin + 16), 7.0, dtype=BF, device="cuda")
        cols[:, :9 * Cin] = float("nan")
        hip.im2col3x3(Xp[:, :Cin], cols[:, :9 * Cin], N, H, W, row0)
        same_bits(cols[:, :9 * Cin], want[row0:], f"cols from row {row0}")
        assert bool((cols[:, 9 * Cin:] == 7.0).all()), "im2col3x3 wrote into the row padding"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_padded_row_strides(hip, shape):
    """ldx > Cin and ldy > Cout: the padding of x holds NaN (never read), the padding of y keeps its fill (never written)."""
    N, H, W, Cin, Cout = shape
    M = N * H * W
    x, w, b, dy, ref = case(shape, "exact")
    Wg = pack_weights(w)[0].cuda()
    Xp = _nan((M, Cin + 24), BF)
    Xp[:, :Cin] = rows_of(x).cuda()
    for dtype in (F32, BF):
        Y = torch.full((M, Cout + 12), 7.0, dtype=dtype, device="cuda")
        Y[:, :Cout] = float("nan")
        hip.conv3x3(Xp[:, :Cin], Wg, Y[:, :Cout], b.cuda(), N, H, W)
        want = ref["y"].to(F32) if dtype == F32 else rne_bf16(ref["y"])
        same_bits(map_of(Y[:, :Cout], N, H, W).contiguous(), want, f"{dtype} y with padded strides")
        assert bool((Y[:, Cout:] == 7.0).all()), "conv3x3 wrote into the row padding"


def test_wrappers_refuse_what_the_header_excludes(hip):
    X = torch.zeros(2 * 3 * 5, 64, dtype=BF, device="cuda")
    Wg = torch.zeros(16, 9 * 64, dtype=BF, device="cuda")
    Y = torch.zeros(30, 16, device="cuda")
    hip.conv3x3(X, Wg, Y, None, 2, 3, 5)                                               # bias may be NULL
    p = lambda t: t.data_ptr()
    lib = hip.lib
    assert lib.csc_conv3x3(p(X), 64, p(Wg), 576, None, p(Y), 16, 0, 2, 3, 5, 32, 16, None) == 1       # Cin % 64: outside the coverage
    assert lib.csc_conv3x3(p(X), 64, p(Wg), 576, None, p(Y), 16, 0, 2, 3, 5, 64, 12, None) == 1       # Cout % 8
    assert lib.csc_im2col3x3(p(X), 64, p(Y), 576, 0, 1, 2, 3, 5, 12, None) == 1                        # Cin % 8
    assert lib.csc_conv3x3(p(X), 60, p(Wg), 576, None, p(Y), 16, 0, 2, 3, 5, 64, 16, None) == -1 and b"stride" in lib.cs_last_error()
    assert lib.csc_conv3x3(p(X) + 2, 64, p(Wg), 576, None, p(Y), 16, 0, 2, 3, 5, 64, 16, None) == -1  # alignment
    assert lib.csc_conv3x3(p(X), 64, p(Wg), 576, None, p(Y), 16, 0, 0, 3, 5, 64, 16, None) == -1      # N = 0
    assert lib.csc_conv3x3(p(X), 64, p(Wg), 576, None, p(Y), 16, 0, 1 << 20, 1 << 10, 2, 64, 16, None) == -1   # 2^31 rows
    assert lib.csc_im2col3x3(p(X), 64, p(Y), 576, 29, 2, 2, 3, 5, 64, None) == -1                      # rows past the map
    assert lib.csc_im2col3x3(p(X), 64, p(Y), 576, 30, 0, 2, 3, 5, 64, None) == 0                       # an empty chunk
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.conv3x3(X[:, :32], Wg[:, :288], Y, None, 2, 3, 5)
    with pytest.raises(ValueError):
        hip.conv3x3(X.float(), Wg, Y, None, 2, 3, 5)
    with pytest.raises(ValueError):
        hip.conv3x3(X, Wg, Y, None, 2, 5, 5)                                           # rows do not match N*H*W
    with pytest.raises(ValueError):
        hip.im2col3x3(X, torch.zeros(31, 576, dtype=BF, device="cuda"), 2, 3, 5)


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_module_under_autograd(hip, shape, route):
    x, w, b, dy, ref = case(shape, "exact")
    m = layer(hip, w, b, device="cuda", fused=True, route=route)
    y, dx, dw, db = run_layer(m, x, dy)
    assert y.is_cuda and y.dtype == F32 and y.permute(0, 2, 3, 1).is_contiguous() and tuple(dw.shape) == tuple(w.shape)
    for k, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        same_bits(got, ref[k].to(F32), f"{route} {k}")
    again = run_layer(m, x, dy, channel_last=False)                                     # an NCHW-contiguous input: nchw_to_rows; equal bits
    assert all(torch.equal(a, c) for a, c in zip((y, dx, dw, db), again))
    yb, dxb, dwb, dbb = run_layer(m, x, dy, dtype=BF)
    same_bits(yb, rne_bf16(ref["y"]), f"{route} bf16 y")
    same_bits(dxb, rne_bf16(ref["dx"]), f"{route} bf16 dx")
    same_bits(dwb, ref["dw"].to(F32), f"{route} dw of a bf16 input")
    xr, wr, br, dyr, rref = case(shape, "random")
    mr = layer(hip, wr, br, device="cuda", fused=True, route=route)
    got = dict(zip(("y", "dx", "dw", "db"), run_layer(mr, xr, dyr)))
    tol = bounds(rref, shape)
    for k in ("y", "dx", "dw", "db"):
        check_bound(f"module {route} {k}", got[k], rref[k], tol[k])


def test_module_on_strided_input_and_default_backend(hip):
    shape = SHAPES[2]
    N, H, W, Cin, Cout = shape
    x, w, b, dy, ref = case(shape, "exact")
    m = layer(None, w, b, device="cuda", fused=True)                                    # the process-wide HipOps of det_backend
    wide = torch.full((N, Cin + 8, H, W + 3), float("nan"), device="cuda")
    wide[:, 4:4 + Cin, :, 1:1 + W] = x.cuda()
    y = m(wide[:, 4:4 + Cin, :, 1:1 + W])                                               # neither NCHW-contiguous nor channel-last
    assert "Conv3x3" in type(y.grad_fn).__name__
    same_bits(y.detach(), ref["y"].to(F32), "strided input")
    stack = torch.nn.Sequential(layer(hip, w, b, device="cuda", fused=True), torch.nn.ReLU())
    out = stack(x.cuda().contiguous(memory_format=torch.channels_last))
    assert out.permute(0, 2, 3, 1).is_contiguous()                                      # channel-last stays channel-last through torch's ReLU
    with pytest.raises(NotImplementedError):
        layer(hip, w, b, fused=True)(x)                                                 # a CPU tensor


# ------------------------------------------------------------------------------------------------ extents
def _extent_case(shape, what, dtype):
    N, H, W, Cin, Cout = shape
    M = N * H * W
    x, w, b, dy, _ = case(shape, "random")

    def fn(ops, a):
        X = a.inp(rows_of(x), a.ld(Cin, 8))                                             # NaN halo rows before and after, NaN row padding
        if what == "conv":
            Wg = a.inp(pack_weights(w)[0], a.ld(9 * Cin, 8))
            Y = a.out((M, Cout), dtype, a.ld(Cout, 4))
            ops.conv3x3(X, Wg, Y, a.inp(b), N, H, W)
            return {"y": Y}
        row0 = M // 3
        cols = a.out((M - row0, 9 * Cin), BF, a.ld(9 * Cin, 8))                         # exactly rows * ldc elements inside the sentinel
        ops.im2col3x3(X, cols, N, H, W, row0)
        return {"cols": cols}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_kernels_stay_inside_their_extents(hip, shape, pad):
    for what, dtype in (("conv", F32), ("conv", BF), ("im2col", BF)):
        key = f"conv3x3.{what}[{shape},{dtype}]"
        problems = run_case(hip, _extent_case(shape, what, dtype), "cuda", pad, key=key)
        assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)
