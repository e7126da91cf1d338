"""Poisoned-halo harness and case table: pins what every op behind the C ABI (include/clipself_hip.h) may read and write.

A case is a function `fn(ops, a)` that builds its tensors through the arena `a`, calls ONE op family on `ops` (HipOps on the GPU,
RefOps on the CPU) and returns {name: output tensor}.  run_case() runs it twice:

  compact -- exactly-sized tensors, natural row strides, clean (zero) padding where an op's contract needs a padded row;
  halo    -- every tensor is a view inside a larger allocation: >= 256 rows of halo before and after (the largest row tile, so that a
             tile-sized over-read stays inside memory the test owns), row stride = natural + pad (pad 8 and 64).  Float input halos are
             NaN, byte / int input halos a fixed pattern; outputs and workspaces sit in a sentinel-filled allocation, workspaces with
             exactly the bytes the op's *_workspace() asks for.

and reports (a) every output that is not bit-identical between the two runs (integer views: NaN != NaN) and (b) every output /
workspace allocation whose halo changed.  A kernel that reads past its extents picks up NaN (a); one that ignores a row stride reads or
writes the wrong elements (a, b); one that writes past its view trips (b).  No tolerance is involved; the one exception (an op that picks
another summation path from the alignment of its row stride) returns an Approx and is held to that op's bound in test_gpu_ops.py.
"""
import math

import torch

from oracle.ops_ref import RefOps
from test_gpu_ops import BF, F32, rel, rnd          # the op suite's seeded inputs and error measure

HALO_ROWS = 256                     # the largest row tile of any kernel (256-row GEMM tiles)
WS_HALO = 1 << 16                   # bytes of sentinel on either side of a workspace
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    return t.detach().contiguous().view(_INT[t.element_size()])


def up(n, m):
    return (n + m - 1) // m * m


class Approx:
    """Replaces the bit-for-bit comparison of one output: `got` against an fp64 reference at an existing bound."""

    def __init__(self, got, want, tol):
        self.got, self.want, self.tol = got, want, tol


def _pattern(dtype, byte):
    """Element whose bytes are `byte` (ints) / a NaN with that payload (floats)."""
    size = torch.empty(0, dtype=dtype).element_size()
    v = int.from_bytes(bytes([byte] * size), "little")
    if dtype.is_floating_point:
        v |= {2: 0xFF80, 4: 0xFFC00000}[size]
    if dtype != torch.uint8 and v >= 1 << (8 * size - 1):
        v -= 1 << (8 * size)
    return v, _INT[size]


class Arena:
    def __init__(self, device, poison, pad):
        self.dev, self.poison, self.pad = device, poison, (pad if poison else 0)
        self.guards = []                                  # (name, allocation, snapshot, view maker, documented zero pad)

    def ld(self, width, mult=1):
        """Row stride of a `width`-wide matrix whose op wants multiples of `mult`: the natural one, plus the pad in the halo run."""
        return up(width, mult) + up(self.pad, mult)

    def _place(self, shape, dtype, ld, fill, halo=None):
        shape = tuple(shape)
        n = math.prod(shape)
        if ld is None:                                    # contiguous tensor, halo before and after
            row = shape[-1] if len(shape) > 1 else 2      # vectors: 512 elements (a 256-column tile twice over)
            h = (HALO_ROWS * row if halo is None else halo) if self.poison else 0
            total = h + n + h
            mk = lambda flat: flat[h:h + n].view(shape)
        else:
            assert len(shape) == 2 and ld >= shape[1]
            h = HALO_ROWS if self.poison else 0
            total = (h + shape[0] + h) * ld
            mk = lambda flat: flat.view(-1, ld)[h:h + shape[0], :shape[1]]
        val, idt = fill
        flat = torch.full((max(total, 1),), val, dtype=idt, device=self.dev).view(dtype)
        return flat, mk

    def inp(self, data, ld=None):
        """Read-only operand holding `data`; halo NaN / 0xA5 bytes (compact run: zeros in the padding of a padded row)."""
        fill = _pattern(data.dtype, 0xA5) if self.poison else (0, _INT[data.element_size()])
        flat, mk = self._place(data.shape, data.dtype, ld, fill)
        v = mk(flat)
        v.copy_(data)
        return v

    def out(self, shape, dtype, ld=None, init=None, zero_pad=0, name=None, halo=None):
        """Output inside a sentinel-filled allocation (a different sentinel per run, so an element the op leaves unwritten shows up
        as a difference).  init: seeded contents for outputs that accumulate or are written in part.  zero_pad: columns right of the
        view that the header documents as written with zeros (checked as exactly that on the kernels, and excluded from the halo)."""
        flat, mk = self._place(shape, dtype, ld, _pattern(dtype, 0xA5 if self.poison else 0xC3), halo)
        v = mk(flat)
        if init is not None:
            v.copy_(init)
        assert zero_pad == 0 or (ld is not None and shape[1] + zero_pad <= ld)
        self.guards.append((name or f"out{len(self.guards)}", flat, flat.clone(), mk, zero_pad))
        return v

    def ws(self, nbytes):
        return self.out((max(int(nbytes), 1),), torch.uint8, name=f"workspace{len(self.guards)}", halo=WS_HALO)

    def halo_problems(self, is_ref):
        bad = []
        for name, flat, snap, mk, zp in self.guards:
            cur, ref = bits(flat).clone(), bits(snap).clone()
            v = mk(cur)
            mk(ref).copy_(v)                              # the view itself may change
            if zp:
                pad_c = torch.as_strided(cur, (v.shape[0], zp), v.stride(), v.storage_offset() + v.shape[1])
                pad_r = torch.as_strided(ref, (v.shape[0], zp), v.stride(), v.storage_offset() + v.shape[1])
                if not is_ref:                            # the reference works on tensors and cannot see these columns
                    if int((pad_c != 0).sum()) != 0:
                        bad.append(f"{name}: documented zero padding holds {int((pad_c != 0).sum())} non-zero elements")
                    pad_r.copy_(pad_c)
            diff = cur != ref
            if bool(diff.any()):
                idx = torch.nonzero(diff)[:, 0]
                bad.append(f"{name}: {int(diff.sum())} halo elements changed (allocation offsets {idx[:4].tolist()}..., view starts at "
                           f"{mk(torch.arange(cur.numel(), device=cur.device)).reshape(-1)[0].item()})")
        return bad


_COMPACT = {}          # (ops name, case id) -> compact-run outputs (bits, on the CPU): computed once, shared by the pads


def run_case(ops, fn, device, pad, key=None):
    """-> list of problems (empty = the op respects its declared extents on this case)."""
    def once(poison):
        a = Arena(device, poison, pad)
        outs = fn(ops, a)
        if device != "cpu":
            torch.cuda.synchronize()
        return a, outs

    problems = []

    def freeze(outs, tag):
        res = {}
        for k, v in outs.items():
            if isinstance(v, Approx):
                r = rel(v.got, v.want)
                print(f"{key} {tag} {k}: rel {r:.3e} (bound {v.tol:.1e})")
                if not (r <= v.tol):
                    problems.append(f"{k} ({tag} run): rel {r:.3e} > {v.tol:.1e} against the fp64 reference")
            else:
                res[k] = bits(v).cpu()
        return res

    ck = (ops.name, key)
    if key is None or ck not in _COMPACT:
        _, o0 = once(False)
        _COMPACT[ck] = freeze(o0, "compact")
    want = _COMPACT[ck]
    a1, o1 = once(True)
    got = freeze(o1, "halo")
    assert got.keys() == want.keys()
    for k in want:
        if got[k].shape != want[k].shape:
            problems.append(f"{k}: shape {tuple(got[k].shape)} != {tuple(want[k].shape)}")
            continue
        d = got[k] != want[k]
        if bool(d.any()):
            problems.append(f"{k}: {int(d.sum())} of {d.numel()} elements differ from the compact run, first at {torch.nonzero(d)[0].tolist()}")
    problems += a1.halo_problems(ops.name == "ref")
    return problems


# ================================================================================================ case table
CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


_ref = RefOps()
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ---- GEMMs.  M in {1, 131, 259}: one row / no multiple of 4, 32, 128 / just past 256.  N a multiple of 32 but not of 128.  K in {64, 192}.
GEMM_FLAGS = [0, 1, 0x10, 0x20, 0x30, 0x31, 0x70, 0x71, 0x8070, 0x90, 0xB0, 0x10B0]       # the list of test_gemm_bf16_bias
GEMM_SHAPES = [(1, 96, 64), (131, 96, 192), (259, 160, 64)]


def _gemm_case(epi, M, N, K):
    def fn(ops, a):
        A = a.inp(rnd((M, K), BF, seed=1), a.ld(K, 8))
        B = a.inp(rnd((N, K), BF, 0.05, seed=2), a.ld(K, 8))
        bias = a.inp(rnd((N,), F32, seed=3))
        outs = {}
        for fl in GEMM_FLAGS:
            if epi in (0, 7, 8):
                C = a.out((M, N), BF, a.ld(N, 4))
                ops.gemm_nt(A, B, C, bias, epi=epi, flags=fl)
            elif epi == 1:
                C = a.out((M, N), F32, a.ld(N, 4))
                ops.gemm_nt(A, B, C, bias, epi=1, flags=fl)
            elif epi == 2:                                 # in place: C is the residual
                C = a.out((M, N), F32, a.ld(N, 4), init=rnd((M, N), F32, seed=4))
                ops.gemm_nt(A, B, C, bias, C, epi=2, flags=fl)
            else:
                assert epi == 3
                C = a.out((M, N // 2), BF, a.ld(N // 2, 4))
                ops.gemm_nt(A, B, C, bias, epi=3, group=N // 2, flags=fl)
            outs[f"C[flags={fl:#x}]"] = C
        return outs
    return fn


for _epi in (0, 1, 2, 3, 7, 8):
    for _M, _N, _K in GEMM_SHAPES:
        case(f"gemm_nt.epi{_epi}[{_M},{_N},{_K}]")(_gemm_case(_epi, _M, _N, _K))


def _patch_case(nimg, G, N, K):
    def fn(ops, a):                                        # epi 5: rows b*(G+1) (the CLS rows) are not written
        A = a.inp(rnd((nimg * G, K), BF, seed=14), a.ld(K, 8))
        W = a.inp(rnd((N, K), BF, 0.1, seed=15), a.ld(K, 8))
        bias = a.inp(rnd((N,), F32, seed=16))
        ldc = a.ld(N, 4)
        pos = a.inp(rnd((G + 1, N), F32, seed=17), ldc)    # extra shares C's row stride
        outs = {}
        for fl in GEMM_FLAGS:
            C = a.out((nimg * (G + 1), N), F32, ldc, init=rnd((nimg * (G + 1), N), F32, seed=18))
            ops.gemm_nt(A, W, C, bias, pos, epi=5, group=G, flags=fl)
            outs[f"C[flags={fl:#x}]"] = C
        return outs
    return fn


case("gemm_nt.epi5[1x1,96,64]")(_patch_case(1, 1, 96, 64))
case("gemm_nt.epi5[7x37,160,192]")(_patch_case(7, 37, 160, 192))

LN_GEMM_FLAGS = [0, 0x10, 0x20, 0x30, 0x70, 0x90, 0xB0, 0x10B0]       # the list of test_block_layernorms_folded_into_gemms


def _rowstats(M, seed):
    return rnd((M,), F32, 0.3, seed=seed), rnd((M,), F32, 0.2, seed=seed + 1).abs() + 0.5


def _gemm_ln_resid_case(M, N, K, epi, extras):
    def fn(ops, a):                                        # epi 2 / 6: fp32 residual in place (+ statistics partials, + bf16 copy)
        A = a.inp(rnd((M, K), BF, seed=70), a.ld(K, 8))
        B = a.inp(rnd((N, K), BF, 0.1, seed=71), a.ld(K, 8))
        bias = a.inp(rnd((N,), F32, seed=73))
        mean, rstd = _rowstats(M, 74)
        kw = dict(ln_mean=a.inp(mean), ln_rstd=a.inp(rstd), ln_colsum=a.inp(rnd((N,), F32, seed=76))) if epi == 6 else {}
        outs = {}
        for fl in LN_GEMM_FLAGS:
            x = a.out((M, N), F32, a.ld(N, 4), init=rnd((M, N), F32, 2.0, seed=72))
            outs[f"x[flags={fl:#x}]"] = x
            if extras:
                P = (N + 63) // 64
                part = a.out((P, M, 2), F32, init=torch.zeros(P, M, 2))
                xb = a.out((M, N), BF, a.ld(N, 4))
                kw.update(stats_part=part, xb_out=xb)
                outs[f"part[flags={fl:#x}]"], outs[f"xb[flags={fl:#x}]"] = part, xb
            ops.gemm_nt_ln(A, B, x, bias=bias, extra=x, epi=epi, flags=fl, **kw)
        return outs
    return fn


def _gemm_ln_bf16_case(M, N, K, epi, stats):
    def fn(ops, a):                                        # epi 0 / 3 with the LayerNorm in front folded in (+ statistics of the SwiGLU output)
        A = a.inp(rnd((M, K), BF, seed=80), a.ld(K, 8))
        B = a.inp(rnd((N, K), BF, 0.1, seed=81), a.ld(K, 8))
        bias = a.inp(rnd((N,), F32, seed=82))
        mean, rstd = _rowstats(M, 83)
        mean, rstd, cs = a.inp(mean), a.inp(rstd), a.inp(rnd((N,), F32, seed=85))
        W = N // 2 if epi == 3 else N
        outs = {}
        for fl in LN_GEMM_FLAGS:
            C = a.out((M, W), BF, a.ld(W, 4))
            kw = {}
            if stats:
                P = 4 * ((W + 127) // 128)                 # slices past the last hidden unit are never read back: seeded, so that either is fine
                kw["stats_part"] = outs[f"part[flags={fl:#x}]"] = a.out((P, M, 2), F32, init=torch.zeros(P, M, 2))
            ops.gemm_nt_ln(A, B, C, bias=bias, ln_mean=mean, ln_rstd=rstd, ln_colsum=cs, epi=epi, group=W if epi == 3 else 0, flags=fl, **kw)
            outs[f"C[flags={fl:#x}]"] = C
        return outs
    return fn


for _M, _N, _K in [(131, 96, 192), (259, 160, 64)]:
    case(f"gemm_nt_ln.epi2+stats+xb[{_M},{_N},{_K}]")(_gemm_ln_resid_case(_M, _N, _K, 2, True))
    case(f"gemm_nt_ln.epi6[{_M},{_N},{_K}]")(_gemm_ln_resid_case(_M, _N, _K, 6, False))
    case(f"gemm_nt_ln.epi6+stats+xb[{_M},{_N},{_K}]")(_gemm_ln_resid_case(_M, _N, _K, 6, True))
    case(f"gemm_nt_ln.epi0[{_M},{_N},{_K}]")(_gemm_ln_bf16_case(_M, _N, _K, 0, False))
    case(f"gemm_nt_ln.epi3[{_M},{_N},{_K}]")(_gemm_ln_bf16_case(_M, _N, _K, 3, False))
    case(f"gemm_nt_ln.epi3+stats[{_M},{_N},{_K}]")(_gemm_ln_bf16_case(_M, _N, _K, 3, True))


def _split_case(M, N, K, form):
    def fn(ops, a):
        A = a.inp(rnd((M, K), BF, seed=90), a.ld(K, 8))
        B = a.inp(rnd((N, K), BF, 0.1, seed=91), a.ld(K, 8))
        bias = a.inp(rnd((N,), F32, seed=92))
        mean, rstd = _rowstats(M, 93)
        mean, rstd, cs = a.inp(mean), a.inp(rstd), a.inp(rnd((N,), F32, seed=95))
        x0 = rnd((M, N), F32, 2.0, seed=96)
        h0, l0 = RefOps.split_planes(x0)
        P = (N + 63) // 64
        ldp = a.ld(N, 8)
        if form == "f32_in":                               # fp32 stream in -> planes + statistics out
            hi, lo = a.out((M, N), BF, ldp), a.out((M, N), torch.int16, ldp)
            part = a.out((P, M, 2), F32, init=torch.zeros(P, M, 2))
            ops.gemm_nt_ln_split(A, B, hi, lo, bias, mean, rstd, cs, x_in=a.inp(x0, a.ld(N, 4)), stats_part=part)
            return {"hi": hi, "lo": lo, "part": part}
        if form == "split":                                # planes updated in place
            hi, lo = a.out((M, N), BF, ldp, init=h0), a.out((M, N), torch.int16, ldp, init=l0)
            part = a.out((P, M, 2), F32, init=torch.zeros(P, M, 2))
            ops.gemm_nt_ln_split(A, B, hi, lo, bias, mean, rstd, cs, stats_part=part)
            return {"hi": hi, "lo": lo, "part": part}
        x = a.out((M, N), F32, a.ld(N, 4))                 # planes in -> fp32 stream out
        ops.gemm_nt_ln_split(A, B, a.inp(h0, ldp), a.inp(l0, ldp), bias, mean, rstd, cs, x_out=x)
        return {"x": x}
    return fn


for _form in ("f32_in", "split", "f32_out"):
    for _M, _N, _K in [(131, 96, 192), (259, 160, 64)]:
        case(f"gemm_nt_ln_split.{_form}[{_M},{_N},{_K}]")(_split_case(_M, _N, _K, _form))


def _quant(x):
    M, K = x.shape
    q, s = torch.zeros(M, up(K, 128), dtype=torch.uint8), torch.empty(M)
    _ref.quant_rows_fp8(x, q, s)
    return q, s


def _quant_case(M, K):
    def fn(ops, a):                                        # clipself_hip.h:42: Kp = K rounded up to 128, padding zero -- part of the output view
        x = a.inp(rnd((M, K), BF, 2.0, seed=100), a.ld(K, 8))
        q, s = a.out((M, up(K, 128)), torch.uint8, a.ld(up(K, 128), 8)), a.out((M,), F32)
        ops.quant_rows_fp8(x, q, s)
        return {"q": q, "scale": s}
    return fn


def _f8_case(M, N, K, epi):
    def fn(ops, a):
        A8, sa = memo(("f8A", M, K), lambda: _quant(rnd((M, K), BF, 2.0, seed=101)))
        B8, sb = memo(("f8B", N, K), lambda: _quant(rnd((N, K), BF, 0.1, seed=102)))
        K8 = A8.shape[1]
        A, B = a.inp(A8, a.ld(K8, 16)), a.inp(B8, a.ld(K8, 16))
        sa, sb, bias = a.inp(sa), a.inp(sb), a.inp(rnd((N,), F32, seed=103))
        if epi == 0:
            C = a.out((M, N), BF, a.ld(N, 4))
            ops.gemm_nt_f8(A, B, C, sa, sb, bias, epi=0)
        else:
            C = a.out((M, N), F32, a.ld(N, 4), init=rnd((M, N), F32, seed=104))
            ops.gemm_nt_f8(A, B, C, sa, sb, bias, extra=C, epi=2)
        return {"C": C}
    return fn


for _M, _K in [(1, 64), (131, 192), (259, 64)]:
    case(f"quant_rows_fp8[{_M},{_K}]")(_quant_case(_M, _K))
for _M, _N, _K in [(1, 96, 64), (131, 96, 192), (259, 160, 64)]:
    for _epi in (0, 2):
        case(f"gemm_nt_f8.epi{_epi}[{_M},{_N},{_K}]")(_f8_case(_M, _N, _K, _epi))


def _wgrad_case(M, N, K):
    def fn(ops, a):                                        # clipself_hip.h:49-51: dW += A . B^T, contraction (tokens) zero padded to K % 64 == 0
        A = a.inp(rnd((M, K), BF, seed=60), a.ld(K, 8))
        B = a.inp(rnd((N, K), BF, seed=61), a.ld(K, 8))
        dW = a.out((M, N), F32, a.ld(N, 4), init=rnd((M, N), F32, seed=62))
        ops.gemm_wgrad(A, B, dW, a.ws(ops.gemm_wgrad_workspace(M, N, K)))
        return {"dW": dW}
    return fn


def _wgrad_tn_case(N, K, T):
    def fn(ops, a):                                        # token-major operands: the rows past `tokens` are halo (NaN)
        dY = a.inp(rnd((T, N), BF, seed=63), a.ld(N, 8))
        X = a.inp(rnd((T, K), BF, seed=64), a.ld(K, 8))
        dW = a.out((N, K), F32, a.ld(K, 4), init=rnd((N, K), F32, seed=65))
        ops.gemm_wgrad_tn(dY, X, dW, a.ws(ops.gemm_wgrad_tn_workspace(N, K, T)))
        return {"dW": dW}
    return fn


for _M, _N, _K in [(1, 96, 64), (131, 96, 192), (259, 160, 64)]:
    case(f"gemm_wgrad[{_M},{_N},{_K}]")(_wgrad_case(_M, _N, _K))
for _N, _K, _T in [(96, 64, 1), (96, 192, 131), (160, 64, 259)]:
    case(f"gemm_wgrad_tn[{_N},{_K},{_T}]")(_wgrad_tn_case(_N, _K, _T))


# ---- LayerNorm.  C = 132: a multiple of 4 whose last 256-column vector group is ragged; 2052: the same in the widest instantiation;
# 130: C % 4 != 0 -- clipself_hip.h (cs_layernorm_fwd / cs_layernorm_bwd): the pad columns of x, dy, gamma, beta are ignored and
# [C, roundup4(C)) of y, dx, dx_copy is written with zeros (zero_pad below); the compact run holds zeros there, the halo run NaN.
def _ln_inputs(a, M, C, xdt, seed=20):
    ld4 = lambda n: a.ld(up(C, 4), n)
    x = a.inp((rnd((M, C), F32, 2.0, seed=seed) + 0.5).to(xdt), ld4(4))
    # gamma / beta are fetched in 16-byte pieces and must be readable up to roundup4(C) (clipself_hip.h, cs_layernorm_fwd): one padded row
    gamma = a.inp(1 + rnd((1, C), F32, 0.2, seed=seed + 1), ld4(4))[0]
    beta = a.inp(rnd((1, C), F32, 0.2, seed=seed + 2), ld4(4))[0]
    return x, gamma, beta


def _ln_fwd_case(M, C, xdt, form):
    def fn(ops, a):
        x, gamma, beta = _ln_inputs(a, M, C, xdt)
        zp = up(C, 4) - C
        mean, rstd = a.out((M,), F32), a.out((M,), F32)
        outs = {"mean": mean, "rstd": rstd}
        if form == "stats":                                # y = NULL: statistics only
            ops.layernorm_fwd(x, gamma, beta, None, mean, rstd)
        elif form == "y":
            y = outs["y"] = a.out((M, C), BF, a.ld(up(C, 4), 4), zero_pad=zp)
            ops.layernorm_fwd(x, gamma, beta, y, mean, rstd)
        elif form == "y_nostats":
            y = a.out((M, C), BF, a.ld(up(C, 4), 4), zero_pad=zp)
            ops.layernorm_fwd(x, gamma, beta, y)
            return {"y": y}
        elif form == "q8":                                 # clipself_hip.h:99-100: q8 [M, >= C rounded up to 128], zero padding
            y = outs["y"] = a.out((M, C), BF, a.ld(up(C, 4), 4), zero_pad=zp)
            q8, qs = a.out((M, up(C, 128)), torch.uint8, a.ld(up(C, 128), 4)), a.out((M,), F32)
            ops.layernorm_fwd_q8(x, gamma, beta, y, q8, qs, mean, rstd)
            outs.update(q8=q8, q_scale=qs)
        else:
            assert form == "f32" and xdt == F32 and C % 4 == 0
            y = outs["y"] = a.out((M, C), F32, a.ld(C, 4))
            ops.layernorm_fwd_f32(x, gamma, beta, y, mean, rstd)
        return outs
    return fn


def _ln_stats(M, C, xdt, seed=20):
    def make():
        x = (rnd((M, C), F32, 2.0, seed=seed) + 0.5).to(xdt).double()
        mu = x.mean(-1)
        return mu.float(), torch.rsqrt(x.var(-1, unbiased=False) + 1e-6).float()
    return memo(("lnstats", M, C, xdt, seed), make)


def _ln_bwd_case(M, C, xdt, mode, form):
    def fn(ops, a):
        x, gamma, _ = _ln_inputs(a, M, C, xdt)
        Cp, zp = up(C, 4), up(C, 4) - C
        dy = a.inp(rnd((M, C), BF, seed=23), a.ld(Cp, 4))
        mean, rstd = _ln_stats(M, C, xdt)
        mean, rstd = a.inp(mean), a.inp(rstd)
        odt = BF if mode == 0 else F32
        dx = a.out((M, C), odt, a.ld(Cp, 4), init=rnd((M, C), F32, seed=24).to(odt) if mode == 2 else None, zero_pad=zp)
        ws = a.ws(ops.layernorm_bwd_workspace(M, C))
        outs = {"dx": dx}
        if form == "frozen":                               # no parameter gradients
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, mode)
            return outs
        dg, db = a.out((C,), F32, init=rnd((C,), F32, seed=27)), a.out((C,), F32, init=rnd((C,), F32, seed=28))
        outs.update(dgamma=dg, dbeta=db)
        if form == "params":
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, mode, dg, db, False, ws)
        elif form == "params_acc":
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, mode, dg, db, True, ws)
        else:
            cpy = outs["dx_copy"] = a.out((M, C), BF, a.ld(Cp, 4), zero_pad=zp)
            cs = outs["copy_colsum"] = a.out((C,), F32, init=rnd((C,), F32, seed=26))
            if form == "copy":
                ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, mode, dg, db, True, ws, dx_copy=cpy, copy_colsum=cs)
            elif form == "copy_only":                      # the copy without its column sums, frozen parameters
                del outs["copy_colsum"], outs["dgamma"], outs["dbeta"]
                ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, mode, dx_copy=cpy)
            else:
                assert form == "q8"                        # clipself_hip.h:117-118
                q8, qs = a.out((M, up(C, 128)), torch.uint8, a.ld(up(C, 128), 4)), a.out((M,), F32)
                ops.layernorm_bwd_q8(dy, x, gamma, mean, rstd, dx, mode, dg, db, True, ws, cpy, cs, q8, qs)
                outs.update(q8=q8, q_scale=qs)
        return outs
    return fn


_xn = {F32: "f32", BF: "bf16"}
for _M, _C in [(1, 132), (131, 132), (259, 130), (5, 2052), (5, 2730)]:
    for _xdt in (F32, BF):
        for _form in ("stats", "y", "y_nostats", "q8"):
            case(f"layernorm_fwd.{_form}[{_M},{_C},{_xn[_xdt]}]")(_ln_fwd_case(_M, _C, _xdt, _form))
    if _C % 4 == 0:
        case(f"layernorm_fwd_f32[{_M},{_C}]")(_ln_fwd_case(_M, _C, F32, "f32"))
for _M, _C in [(131, 132), (259, 130), (5, 2730)]:
    for _xdt in (F32, BF):
        for _mode in (0, 1, 2):
            for _form in ("frozen", "params", "params_acc") + (("copy", "copy_only", "q8") if _mode else ()):
                case(f"layernorm_bwd.dx{_mode}.{_form}[{_M},{_C},{_xn[_xdt]}]")(_ln_bwd_case(_M, _C, _xdt, _mode, _form))


def _finalize_case(M, P, npp, C):
    def fn(ops, a):
        part = a.inp(rnd((P, M, 2), F32, seed=110).abs() + 0.1)
        mean, rstd = a.out((M,), F32), a.out((M,), F32)
        ops.ln_stats_finalize(part, npp, C, mean, rstd, 1e-6)
        return {"mean": mean, "rstd": rstd}
    return fn


for _M in (1, 131, 258):                                   # odd / even M: the one-row and the two-rows-per-thread kernels
    for _P, _npp, _C in [(2, 64, 100), (12, 64, 768), (17, 32, 530)]:
        case(f"ln_stats_finalize[{_M},{_P},{_npp},{_C}]")(_finalize_case(_M, _P, _npp, _C))


def _l2_case(M, C):
    def fn(ops, a):
        x, dy = rnd((M, C), F32, seed=28), rnd((M, C), F32, seed=29)
        y, inv = a.out((M, C), F32), a.out((M,), F32)
        ops.l2norm_fwd(a.inp(x), y, inv)
        yr, ir = torch.empty(M, C), torch.empty(M)
        _ref.l2norm_fwd(x, yr, ir)
        dx = a.out((M, C), BF)
        ops.l2norm_bwd(a.inp(dy), a.inp(yr), a.inp(ir), dx)
        return {"y": y, "inv_norm": inv, "dx": dx}
    return fn


for _M, _C in [(1, 4), (131, 260)]:
    case(f"l2norm[{_M},{_C}]")(_l2_case(_M, _C))


# ---- attention: head dim 64, B = H = 2.  Ntok 17: the short-sequence forward and the one-chunk backward; 226: the 224-key-chunk kernels
# with one key in the second chunk.
def _rope(Ntok):
    from oracle.eva_ref import rope_tables
    return memo(("rope", Ntok), lambda: rope_tables(int(round((Ntok - 1) ** 0.5)), 64))


def _attn_data(B, Ntok, H):
    def make():
        C = H * 64
        qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=30)
        qkv[:, :2 * C] *= 2.0
        qkv = qkv.to(BF)
        cos, sin = _rope(Ntok)
        o, lse = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
        _ref.attn_fwd(qkv, cos, sin, o, lse, B, Ntok, H, 64 ** -0.5)
        return qkv, o, lse, rnd((B * Ntok, C), BF, seed=31)
    return memo(("attn", B, Ntok, H), make)


def _attn_case(B, Ntok, H, form):
    def fn(ops, a):
        C, scale = H * 64, 64 ** -0.5
        qkv0, o0, lse0, dout0 = _attn_data(B, Ntok, H)
        cos, sin = _rope(Ntok)
        qkv, cos, sin = a.inp(qkv0, a.ld(3 * C, 8)), a.inp(cos), a.inp(sin)
        if form == "bwd":
            ldo = a.ld(C, 8)
            dqkv = a.out((B * Ntok, 3 * C), BF, a.ld(3 * C, 8))
            ops.attn_bwd(qkv, a.inp(o0, ldo), a.inp(dout0, ldo), a.inp(lse0), cos, sin, dqkv, a.ws(ops.attn_bwd_workspace(B, Ntok, H)),
                         B, Ntok, H, scale)
            return {"dqkv": dqkv}
        out = a.out((B * Ntok, C), BF, a.ld(C, 8))
        if form == "fwd_nolse":
            ops.attn_fwd(qkv, cos, sin, out, None, B, Ntok, H, scale)
            return {"out": out}
        lse = a.out((B * H, Ntok), F32)
        if form == "fwd":
            ops.attn_fwd(qkv, cos, sin, out, lse, B, Ntok, H, scale)
            return {"out": out, "lse": lse}
        part = a.out((H, B * Ntok, 2), F32)
        ops.attn_fwd_stats(qkv, cos, sin, out, lse, part, B, Ntok, H, scale)
        return {"out": out, "lse": lse, "stats_part": part}
    return fn


for _Ntok in (17, 226):
    for _form in ("fwd", "fwd_nolse", "fwd_stats", "bwd"):
        case(f"attn_{_form}[2,{_Ntok},2]")(_attn_case(2, _Ntok, 2, _form))


def _attn_cls_case(B, Ntok, H):
    def fn(ops, a):
        C = H * 64
        cos, sin = _rope(Ntok)
        q = a.inp(rnd((B, C), BF, 2.0, seed=32), a.ld(C, 8))
        kv = a.inp(rnd((B * Ntok, 2 * C), BF, seed=33), a.ld(2 * C, 8))
        out = a.out((B, C), BF, a.ld(C, 8))
        ops.attn_cls_fwd(q, kv, a.inp(cos), a.inp(sin), out, B, Ntok, H, 64 ** -0.5)
        return {"out": out}
    return fn


def _attn_query_case(B, Q, Ntok, H):
    def fn(ops, a):
        C = H * 64
        q = a.inp(rnd((B * Q, C), BF, 2.0, seed=34), a.ld(C, 8))
        kv = a.inp(rnd((B * Ntok, 2 * C), BF, seed=35), a.ld(2 * C, 8))
        allow = (torch.rand(B * Q, Ntok, generator=torch.Generator().manual_seed(36)) < 0.6).to(torch.uint8)
        allow[:, 0] = 1
        allow[0, 1:] = 0                                   # a CLS-only row
        out = a.out((B * Q, C), BF, a.ld(C, 8))
        ops.attn_query_fwd(q, kv, a.inp(allow), out, B, Q, Ntok, H, 64 ** -0.5)
        return {"out": out}
    return fn


for _Ntok in (17, 226):
    case(f"attn_cls_fwd[3,{_Ntok},2]")(_attn_cls_case(3, _Ntok, 2))
    case(f"attn_query_fwd[2,3,{_Ntok},2]")(_attn_query_case(2, 3, _Ntok, 2))
case("attn_query_fwd[1,1,17,1]")(_attn_query_case(1, 1, 17, 1))


# ---- element-wise.  Hd / N = 72: a multiple of 8 (the 16-byte vectors) that fills no 64-lane group.
def _swiglu_case(M, Hd, form):
    def fn(ops, a):
        x12 = a.inp(rnd((M, 2 * Hd), BF, 2.0, seed=40), a.ld(2 * Hd, 8))
        if form == "fwd":
            h = a.out((M, Hd), BF, a.ld(Hd, 8))
            ops.swiglu_fwd(x12, h)
            return {"h": h}
        dh = a.inp(rnd((M, Hd), BF, seed=41), a.ld(Hd, 8))
        dx = a.out((M, 2 * Hd), BF, a.ld(2 * Hd, 8))
        outs = {"dx12": dx}
        if form == "bwd":
            ops.swiglu_bwd(dh, x12, dx)
        elif form == "bwd_colsum":
            cs = outs["colsum"] = a.out((2 * Hd,), F32, init=rnd((2 * Hd,), F32, seed=42))
            ops.swiglu_bwd_colsum(dh, x12, dx, cs, a.ws(ops.colsum_workspace(M, 2 * Hd)))
        else:                                              # clipself_hip.h:167-168: bytes [dx1 | dx2 | zero padding to a multiple of 128]
            Kp = up(2 * Hd, 128)
            q8, qs = a.out((M, Kp), torch.uint8, a.ld(Kp, 8)), a.out((M,), F32)
            ops.swiglu_bwd_q8(dh, x12, dx, q8, qs)
            outs.update(q8=q8, q_scale=qs)
        return outs
    return fn


def _gelu_case(M, N, quick):
    def fn(ops, a):
        x = a.inp(rnd((M, N), BF, 2.0, seed=90), a.ld(N, 8))
        dy = a.inp(rnd((M, N), BF, seed=91), a.ld(N, 8))
        y, dx = a.out((M, N), BF, a.ld(N, 8)), a.out((M, N), BF, a.ld(N, 8))
        ops.gelu_fwd(x, y, quick)
        ops.gelu_bwd(dy, x, dx, quick)
        return {"y": y, "dx": dx}
    return fn


for _M in (1, 131, 259):
    for _form in ("fwd", "bwd", "bwd_colsum", "bwd_q8"):
        case(f"swiglu_{_form}[{_M},72]")(_swiglu_case(_M, 72, _form))
    for _quick in (False, True):
        case(f"gelu[{_M},72,quick={int(_quick)}]")(_gelu_case(_M, 72, _quick))


def _transpose_case(shapes, batched):
    def fn(ops, a):                                        # clipself_hip.h:179: out[c, r], zero pad r in [R, ld_out) -- part of the (contiguous) output
        ins = [a.inp(rnd((R, Cc), BF, seed=43 + i), a.ld(Cc)) for i, (R, Cc) in enumerate(shapes)]
        outs = [a.out((Cc, up(R, 64)), BF) for R, Cc in shapes]
        if batched:
            ops.transpose_bf16_batched(list(zip(ins, outs)))
        else:
            for i, o in zip(ins, outs):
                ops.transpose_bf16(i, o)
        return {f"out{i}": o for i, o in enumerate(outs)}
    return fn


case("transpose_bf16[131,70]")(_transpose_case([(131, 70)], False))
case("transpose_bf16[1,96]")(_transpose_case([(1, 96)], False))
case("transpose_bf16[259,128]")(_transpose_case([(259, 128)], False))
case("transpose_bf16_batched")(_transpose_case([(131, 70), (1, 96), (259, 128)], True))


def _colsum_case(M, N, ldx=None):
    def fn(ops, a):
        x0 = rnd((M, N), BF, seed=44)
        base = rnd((N,), F32, seed=45)
        x = a.inp(x0, (ldx if a.poison else None) if ldx else a.ld(N))
        out = a.out((N,), F32, init=base)
        ops.colsum_bf16(x, out, a.ws(ops.colsum_workspace(M, N)))
        if ldx:
            # the kernel picks 16-byte loads from the alignment of ldx (elementwise.hip, `vec`): ldx = 770 runs every column group through
            # the scalar path, 776 the whole groups through the vector path and the ragged last one through the scalar path.  A different
            # path, not a different contract: both runs are held to the fp64 column sums at the bound of test_gpu_ops.py ("colsum", 1e-4)
            return {"out": Approx(out, base.double() + x0.double().sum(0), 1e-4)}
        return {"out": out}
    return fn


case("colsum_bf16[259,770,ldx=776]")(_colsum_case(259, 770, ldx=776))
for _M, _N in [(1, 72), (131, 72), (259, 520)]:
    case(f"colsum_bf16[{_M},{_N}]")(_colsum_case(_M, _N))


def _im2row_case(B, S, p, dt):
    def fn(ops, a):                                        # clipself_hip.h (cs_im2row): the whole row is written, [3*p*p, ldo) with zeros
        img = a.inp(rnd((B, 3, S, S), F32, seed=46).to(dt))
        kk = 3 * p * p                                     # p = 14: 588 -> 640; p = 16: no padding on the compact run (the 16-byte kernel)
        out = a.out((B * (S // p) ** 2, a.ld(up(kk, 64), 8)), BF)
        ops.im2row(img, out, p)
        return {"out": out[:, :kk], "nonzero_padding": (bits(out[:, kk:]) != 0).sum().reshape(1)}
    return fn


for _dt in (F32, BF):
    case(f"im2row[2,28,14,{_xn[_dt]}]")(_im2row_case(2, 28, 14, _dt))
    case(f"im2row[1,16,16,{_xn[_dt]}]")(_im2row_case(1, 16, 16, _dt))


def _cast_cls_case(fn_name):
    def fn(ops, a):
        if fn_name == "cast":
            y = a.out((8 * 131,), BF)
            ops.cast_f32_bf16(a.inp(rnd((8 * 131,), F32, seed=42)), y)
            return {"y": y}
        B, Ntok, C = 3, 5, 132
        x = a.out((B, Ntok, C), F32, init=rnd((B, Ntok, C), F32, seed=47))
        ops.cls_row(x, a.inp(rnd((C,), F32, seed=48)), a.inp(rnd((Ntok, C), F32, seed=49)))
        return {"x": x}
    return fn


case("cast_f32_bf16[1048]")(_cast_cls_case("cast"))
case("cls_row[3,5,132]")(_cast_cls_case("cls"))


# ---- RoIAlign / losses / AdamW / resampling: no row strides, front and back halo only
def _boxes(K, B, seed):
    g = torch.Generator().manual_seed(seed)
    xy0 = torch.rand(K, 2, generator=g) * 0.6
    xy1 = (xy0 + torch.rand(K, 2, generator=g) * 0.3 + 0.1).clamp(max=1.0)
    if K > 2:
        xy0[1], xy1[1] = torch.tensor([-0.2, 0.1]), torch.tensor([0.2, 0.5])       # crosses the border
        xy0[2], xy1[2] = torch.tensor([0.9, 0.9]), torch.tensor([1.2, 1.3])
    return torch.cat([torch.randint(0, B, (K, 1), generator=g).float(), xy0, xy1], dim=1)


def _roialign_case(B, K, grid, E):
    def fn(ops, a):
        Ntok = grid * grid + 1
        rois = a.inp(_boxes(K, B, 51))
        pooled = a.out((K, E), F32)
        ops.roialign_fwd(a.inp(rnd((B, Ntok, E), F32, seed=50)), rois, pooled, grid, grid, 1)
        dfeat = a.out((B, Ntok, E), F32, init=rnd((B, Ntok, E), F32, seed=53))
        ops.roialign_bwd(a.inp(rnd((K, E), F32, seed=52)), rois, dfeat, grid, grid, 1)
        return {"pooled": pooled, "dfeat": dfeat}
    return fn


case("roialign[1,1,2,4]")(_roialign_case(1, 1, 2, 4))
case("roialign[3,7,5,1028]")(_roialign_case(3, 7, 5, 1028))                            # wider than one workgroup's 1024 channels


def _cosine_case(K, E):
    def fn(ops, a):
        s, t = a.inp(rnd((K, E), F32, 0.3, seed=60)), a.inp(rnd((K, E), F32, 2.0, seed=61))
        stats, loss, ds = a.out((K, 3), F32), a.out((1,), F32), a.out((K, E), F32)
        ops.cosine_loss_fwd(s, t, stats, loss, 1.0)
        sr, lr = torch.empty(K, 3), torch.empty(1)
        _ref.cosine_loss_fwd(rnd((K, E), F32, 0.3, seed=60), rnd((K, E), F32, 2.0, seed=61), sr, lr, 1.0)
        ops.cosine_loss_bwd(s, t, a.inp(sr), ds, 1.0, 1.0, a.inp(torch.tensor([0.7])))
        return {"stats": stats, "loss": loss, "dstudent": ds}
    return fn


case("cosine_loss[1,4]")(_cosine_case(1, 4))
case("cosine_loss[131,260]")(_cosine_case(131, 260))


def _fed_bce_case(K, ns):
    def fn(ops, a):                                        # clipself_hip.h (cs_fed_bce_bwd): the whole row [K, ldd] is written, [ns, ldd) with zeros
        W = a.ld(up(ns, 8) + 8)
        logits = a.inp(rnd((K, ns), F32, 3.0, seed=80), a.ld(ns))
        tgt = a.inp(torch.randint(-1, ns, (K,), generator=torch.Generator().manual_seed(81)).to(torch.int32))
        rl, loss = a.out((K,), F32), a.out((1,), F32)
        ops.fed_bce_fwd(logits, tgt, rl, loss, ns, 14.3, 1.0)
        dz = a.out((K, W), BF)
        ops.fed_bce_bwd(logits, tgt, dz, ns, 14.3, 1.0, a.inp(torch.tensor([0.7])))
        return {"rowloss": rl, "loss": loss, "dz": dz[:, :ns], "nonzero_padding": (bits(dz[:, ns:]) != 0).sum().reshape(1)}
    return fn


case("fed_bce[1,1]")(_fed_bce_case(1, 1))
case("fed_bce[131,100]")(_fed_bce_case(131, 100))


def _adamw_case(n):
    def fn(ops, a):
        flags = torch.tensor([3, 1, 0, 2, 1, 0, 3, 3] * (n // 512), dtype=torch.uint8)[:n // 64]
        p, m, v = (a.out((n,), F32, init=rnd((n,), F32, s, seed=70 + i)) for i, s in enumerate((0.02, 1e-3, 1e-3)))
        v.abs_()
        sh = a.out((n,), BF, init=torch.zeros(n, dtype=BF))
        ops.adamw_step(p, a.inp(rnd((n,), F32, 1e-3, seed=74)), m, v, sh, a.inp(flags), 1e-3, 0.9, 0.999, 1e-8, 0.1, 2)
        return {"p": p, "m": m, "v": v, "shadow": sh}
    return fn


case("adamw_step[512]")(_adamw_case(512))
case("adamw_step[1536]")(_adamw_case(1536))


def _resize_case(shape, size):
    def fn(ops, a):                                        # the wrapper allocates the output itself: only the input sits in a halo
        return {"out": ops.resize_bilinear(a.inp(rnd(shape, F32, seed=120)), size)}
    return fn


def _crop_case(H, W, K, S):
    def fn(ops, a):                                        # the workspace belongs to the wrapper; image, boxes and output sit in halos
        g = torch.Generator().manual_seed(121)
        img = a.inp(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
        xy0 = torch.rand(K, 2, generator=g) * torch.tensor([W * 0.5, H * 0.5])
        boxes = torch.cat([xy0, xy0 + 8 + torch.rand(K, 2, generator=g) * torch.tensor([W * 0.4, H * 0.4])], dim=1).round()
        out = a.out((K, 3, S, S), F32)
        ops.crop_resize(img, a.inp(boxes), S, True, out=out)
        return {"out": out}
    return fn


case("resize_bilinear_f32[1,1,1,1->3]")(_resize_case((1, 1, 1, 1), 3))
case("resize_bilinear_f32[2,3,9,9->14]")(_resize_case((2, 3, 9, 9), 14))
case("crop_resize_u8[37,53,1,16]")(_crop_case(37, 53, 1, 16))
case("crop_resize_u8[64,48,5,24]")(_crop_case(64, 48, 5, 24))
