"""TEST INFRASTRUCTURE -- attention operands with known answers (tests/test_attn_exact_cpu.py, tests/test_gpu_attn_exact.py).

The relative-L2 checks of the attention kernels pass a defect that is confined to a few rows.  The cases built here have answers that follow
from index arithmetic on integer scores, so that every element of o, every lse and every gradient element can be compared on its own:

  needle   rotated key j = 8 * code(j), rotated query i = the key vector of pi(i): one probability is 1, every other one exactly 0.
           o[i] = v[pi(i)] bit for bit, lse = 8 * 8 * 64 / 8 = 512, dV[j] = dout[pi^-1(j)], dQ = dK = 0 by value.
  tied     keys j and j + N // 2 share a 32-dim code (amp 16), the other 32 dims of k are free and zero in q: p in {0, 1/2, 1},
           o = (v_a + v_b) / 2, lse = 1024 + ln 2, and a backward that is non-trivial and exact (dS_a = -dS_b = dout . (v_a - v_b) / 32).
  uniform  q = 0: p = 1 / N for every key, lse = ln N, o = colsum(v) / N, dK = 0, dV = bf16(bf16(1 / N) * sum_i dout_i).
  allow / causal / CLS variants of needle and tied: the query is 8 * (2 code(a) + code(b)) with b the nearest neighbour of a among the keys
           the row may see, so that b wins exactly when a is masked or lies in the future.

All operands are small integers, exact in bf16; the scale is 64 ** -0.5 = 2 ** -3.  The expected values are gathers and products with a
probability matrix whose entries are written down, not computed by a softmax (hard_attention / hard_backward): independent of
oracle/ops_ref.RefOps.  The rotary tables are quarter turns (cos, sin in {0, 1, -1}), so that a rotation is a signed permutation, exact in
bf16; the inputs are the wanted rotated rows with the inverse rotation applied in advance, and a wrong table row or token position
yields a different code vector.

Exactness assumptions (asserted where they can be, reasoned from the kernels' rounding points otherwise):
 A1  the scaled score gap between the winners and every other visible key is >= GAP = 104: exp(-104) = 6.8e-46 is below the smallest fp32
     denormal, so every other probability is exactly 0 and the online-softmax rescale of an earlier chunk (alpha = exp2((m - m_new) sl2))
     is exactly 0 or exactly 1.  Asserted in hard_attention.
 A2  a winner's exponent is 0 up to the rounding of m * sl2 (sl2 = scale * log2 e): the forward computes exp2(s * sl2 - fl(m * sl2)), where
     the compiler may contract the product and the difference into one FMA; the residue is at most ulp(m * sl2) / 2 <= 6.1e-5 at the scores
     used here, so the winner's p is within 5e-5 of 1.  Rounded to bf16 (unit roundoff 2^-8) for P.V it is exactly 1; the fp32 row sum l
     carries the residue, and o = (P.V) * (1 / l) is within 1e-4 relative of a value that has at most 5 significant bits, so its rounding to
     bf16 returns that value.  The backward computes exp2(fma(s, sl2, -lse * log2 e)): within 2e-4 of 1 or 1/2, which rounds to 1 or 1/2
     in bf16, and dS = bf16(p * (dP * scale - D * scale)) is within 2e-4 relative of a value with at most 6 significant bits (asserted
     representable in hard_backward), so its rounding is exact.
 A3  every fp32 sum (P.V, dS.K, dS^T.Q, P^T.dO, dO.O) is exact in any order: all terms are multiples of one power of two and their absolute
     sum stays below 2^24 of it.  Asserted in hard_attention / hard_backward.
 A4  uniform case: exp2(-fl(fl(ln N) * log2 e)) is within DELTA_P(N) of 1 / N (below) and N is rejected when 1 / N lies within 1e-5 relative
     of a bf16 rounding tie, so the bf16 probability of the dV product is bf16(1 / N).

lse bounds, in fp32 ulps of |lse| (ulp32): the image forward writes m * scale + logf(l).
   m * scale        exact: m is an integer below 2^24, the scale a power of two                                   0
   rounding of m*sl2 the residue of A2 reaches l and logf(l) as at most ulp(m sl2) / 2 * ln 2 <= 2^-24 |lse|        < 1
   logf             <= 1 ulp of its result, which is |lse| itself in the uniform case (m = 0) and below 1 otherwise  <= 1
   final add        one rounding                                                                                  <= 1/2
 LSE_ULPS_IMAGE = 3.  The query kernel (cs_attn_query_fwd) writes (fl(dot * sl2) + log2(sum)) * fl(1 / log2e_f): the product dot * sl2, the
 add, the constant 1 / log2e_f and the final product are one rounding of 2^-24 relative each (the rounding of log2 e itself cancels between
 sl2 and its reciprocal in the leading term); log2(sum) is log2 of 1 or 2, and its share of |lse| is below 1e-3: 4 * 2^-24 |lse| <= 4 ulps,
 LSE_ULPS_QUERY = 5.  A dropped or duplicated key moves lse by >= ln(3/2) (tied) or >= 1 / N (uniform): >= 1e4 ulps at every size used."""
import math
from types import SimpleNamespace

import torch

from oracle.ops_ref import _rope_rows

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SCALE = 64 ** -0.5
GAP = 104.0
LSE_ULPS_IMAGE, LSE_ULPS_QUERY = 3.0, 5.0
U = 2.0 ** -24                                                     # fp32 unit roundoff
UB = 2.0 ** -8                                                     # bf16 unit roundoff
KINDS = ("needle", "tied_lo", "tied_hi", "uniform")
TABLES = ("quarter", "ident", "null")
# (B, Ntok, H) of the image kernels: the smallest token counts that reach each kernel form (tests/test_gpu_attn_norope.py lists them); 785 has
# a first, middle and ragged last key chunk and a tile riding on a split block.  NON_SQUARE: no grid, NULL tables only.
IMAGE_SQUARE = [(3, 17, 2), (2, 65, 2), (2, 170, 2), (2, 197, 2), (2, 226, 2), (1, 257, 3), (1, 401, 2), (1, 785, 2)]
IMAGE_NON_SQUARE = [2, 100, 200, 224, 225, 250, 449]
# (Ntok, H) of cs_attn_cls_fwd: every HG instantiation attn_cls_launch can choose (H % 6 == 0: 6, % 4: 4, % 3: 3, % 2: 2, else 1)
CLS_SHAPES = [(17, 1), (65, 2), (197, 3), (197, 4), (197, 6), (50, 5)]
QUERY_SHAPES = [(2, 1, 17, 2), (4, 3, 65, 4), (2, 5, 197, 2)]      # (B, Q, Ntok, H)
# (B, L, H) of tests/test_gpu_text.py: every attn_causal_kernel instantiation, every 32-row tile boundary and packing remainder
CAUSAL_SHAPES = [(1, 1, 1), (2, 2, 2), (3, 31, 2), (3, 32, 8), (2, 33, 12), (5, 64, 8), (2, 65, 2), (3, 77, 8), (2, 77, 12), (1, 96, 2), (1, 97, 2),
                 (2, 128, 2)]
PASSENGER_SHAPES = [(2, Q, N, 2) for N in (65, 197) for Q in (1, 5)]   # (B, Q, Ntok, H)


# ------------------------------------------------------------------------------------------------ tables and codes
def quarter_tables(g):
    """[g*g, 64] cos / sin of angle ((i + 1) * (f + 1)) % 4 quarter turns for grid index i and frequency f < 16, in the layout
    HipOps._check_rope_tables accepts: dims [0, 32) of token (r, c) follow r, dims [32, 64) follow c, one entry per rotation pair."""
    i, f = torch.arange(g)[:, None], torch.arange(16)[None, :]
    qt = ((i + 1) * (f + 1)) % 4
    cr = torch.tensor([1.0, 0.0, -1.0, 0.0])[qt].repeat_interleave(2, 1)
    sr = torch.tensor([0.0, 1.0, 0.0, -1.0])[qt].repeat_interleave(2, 1)
    lay = lambda t: torch.cat([t[:, None, :].expand(g, g, 32), t[None, :, :].expand(g, g, 32)], -1).reshape(g * g, 64).contiguous()
    return lay(cr), lay(sr)


def is_square(Ntok):
    g = int(round((Ntok - 1) ** 0.5))
    return g * g == Ntok - 1 and g > 0


def make_tables(kind, Ntok):
    """-> (cos, sin) that the kernel is given: quarter turns, identity, or (None, None)."""
    if kind == "null":
        return None, None
    assert is_square(Ntok), "tables need a square grid + 1 tokens"
    if kind == "ident":
        return torch.ones(Ntok - 1, 64), torch.zeros(Ntok - 1, 64)
    return quarter_tables(int(round((Ntok - 1) ** 0.5)))


def unrotate(t, cos, sin):
    """[..., N, 64] float64 rows in the rotated frame -> the rows whose rotation they are (also: the gradient w.r.t. the un-rotated rows)."""
    return t if cos is None else _rope_rows(t, cos.double(), sin.double(), inverse=True)


def codes(n, dims, amp):
    """[n, dims] float64 of +-amp: the bits of j repeated dims // (nbits + 1) times, the parity of j filling the rest."""
    nb = max(1, (n - 1).bit_length())
    rep = dims // (nb + 1)
    idx = torch.arange(n)
    bits = torch.stack([(idx >> b) & 1 for b in range(nb)], 1)
    par = bits.sum(1, keepdim=True) % 2
    c = torch.cat([bits.repeat(1, rep), par.repeat(1, dims - nb * rep)], 1)
    return (1 - 2 * c).double() * amp


def _ints(gen, shape, hi):
    """seeded integers in +-{1..hi} as float64"""
    return (torch.randint(1, hi + 1, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).double()


def _one_hot_dout(gen, B, H, rows):
    """one non-zero small integer (+-{1..4}) per row, at a seeded dim"""
    d = torch.zeros(B, H, rows, 64, dtype=F64)
    d.scatter_(-1, torch.randint(0, 64, (B, H, rows, 1), generator=gen), _ints(gen, (B, H, rows, 1), 4))
    return d


def to_bf16_exact(t, what):
    r = t.to(F32).to(BF)
    assert torch.equal(r.double(), t.double()), f"{what}: not representable in bf16"
    return r


def rows_of(t):
    """[B, H, N, 64] -> [B*N, H*64]"""
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * 64)


def heads_of(t, B, N, H):
    """[B*N, >= H*64] -> [B, H, N, 64] float64"""
    return t[:, :H * 64].double().reshape(B, N, H, 64).permute(0, 2, 1, 3)


def _sum_exact(a_abs, b_abs, quantum, what):
    """A3: every term of a @ b is a multiple of `quantum`; partial sums in any order stay below 2^24 * quantum."""
    worst = float((a_abs @ b_abs).max()) if a_abs.numel() and b_abs.numel() else 0.0
    assert worst <= 2.0 ** 24 * quantum, f"{what}: an fp32 sum may round (|terms| sum to {worst}, quantum {quantum})"


# ------------------------------------------------------------------------------------------------ expected values by index arithmetic
def hard_attention(q, k, v, allowed=None):
    """q [B,H,Q,64], k / v [B,H,N,64] float64 integers (rotated frame), allowed bool broadcastable to [B,H,Q,N] (None: every key).
    The raw scores q.k are exact integers; a row's winners are its visible keys with the highest score.  Asserts A1 (one or two winners,
    every other visible key >= GAP below after scaling) and A3, and returns P in {0, 1/2, 1}, o = P v, lse = top * scale + ln(winners)
    (+inf and o = 0 for a row that sees no key, the kernel's documented answer) -- no exponential is evaluated."""
    S = q @ k.transpose(-1, -2)
    assert float(S.abs().max()) < 2.0 ** 24 and torch.equal(S, S.round())
    vis = torch.ones_like(S, dtype=torch.bool) if allowed is None else allowed.expand_as(S)
    Sm = S.masked_fill(~vis, float("-inf"))
    top = Sm.max(-1, keepdim=True).values
    win = vis & (Sm == top)
    cnt = win.sum(-1, keepdim=True)
    rest = Sm.masked_fill(win, float("-inf")).max(-1, keepdim=True).values
    live = cnt > 0
    gap = ((top - rest) * SCALE)[live]
    assert int(cnt.max()) <= 2, "more than two keys tie for a row's maximum"
    assert gap.numel() == 0 or float(gap.min()) >= GAP, f"A1: score gap {float(gap.min())} < {GAP}"
    P = win.double() / cnt.clamp_min(1)
    _sum_exact(P, v.abs(), 0.5, "P.V")
    o = P @ v
    lse = torch.where(live, top * SCALE + torch.log(cnt.clamp_min(1).double()), torch.full_like(top, float("inf")))[..., 0]
    return SimpleNamespace(P=P, o=o, lse=lse, cnt=cnt[..., 0], gap=float(gap.min()) if gap.numel() else float("inf"))


def hard_backward(P, q, k, v, o, dout, exact=True):
    """Backward of o = P v with P = softmax(scale q k^T) at the given P: dV = P^T dO, dS = P (dO V^T - rowsum(dO o)) scale, dQ = dS K,
    dK = dS^T Q, all in float64 (rotated frame).  exact: asserts that every dS is representable in bf16 (A2) and every sum exact (A3)."""
    dP = dout @ v.transpose(-1, -2)
    D = (dout * o).sum(-1, keepdim=True)
    dS = P * (dP - D) * SCALE
    if exact:
        assert torch.equal(dS.to(F32).to(BF).double(), dS), "A2: a dS is not representable in bf16"
        _sum_exact(dout.abs(), (v.abs()).transpose(-1, -2), 1.0, "dO.V^T")
        _sum_exact(dout.abs(), o.abs().transpose(-1, -2), 0.5, "dO.O")
        _sum_exact(dS.abs(), k.abs(), 2.0 ** -5, "dS.K")
        _sum_exact(dS.abs().transpose(-1, -2), q.abs(), 2.0 ** -5, "dS^T.Q")
        _sum_exact(P.transpose(-1, -2), dout.abs(), 0.5, "P^T.dO")
    return dS @ k, dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ dout, dS


# ------------------------------------------------------------------------------------------------ the uniform case's bounds
def delta_p(N):
    """A4: relative error of the backward's p = exp2(-fl(fl(ln N) * log2e_f)) against 1 / N.  The argument carries three roundings of
    2^-24 relative (ln N to fp32, the constant, the product) on a magnitude of log2 N, i.e. 3 * 2^-24 * log2 N absolute, times ln 2 in the
    result; v_exp_f32 adds 1 ulp = 2 * 2^-24."""
    return (3.0 * math.log(2.0) * max(math.log2(N), 1.0) + 2.0) * U


def check_uniform_N(N):
    """Rejects an N whose 1 / N lies within 1e-5 relative of a bf16 rounding tie (A4)."""
    assert delta_p(N) < 1e-5
    x = 1.0 / N
    e = math.floor(math.log2(x))
    ulp = 2.0 ** (e - 7)
    frac = (x / ulp) % 1.0                                          # position between two bf16 neighbours; a tie is 0.5
    assert abs(frac - 0.5) * ulp / x > 1e-5, f"uniform case: 1 / {N} is within 1e-5 of a bf16 rounding tie"
    return float(torch.tensor(x, dtype=F32).to(BF))


def ulp_bf16(x):
    """spacing of bf16 at |x| (float64 tensor); 0 at 0"""
    ax = x.abs()
    e = torch.floor(torch.log2(ax.clamp_min(2.0 ** -126)))
    return torch.where(ax > 0, torch.exp2(e - 7), torch.zeros_like(ax))


def ulp_f32(x):
    ax = x.abs().double()
    return torch.exp2(torch.floor(torch.log2(ax.clamp_min(2.0 ** -126))) - 23)


def uniform_o_bound(o64):
    """|o - colsum(v) / N| <= ulp_bf16 / 2 + 4 * 2^-24 |x|: the accumulators hold colsum(v) exactly (A3), the reciprocal of l = N and the
    product are fp32 operations (<= 3 * 2^-24 relative together, taken as 4), then one rounding to bf16."""
    return 0.5 * ulp_bf16(o64) + 4.0 * U * o64.abs()


def uniform_dq_bound(N, k, v, o_given, dout):
    """Per-element bound of the uniform case's dQ (rotated frame) against the float64 value at p = 1 / N exactly,
        dQ64[i] = sum_j dS64[i,j] k[j],   dS64[i,j] = (dO_i . v_j - D_i) * scale / N,   D_i = dO_i . o_i  (o as given to the kernel, bf16),
    derived from the kernel's rounding points (attn_bwd_dq2_kernel; the passenger and round-1 kernels round at the same places):
      D_i     an fp32 sum of 64 exact products in some order: |dD_i| <= 63 * 2^-24 * sum_d |dO_id o_id|  (the standard gamma_63 bound);
      dP_ij   an fp32 MFMA sum of small integers: exact (A3);
      x_ij    = fma(dP, scale, -D * scale): one rounding, 2^-24 relative;  p * x: one more;
      p       within delta_p(N) of 1 / N;
      dS      = bf16(p * x): unit roundoff 2^-8 relative.
      => dS_ij = dS64_ij (1 + e), |e| <= r = (2^-8 + delta_p + 2 * 2^-24) (1 + 2^-7), plus |dD_i| * scale / N * (1 + 2^-7) absolute;
      dQ      an fp32 MFMA sum of N (+ the tile's padding) products dS * k, each exact in fp32 (8 x 8 significant bits): at most two roundings
              per added term, (N + 64) * 2^-23 relative to sum_j |dS_ij k_jd|;
      the inverse rotation with quarter-turn or identity tables is a signed permutation (exact); the result is rounded to bf16 once.
    bound[i,d] = E + ulp_bf16(|dQ64| + E) / 2 with
      E[i,d] = sum_j |dS64_ij| |k_jd| (r + (N + 64) 2^-23) + |dD_i| scale / N (1 + 2^-7) sum_j |k_jd|."""
    dP = dout @ v.transpose(-1, -2)
    D = (dout * o_given).sum(-1, keepdim=True)
    dS = (dP - D) * SCALE / N
    dq64 = dS @ k
    dD = 63.0 * U * (dout * o_given).abs().sum(-1, keepdim=True)
    r = (UB + delta_p(N) + 2.0 * U) * (1.0 + 2.0 ** -7)
    E = (dS.abs() @ k.abs()) * (r + (N + 64) * 2.0 * U) + dD * SCALE / N * (1.0 + 2.0 ** -7) * k.abs().sum(-2, keepdim=True)
    return dq64, E + 0.5 * ulp_bf16(dq64.abs() + E), dS


# ------------------------------------------------------------------------------------------------ image-token cases
_CASES = {}


def image_case(kind, B, N, H, seed=0):
    """The case in the rotated frame (float64 [B, H, N, 64] each): q, k, v, dout and the expected P, o, lse, dq, dk, dv.  Memoised."""
    key = (kind, B, N, H, seed)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(1000 * seed + 7 * N + KINDS.index(kind))
    q, k = torch.zeros(B, H, N, 64, dtype=F64), torch.zeros(B, H, N, 64, dtype=F64)
    c = SimpleNamespace(kind=kind, B=B, N=N, H=H, exact=kind != "uniform")
    if kind == "needle":
        code = codes(N, 64, 8.0)
        c.pi = torch.stack([torch.stack([torch.randperm(N, generator=gen) for _ in range(H)]) for _ in range(B)])      # [B,H,N]
        k[:] = code
        q = torch.gather(k, 2, c.pi[..., None].expand(B, H, N, 64))
        v = _ints(gen, (B, H, N, 64), 8)
        dout = _one_hot_dout(gen, B, H, N)
    elif kind in ("tied_lo", "tied_hi"):
        M = N // 2
        G = M + (N - 2 * M)
        gid = torch.cat([torch.arange(M), torch.arange(M), torch.arange(M, G)])
        code = codes(G, 32, 16.0)
        cd, fr = (slice(0, 32), slice(32, 64)) if kind == "tied_lo" else (slice(32, 64), slice(0, 32))
        c.t = torch.stack([torch.stack([torch.randperm(N, generator=gen) % G for _ in range(H)]) for _ in range(B)])
        c.gid, c.M = gid, M
        k[..., cd] = code[gid]
        k[..., fr] = _ints(gen, (B, H, N, 32), 4)
        q[..., cd] = code[c.t]
        v = _ints(gen, (B, H, N, 64), 7)
        dout = _one_hot_dout(gen, B, H, N)
    else:
        assert kind == "uniform"
        c.pN = check_uniform_N(N)
        k = _ints(gen, (B, H, N, 64), 4)
        v = _ints(gen, (B, H, N, 64), 8)
        dout = _ints(gen, (B, H, N, 64), 4)
    c.q, c.k, c.v, c.dout = q, k, v, dout
    if c.exact:
        h = hard_attention(q, k, v)
        c.P, c.o, c.lse, c.gap = h.P, h.o, h.lse, h.gap
        c.o_bound = None
        c.dq, c.dk, c.dv, c.dS = hard_backward(c.P, q, k, v, c.o, dout)
        c.dq_bound = None
    else:
        c.P = torch.full((B, H, N, N), 1.0 / N, dtype=F64)
        c.o = v.sum(-2, keepdim=True).expand(B, H, N, 64) / N
        _sum_exact(torch.ones(1, N, dtype=F64), v.abs(), 1.0, "colsum(v)")
        c.lse = torch.full((B, H, N), math.log(N), dtype=F64)
        c.gap = float("inf")
        c.o_bound = uniform_o_bound(c.o)
        c.o_given = c.o.to(F32).to(BF).double()                     # what the backward is fed: the expected o rounded once
        c.dq, c.dq_bound, c.dS = uniform_dq_bound(N, k, v, c.o_given, dout)
        c.dk = torch.zeros_like(k)
        colsum = dout.sum(-2, keepdim=True).expand(B, H, N, 64)
        _sum_exact(torch.ones(1, N, dtype=F64), dout.abs(), 1.0, "colsum(dout)")
        assert float(dout.abs().sum(-2).max()) < 2.0 ** 16           # bf16(1/N) (8 bits) times the sum (< 16 bits): exact in fp32
        c.dv = (c.pN * colsum).to(F32).to(BF).double()              # bf16(bf16(1 / N) * sum_i dout_i)
    _CASES[key] = c
    return c


def image_inputs(c, tables):
    """The kernel-side tensors of a case for one table kind (CPU): qkv bf16 [B*N, 3C] (the rotated rows un-rotated in advance), cos / sin as
    given to the kernel, dout, the o / lse the backward is fed, and the expected d(q|k|v) in the un-rotated frame (float64, plus the bound of
    the uniform dQ in that frame: a signed permutation of the rotated frame's)."""
    B, N, H = c.B, c.N, c.H
    cos, sin = make_tables(tables, N)
    un = lambda t: unrotate(t, cos, sin)
    qkv = torch.cat([rows_of(un(c.q)), rows_of(un(c.k)), rows_of(c.v)], 1)
    o_in = c.o if c.exact else c.o_given
    want = torch.cat([rows_of(un(c.dq)), rows_of(un(c.dk)), rows_of(c.dv)], 1)
    inp = SimpleNamespace(case=c, tables=tables, cos=cos, sin=sin, qkv=to_bf16_exact(qkv, "qkv"), dout=to_bf16_exact(rows_of(c.dout), "dout"),
                          o_in=to_bf16_exact(rows_of(o_in), "o"), lse_in=c.lse.reshape(B * H, N).to(F32), want_dqkv=want,
                          dq_bound=None if c.exact else rows_of(un(c.dq_bound).abs()))
    return inp


# ------------------------------------------------------------------------------------------------ checks (return problems, never raise)
def _bad_rows(name, bad):
    rows = torch.nonzero(bad.reshape(bad.shape[0], -1).any(-1))[:, 0].tolist()
    return f"{name}: {int(bad.sum())} elements in {len(rows)} rows differ, first rows {rows[:6]}"


def check_exact(name, got, want64, problems):
    """every element equal by value to the float64 expectation rounded once to bf16 (-0.0 == +0.0), no NaN"""
    g = got.detach().cpu().double()
    w = want64.to(F32).to(BF).double()
    bad = ~(g == w)
    if bool(bad.any()):
        problems.append(_bad_rows(name, bad))


def check_bound(name, got, want64, bound, problems):
    """|got - want| <= bound per element; -> the worst |error| / bound (the share of the bound that is used)"""
    err = (got.detach().cpu().double() - want64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        problems.append(_bad_rows(name, bad) + f", worst |error| / bound {float((err / bound.clamp_min(1e-300))[bad].max()):.3g}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def check_lse(name, got, want64, ulps, problems):
    """|got - want| <= ulps * ulp32(|want|); +inf must be +inf.  -> the worst error in ulps"""
    g, w = got.detach().cpu().double().reshape(-1), want64.double().reshape(-1)
    inf = torch.isinf(w)
    if not torch.equal(torch.isinf(g) & (g > 0), inf):
        problems.append(f"{name}: +inf exactly for the rows that see no key")
    err = ((g - w).abs() / ulp_f32(w))[~inf]
    bad = ~(err <= ulps)
    if bool(bad.any()):
        problems.append(f"{name}: {int(bad.sum())} rows off by more than {ulps} ulps, worst {float(err[bad].max()):.3g}, first {torch.nonzero(bad)[:6, 0].tolist()}")
    seen = err[~torch.isnan(err)]
    return float(seen.max()) if seen.numel() else 0.0


def check_image_forward(tag, inp, o, lse, problems, stats_part=None):
    """o [B*N, C] bf16 and lse [B*H, N] f32 of cs_attn_fwd on `inp`; stats_part [H, B*N, 2] of cs_attn_fwd_stats.  -> metrics"""
    c = inp.case
    want_o = rows_of(c.o)
    m = {}
    if c.exact:
        check_exact(tag + ".o", o, want_o, problems)
    else:
        m["o_share"] = check_bound(tag + ".o", o, want_o, rows_of(c.o_bound), problems)
    if lse is not None:
        m["lse_ulps"] = check_lse(tag + ".lse", lse, c.lse.reshape(c.B * c.H, c.N), LSE_ULPS_IMAGE, problems)
    if stats_part is not None:
        sp = stats_part.detach().cpu().double()
        if c.exact:                                                 # sums of 64 half-integers and of their squares: exact in any order
            ob = want_o.reshape(c.B * c.N, c.H, 64)
            want = torch.stack([ob.sum(-1).T, (ob * ob).sum(-1).T], -1)
            if not bool((sp == want).all()):
                problems.append(_bad_rows(tag + ".stats_part", ~(sp == want).reshape(c.H * c.B * c.N, 2)))
        else:                                                       # of the kernel's own rounded rows: fp32 sums of 64 terms in some order
            ob = o.detach().cpu().double().reshape(c.B * c.N, c.H, 64)
            want = torch.stack([ob.sum(-1).T, (ob * ob).sum(-1).T], -1)
            bound = 64.0 * U * torch.stack([ob.abs().sum(-1).T, (ob * ob).sum(-1).T], -1)
            check_bound(tag + ".stats_part", sp, want, bound, problems)
    return m


def check_image_backward(tag, inp, dqkv, problems):
    c = inp.case
    C = c.H * 64
    m = {}
    if c.exact:
        for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
            check_exact(f"{tag}.{name}", dqkv[:, sl], inp.want_dqkv[:, sl], problems)
    else:
        m["dq_share"] = check_bound(tag + ".dq", dqkv[:, :C], inp.want_dqkv[:, :C], inp.dq_bound, problems)
        check_exact(tag + ".dk", dqkv[:, C:2 * C], inp.want_dqkv[:, C:2 * C], problems)
        check_exact(tag + ".dv", dqkv[:, 2 * C:3 * C], inp.want_dqkv[:, 2 * C:3 * C], problems)
    return m


# ------------------------------------------------------------------------------------------------ query rows: CLS, allow masks, causal, passengers
def _nearest(code, a, among):
    """the key of `among` (a bool mask over keys, a excluded) whose code is nearest to key a's (first of the nearest)"""
    d = (code != code[a]).sum(-1).double()
    d[~among] = float("inf")
    d[a] = float("inf")
    return int(torch.argmin(d))


def two_level(code, a, b):
    """query 8 * (2 code(a) + code(b)) against keys 8 * code(j), code in +-1: key a wins by 16 * d(a, b) after scaling; with a invisible,
    b wins by >= 16 * d(b, j) over every visible j when no visible key is nearer to a than b is.  Entries +-8 / +-24: exact in bf16."""
    return 8.0 * (2.0 * code[a] + code[b])


def cls_case(kind, Ntok, H, seed=0):
    """One image per probe: the CLS query of image b, head h targets a key chosen so that over the images the hit lands in every 32-key pass of
    attn_cls_kernel and on the last key.  kind: needle | tied_lo | tied_hi.  -> keys / values of image_case, q [B,H,1,64], expected o."""
    hits = sorted({min(32 * p + (7 * p + 3) % 32, Ntok - 1) for p in range((Ntok + 31) // 32)} | {0, Ntok - 1})
    B = len(hits)
    base = image_case(kind, B, Ntok, H, seed)
    tgt = torch.tensor([[hits[(b + h) % B] for h in range(H)] for b in range(B)])
    q = torch.zeros(B, H, 1, 64, dtype=F64)
    for b in range(B):
        for h in range(H):
            if kind == "needle":
                q[b, h, 0] = base.k[b, h, tgt[b, h]]
            else:
                cd = slice(0, 32) if kind == "tied_lo" else slice(32, 64)
                q[b, h, 0, cd] = base.k[b, h, tgt[b, h], cd]
    hard = hard_attention(q, base.k, base.v)
    return SimpleNamespace(kind=kind, B=B, N=Ntok, H=H, base=base, q=q, tgt=tgt, o=hard.o, lse=hard.lse, hits=hits)


def query_case(kind, B, Q, Ntok, H, order=("one_off", "none", "both"), seed=0):
    """cs_attn_query_fwd with allow masks (no rotary embedding): Q query rows per image, allow [B*Q, Ntok] shared by the heads.  Row b*Q + r
    takes the kinds of `order` in turn:
      needle:  one_off = the needle key disallowed (the runner-up wins), both = needle and runner-up allowed (the needle wins);
      tied_*:  one_off = one partner disallowed (the other wins alone), both = both allowed (p = 1/2 each);
      none = every key disallowed (o = 0, lse = +inf).  Every other key is allowed with probability 1/2.
    The heads of a row target disjoint keys, so that one head's mask does not hide another head's target."""
    gen = torch.Generator().manual_seed(5000 + 31 * Ntok + 7 * Q + len(kind) + seed)
    base = image_case(kind, B, Ntok, H, seed)
    k, v = base.k, base.v
    q = torch.zeros(B, H, Q, 64, dtype=F64)
    allow = (torch.rand(B * Q, Ntok, generator=gen) < 0.5)
    kinds = []
    unit = codes(Ntok, 64, 1.0)
    for b in range(B):
        for r in range(Q):
            g = b * Q + r
            what = order[g % len(order)]
            kinds.append(what)
            if kind == "needle":
                while True:
                    a = torch.randperm(Ntok, generator=gen)[:H].tolist()
                    nb = [_nearest(unit, x, torch.ones(Ntok, dtype=torch.bool)) for x in a]
                    if len(set(a) | set(nb)) == 2 * H:
                        break
                for h in range(H):
                    # no visible key may be nearer to a than b: b is the nearest of ALL keys
                    q[b, h, r] = two_level(unit, a[h], nb[h])
                    allow[g, nb[h]] = True
                    allow[g, a[h]] = what != "one_off"
            else:
                M = base.M
                cd = slice(0, 32) if kind == "tied_lo" else slice(32, 64)
                t = torch.randperm(M, generator=gen)[:H].tolist()
                assert len(t) == H
                for h in range(H):
                    q[b, h, r, cd] = k[b, h, t[h], cd]
                    allow[g, t[h]] = allow[g, t[h] + M] = True
                    if what == "one_off":
                        allow[g, t[h] + M * ((g // len(order) + h) % 2)] = False
            if what == "none":
                allow[g] = False
    vis = allow.view(B, 1, Q, Ntok)
    hard = hard_attention(q, k, v, vis)
    return SimpleNamespace(kind=kind, B=B, Q=Q, N=Ntok, H=H, base=base, q=q, k=k, v=v, allow=allow.to(torch.uint8), vis=vis, kinds=kinds,
                           P=hard.P, o=hard.o, lse=hard.lse, cnt=hard.cnt)


def passenger_case(kind, B, Q, Ntok, H, seed=0):
    """query_case(tied) plus the backward of the extra rows: dout one small integer per row, expected dq [B,H,Q,64] and the dK / dV the
    image-less cs_attn_bwd(extra=) writes (float64; exactness asserted)."""
    c = query_case(kind, B, Q, Ntok, H, order=("both", "one_off", "none"), seed=seed)
    gen = torch.Generator().manual_seed(9000 + Ntok + Q)
    c.dout = _one_hot_dout(gen, B, H, Q)
    c.dq, c.dk, c.dv, c.dS = hard_backward(c.P, c.q, c.k, c.v, c.o, c.dout)
    return c


def causal_case(B, L, H, seed=0):
    """Causal self-attention: keys 8 * code(j); even rows carry a needle in the past (a <= i: a wins), odd rows their best key in the future
    (a > i, b = the nearest past key to a: b wins).  -> q, k, v [B,H,L,64] and the expected o."""
    gen = torch.Generator().manual_seed(7000 + 13 * L + H + seed)
    unit = codes(L, 64, 1.0)
    k = (8.0 * unit).expand(B, H, L, 64).clone()
    v = _ints(gen, (B, H, L, 64), 8)
    q = torch.zeros(B, H, L, 64, dtype=F64)
    future = torch.zeros(B, H, L, dtype=torch.bool)
    past = torch.arange(L)
    for b in range(B):
        for h in range(H):
            for i in range(L):
                if i % 2 == 1 and i < L - 1:
                    a = i + 1 + int(torch.randint(0, L - 1 - i, (1,), generator=gen))
                    nb = _nearest(unit, a, past <= i)
                    future[b, h, i] = True
                else:
                    a = int(torch.randint(0, i + 1, (1,), generator=gen))
                    nb = _nearest(unit, a, torch.ones(L, dtype=torch.bool)) if L > 1 else a
                q[b, h, i] = two_level(unit, a, nb)
    vis = torch.ones(L, L, dtype=torch.bool).tril_().view(1, 1, L, L)
    hard = hard_attention(q, k, v, vis)
    return SimpleNamespace(B=B, L=L, H=H, q=q, k=k, v=v, vis=vis, future=future, o=hard.o, P=hard.P)


# ------------------------------------------------------------------------------------------------ a float64 model that can be made wrong
def model64(q, k, v, vis=None, chunk=None, skip_rescale=None):
    """softmax(scale q k^T | vis) v in float64 on rotated rows [B,H,*,64], as an online softmax over key chunks of `chunk` keys (None: one
    chunk).  skip_rescale = (b, h, row): that row keeps alpha = 1 when its maximum rises in a later chunk (the mutation).  -> o, lse"""
    S = (q @ k.transpose(-1, -2)) * SCALE
    if vis is not None:
        S = S.masked_fill(~vis.expand_as(S), float("-inf"))
    N = k.shape[-2]
    step = chunk or N
    m = torch.full(S.shape[:-1] + (1,), float("-inf"), dtype=F64)
    l = torch.zeros_like(m)
    o = torch.zeros(q.shape, dtype=F64)
    for k0 in range(0, N, step):
        s = S[..., k0:k0 + step]
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp(m - safe)
        if skip_rescale is not None and k0 > 0:
            b, h, r = skip_rescale
            alpha[b, h, r] = 1.0
        p = torch.exp(s - safe)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ v[..., k0:k0 + step, :]
        m = m_new
    none = l == 0
    o = torch.where(none, torch.zeros_like(o), o / l.clamp_min(1e-300))
    lse = torch.where(none, torch.full_like(m, float("inf")), m + torch.log(l.clamp_min(1e-300)))[..., 0]
    return o, lse
