"""`-m gpu`: the point-wise, column-sum, L2-norm and loss kernels element by element against tests/_pointwise_ref.py.

Activations (cs_gelu_fwd / bwd for both forms, cs_swiglu_fwd / bwd / bwd_q8) on every finite bf16 input, inside the bounds that module's
docstring derives and with at most 1 % of the elements off bf16(float64 value); cs_cast_f32_bf16 on every tie, bit for bit;
cs_colsum_bf16 on integers at every residue of its unrolled loops, bit for bit, and cs_swiglu_bwd_colsum bit-equal to the two-pass
form at the row-block edges; cs_l2norm, cs_cosine_loss and cs_fed_bce per row and per element, bit for bit where the case is exact;
one case per grid-stride kernel that makes its loop wrap.  Outputs are handed in as NaN, so an unwritten element fails.  The worst
err / bound and the largest share of each family go to the metrics file of test_gpu_ops.check (profiles/pointwise_parity.md)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pointwise_ref as P  # noqa: E402
from test_gpu_ops import _metric  # noqa: E402  (one metrics file for both modules)

BF, F32 = torch.bfloat16, torch.float32
WORST, SHARE = {}, {}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    yield HipOps()
    for k in sorted(WORST):
        _metric(f"pointwise.{k}: worst err/bound {WORST[k]:.4f}" + (f", largest share off bf16(float64) {SHARE[k]:.4%}" if k in SHARE else ""))


# ------------------------------------------------------------------------------------------------ plumbing
def _bf_dev(bits, pad=0):
    """uint16 bf16 bits [M, N] -> cuda bf16 view [M, N] of rows N + pad wide; the padding holds NaN."""
    M, N = bits.shape
    full = np.full((M, N + pad), 0x7FC0, np.uint16)
    full[:, :N] = bits
    return torch.from_numpy(full.view(np.int16)).cuda().view(BF)[:, :N]


def _vals_dev(v, pad=0):
    return _bf_dev(P.bits_of(v), pad)


def _bf_host(t):
    """cuda bf16 tensor -> float64 numpy."""
    return P.bf16_to_f32(t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)).astype(np.float64)


def _nan(shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _f32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _check(family, name, got, want, bound, inputs=None, share=False):
    msg, worst = P.compare(f"{family}[{name}]", got, want, bound, inputs)
    line = f"pointwise.{family}[{name}]: worst err/bound {worst:.4f}"
    WORST[family] = max(WORST.get(family, 0.0), worst)
    if share and msg is None:
        s = P.share_differing(got, want)
        line += f", share off bf16(float64) {s:.4%}"
        if want.size >= P.SHARE_MIN_ELEMENTS:
            SHARE[family] = max(SHARE.get(family, 0.0), s)
        msg = P.share_message(f"{family}[{name}]", s, want.size)
    _metric(line)
    print(line)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ activations
ACTS = [(kind, shape) for kind in ("gelu", "quick", "swiglu") for shape in P.ACT_SHAPES]
ACT_IDS = [f"{kind}-{shape[0]}" for kind, shape in ACTS]


def _run_fwd(hip, kind, pat, x2_bits, pad=0):
    """The kernel's output (float64 numpy) on the pattern matrix; x2_bits: bf16 bits of the SwiGLU companion."""
    M, N = pat.shape
    if kind == "swiglu":
        h = _nan((M, N))
        hip.swiglu_fwd(_bf_dev(np.concatenate([pat, x2_bits], 1), pad), h)
        return _bf_host(h)
    y = _nan((M, N))
    hip.gelu_fwd(_bf_dev(pat, pad), y, kind == "quick")
    return _bf_host(y)


def _run_bwd(hip, kind, pat, x2_bits, dh_bits, pad=0):
    M, N = pat.shape
    if kind == "swiglu":
        dx12 = _nan((M, 2 * N))
        hip.swiglu_bwd(_bf_dev(dh_bits, pad), _bf_dev(np.concatenate([pat, x2_bits], 1), pad), dx12)
        return _bf_host(dx12)
    dx = _nan((M, N))
    hip.gelu_bwd(_bf_dev(dh_bits, pad), _bf_dev(pat, pad), dx, kind == "quick")
    return _bf_host(dx)


def _want_fwd(kind, pat, x2):
    return P.expect_swiglu_fwd(pat, x2) if kind == "swiglu" else P.expect_act_fwd(kind, pat)


def _want_bwd(kind, pat, x2, dh):
    return P.expect_swiglu_bwd(pat, x2, dh) if kind == "swiglu" else P.expect_act_bwd(kind, pat, dh)


@pytest.mark.parametrize("kind,shape", ACTS, ids=ACT_IDS)
def test_activation_forward_on_every_finite_bf16_input(hip, kind, shape):
    name, M, N, pad, ones = shape
    pat = P.patterns(M, N)
    x2 = P.companions(pat, 3, ones)
    got = _run_fwd(hip, kind, pat, P.bits_of(x2), pad)
    want, bound = _want_fwd(kind, pat, x2)
    _check("act_fwd", f"{kind}-{name}", got, want, bound, P.X64[pat], share=True)


@pytest.mark.parametrize("kind,shape", ACTS, ids=ACT_IDS)
def test_activation_backward_on_every_finite_bf16_input(hip, kind, shape):
    name, M, N, pad, ones = shape
    pat = P.patterns(M, N)
    x2, dh = P.companions(pat, 3, ones), P.companions(pat, 5, ones)
    got = _run_bwd(hip, kind, pat, P.bits_of(x2), P.bits_of(dh), pad)
    want, bound = _want_bwd(kind, pat, x2, dh)
    x = P.X64[pat]
    _check("act_bwd", f"{kind}-{name}", got, want, bound, np.concatenate([x, x], 1) if kind == "swiglu" else x, share=True)


@pytest.mark.parametrize("M,Hd", P.Q8_SHAPES)
def test_swiglu_backward_q8_writes_the_same_dx12(hip, M, Hd):
    pat = P.patterns(M, Hd, P.q8_offsets()[(M, Hd)])
    x2, dh = P.companions(pat, 3), P.companions(pat, 5)
    x12 = _bf_dev(np.concatenate([pat, P.bits_of(x2)], 1))
    dx12 = _nan((M, 2 * Hd))
    Kp = (2 * Hd + 127) // 128 * 128
    q8, scale = torch.full((M, Kp), 0x55, dtype=torch.uint8, device="cuda"), _nan((M,), F32)
    hip.swiglu_bwd_q8(_vals_dev(dh), x12, dx12, q8, scale)
    want, bound = P.expect_swiglu_bwd(pat, x2, dh)
    x = P.X64[pat]
    _check("q8", f"M{M}-Hd{Hd}", _bf_host(dx12), want, bound, np.concatenate([x, x], 1), share=True)
    assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all())


# ------------------------------------------------------------------------------------------------ cast
def test_cast_rounds_every_tie_to_even(hip):
    bits = P.cast_inputs()
    y = _nan((bits.size,))
    hip.cast_f32_bf16(torch.from_numpy(bits.view(np.int32)).cuda().view(F32), y)
    msg = P.cast_mismatch("cast", bits, y.cpu().view(torch.int16).numpy().view(np.uint16))
    _metric(f"pointwise.cast: {bits.size} inputs, {'bit-equal to round-to-nearest-even' if msg is None else msg}")
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("name", list(P.COLSUM_CASES))
def test_column_sums_of_integers_bit_for_bit(hip, name):
    c = P.colsum_case(name)
    flat = torch.from_numpy(P.bits_of(c["flat"]).view(np.int16)).cuda().view(BF)
    x = flat.as_strided((c["M"], c["N"]), (c["ld"], 1), c["offset"])
    assert (x.data_ptr() % 16 != 0) == (c["offset"] != 0)
    out = _f32_dev(c["start"])
    hip.colsum_bf16(x, out)
    got = out.cpu().numpy()
    _check("colsum", name, got, c["want"], 0.0)
    assert P.same_bits32(got, c["want"])


@pytest.mark.parametrize("M,Hd", P.FUSED_COLSUM_SHAPES)
def test_fused_swiglu_bias_gradients_equal_the_two_pass_form_at_the_block_edges(hip, M, Hd):
    g = torch.Generator().manual_seed(1000 * M + Hd)
    dh = (0.5 * torch.randn((M, Hd), generator=g)).to(BF).cuda()
    x12 = (1.5 * torch.randn((M, 2 * Hd), generator=g)).to(BF).cuda()
    start = torch.randn((2 * Hd,), generator=g).cuda()
    ws = torch.empty(hip.colsum_workspace(M, 2 * Hd), dtype=torch.uint8, device="cuda")
    d0, c0 = _nan((M, 2 * Hd)), start.clone()
    hip.swiglu_bwd(dh, x12, d0)
    hip.colsum_bf16(d0, c0, ws)
    d1, c1 = _nan((M, 2 * Hd)), start.clone()
    hip.swiglu_bwd_colsum(dh, x12, d1, c1, ws)
    assert bool(torch.isfinite(d0.float()).all())
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16)), f"{int((d0 != d1).sum())} elements of dx12 differ"
    assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)), f"{int((c0 != c1).sum())} of {2 * Hd} column sums differ"


# ------------------------------------------------------------------------------------------------ L2 norm
@pytest.mark.parametrize("name", list(P.L2_CASES))
def test_l2norm_per_row_and_per_element(hip, name):
    c = P.l2_case(name)
    M, C = c["M"], c["C"]
    y, inv, dx = _nan((M, C), F32), _nan((M,), F32), _nan((M, C))
    hip.l2norm_fwd(_f32_dev(c["x"]), y, inv)
    hip.l2norm_bwd(_f32_dev(c["dy"]), _f32_dev(c["y32"]), _f32_dev(c["inv32"]), dx)      # from the statement's forward: its own error only
    _check("l2norm.inv", name, inv.cpu().numpy(), c["inv"], c["inv_b"])
    _check("l2norm.y", name, y.cpu().numpy(), c["y"], c["y_b"], c["x"])
    _check("l2norm.dx", name, _bf_host(dx), c["dx"], c["dx_b"], c["dy"])


# ------------------------------------------------------------------------------------------------ cosine loss
@pytest.mark.parametrize("name", list(P.COS_CASES))
def test_cosine_loss_per_row_and_per_element(hip, name):
    c = P.cos_case(name)
    K, E = c["K"], c["E"]
    s, t = _f32_dev(c["s"]), _f32_dev(c["t"])
    stats, loss = _nan((K, 3), F32), _nan((1,), F32)
    hip.cosine_loss_fwd(s, t, stats, loss, c["weight"])
    _check("cosine.stats", name, stats.cpu().numpy(), c["stats"], c["stats_b"])
    _check("cosine.loss", name, loss.cpu().numpy(), np.array([c["loss"]]), c["loss_b"])
    st32 = _f32_dev(c["stats32"])
    for key, up in (("ds", None), ("ds_up", torch.tensor([P.COS_UPSTREAM], device="cuda"))):
        ds = _nan((K, E), F32)
        hip.cosine_loss_bwd(s, t, st32, ds, c["weight"], c["grad_scale"], up)
        _check(f"cosine.{key}", name, ds.cpu().numpy(), c[key], c[key + "_b"], c["s"])


# ------------------------------------------------------------------------------------------------ federated BCE
@pytest.mark.parametrize("name", list(P.BCE_CASES))
def test_fed_bce_per_row_and_per_element(hip, name):
    c = P.bce_case(name)
    K, ns = c["K"], c["ns"]
    logits, tgt = _f32_dev(c["logits"]), torch.from_numpy(c["tgt"]).cuda()
    row, loss = _nan((K,), F32), _nan((1,), F32)
    hip.fed_bce_fwd(logits, tgt, row, loss, ns, c["temp"], c["weight"])
    _check("fed_bce.row", name, row.cpu().numpy(), c["row"], c["row_b"])
    _check("fed_bce.loss", name, loss.cpu().numpy(), np.array([c["loss"]]), c["loss_b"])
    for key, up in (("dz", None), ("dz_up", torch.tensor([P.BCE_UPSTREAM], device="cuda"))):
        dz = _nan((K, c["ldd"]))
        hip.fed_bce_bwd(logits, tgt, dz, ns, c["temp"], c["weight"], up)
        _check(f"fed_bce.{key}", name, _bf_host(dz), c[key], c[key + "_b"])


# ------------------------------------------------------------------------------------------------ grid-stride wrap
WRAPS = ["gelu_fwd", "quick_fwd", "gelu_bwd", "quick_bwd", "swiglu_fwd", "swiglu_bwd", "cast"]


@pytest.mark.parametrize("which", WRAPS)
def test_grid_stride_loop_second_trip(hip, which):
    """Just over 4096 x 256 vectors of eight: the loop's second trip.  Row r, column c holds pattern (r N + c) mod 65536 (companions 1),
    so the expected matrix repeats every 32 rows and is one gather from the table."""
    if which == "cast":
        i = np.arange(P.WRAP_CAST, dtype=np.uint64)
        bits = (((i % 65536) << 16) | ((i * 40503) & 0xFFFF)).astype(np.uint32)
        bits = np.where((bits & 0x7F800000) == 0x7F800000, np.uint32(0), bits)
        y = _nan((bits.size,))
        hip.cast_f32_bf16(torch.from_numpy(bits.view(np.int32)).cuda().view(F32), y)
        msg = P.cast_mismatch("wrap cast", bits, y.cpu().view(torch.int16).numpy().view(np.uint16))
        assert msg is None, msg
        return
    M, N = P.WRAP_ROWS, P.WRAP_COLS
    assert 65536 % N == 0
    period = 65536 // N
    block = P.patterns(period, N)
    ones = np.ones(block.shape)
    kind, direction = which.split("_")
    reps = -(-M // period)
    pat = np.tile(block, (reps, 1))[:M]
    one = np.full((M, N), 0x3F80, np.uint16)
    got = _run_fwd(hip, kind, pat, one) if direction == "fwd" else _run_bwd(hip, kind, pat, one, one)
    want, bound = _want_fwd(kind, block, ones) if direction == "fwd" else _want_bwd(kind, block, ones, ones)
    x = P.X64[block]
    x = np.concatenate([x, x], 1) if which == "swiglu_bwd" else x
    image = P.bf16_round64(want)
    worst, differing = 0.0, 0
    for r0 in range(0, M, period):
        rows = min(period, M - r0)
        msg, w = P.compare(f"wrap[{which}] rows {r0}..{r0 + rows - 1}", got[r0:r0 + rows], want[:rows], bound[:rows], x[:rows])
        assert msg is None, msg
        worst = max(worst, w)
        differing += int((got[r0:r0 + rows] != image[:rows]).sum())
    share = differing / got.size
    WORST["wrap"] = max(WORST.get("wrap", 0.0), worst)
    SHARE["wrap"] = max(SHARE.get("wrap", 0.0), share)
    _metric(f"pointwise.wrap[{which}]: worst err/bound {worst:.4f}, share off bf16(float64) {share:.4%}")
    msg = P.share_message(f"wrap[{which}]", share, got.size)
    assert msg is None, msg
