"""tests/_pointwise_ref.py on the CPU: the generators meet their own preconditions, an fp32 numpy restatement of every kernel's
expression lies inside the bounds on every case (the QuickGELU gradient in the fixed form; the parent commit's form is shown to give
NaN on exactly the inputs whose product with 1.702 overflows), the share cap holds for the restatement, and the bounds reject each
planted error."""
import numpy as np
import pytest
import torch

import _pointwise_ref as P

F32, F64 = np.float32, np.float64


def _bf(v32):
    """What the kernels store: the fp32 value rounded to bf16 (nearest even), as float64."""
    return P.bf16_to_f32(P.rne_bits(np.asarray(v32, F32))).astype(F64)


def _x32(pat):
    return P.X64[pat].astype(F32)


def _ok(name, got, want, bound, inputs=None):
    msg, worst = P.compare(name, got, want, bound, inputs)
    assert msg is None, msg
    return worst


def _rejects(name, got, want, bound):
    msg, worst = P.compare(name, got, want, bound)
    assert msg is not None and worst > 1.0, f"{name}: the planted error passes (worst err / bound {worst:.3g})"
    return msg


# ------------------------------------------------------------------------------------------------ generators
def test_every_finite_pattern_is_an_input_exactly_once():
    assert int(P.FINITE.sum()) == 65280
    for _, M, N, _, _ in P.ACT_SHAPES:
        pat = P.patterns(M, N).ravel()
        counts = np.bincount(pat, minlength=65536)
        assert M * N == 65536 and np.all(counts[P.FINITE][1:] == 1) and counts[0] == 1 + 256        # 0 stands in for the 256 non-finite ones
    seen = np.zeros(65536, bool)
    offsets = P.q8_offsets()
    for M, Hd in P.Q8_SHAPES:
        seen[P.patterns(M, Hd, offsets[(M, Hd)]).ravel()] = True
    assert np.all(seen[P.FINITE]), "the q8 cases together do not walk the whole domain"
    assert P.WRAP_ROWS * P.WRAP_COLS // 8 > P.GRID_CAP_VECTORS and P.WRAP_CAST // 8 > P.GRID_CAP_VECTORS and P.WRAP_CAST % 8 == 0
    assert (P.WRAP_ROWS - 1) * P.WRAP_COLS // 8 < P.GRID_CAP_VECTORS + 4 * 256, "the wrap case is larger than it needs to be"


def test_companions_are_bf16_numbers_and_keep_every_product_finite():
    P.bits_of(P.COMPANIONS)
    assert set(np.sign(P.COMPANIONS)) == {-1.0, 0.0, 1.0} and {0.0, 1.0, 0.5} <= set(P.COMPANIONS) and np.abs(P.COMPANIONS).max() <= 8
    pat = P.patterns(128, 512)
    x2, dh = P.companions(pat, 3), P.companions(pat, 5)
    pairs = set(zip((np.arange(pat.size) % 65536).tolist()[:22], x2.ravel().tolist()[:22]))
    assert len(pairs) == 22
    x1 = P.X64[pat]
    with np.errstate(over="raise"):
        for prod in (dh * x2, dh * x1, x2 * x1):
            assert np.all(np.abs(prod.astype(F32)) <= P.BF16_MAX)
    for want, _ in (P.expect_swiglu_fwd(pat, x2), P.expect_swiglu_bwd(pat, x2, dh), P.expect_act_bwd("gelu", pat, dh),
                    P.expect_act_bwd("quick", pat, dh)):
        assert np.all(np.isfinite(want)) and np.abs(want).max() <= P.BF16_MAX


def test_bf16_rounding_helpers_agree_with_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, 1, 4096), np.ldexp(rng.normal(0, 1, 4096), rng.integers(-140, 127, 4096)), [0.0, -0.0, 3.4e38]]).astype(F32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(P.rne_bits(x), want)
    assert np.array_equal(P.bf16_round64(x.astype(F64)), P.bf16_to_f32(want).astype(F64))
    assert P.bf16_round64(np.array([1.0 + 2.0 ** -8]))[0] == 1.0 and P.bf16_round64(np.array([1.0 + 3 * 2.0 ** -8]))[0] == 1.0 + 2.0 ** -6
    assert P.bf16_round64(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -7          # where rounding through fp32 first goes wrong
    assert P.bf16_spacing(np.array([1.0, 0.0, 2.0 ** -126, 1.99]))[[0, 1, 2, 3]].tolist() == [2.0 ** -7, 2.0 ** -133, 2.0 ** -133, 2.0 ** -7]


def test_column_sum_cases_cover_the_unroll_tails_and_block_counts():
    last_block_rows = {M % P.COLSUM_ROWS or P.COLSUM_ROWS for M in P.COLSUM_M}         # 16-row unroll (4 per row phase) and its tail
    assert last_block_rows == {1, 3, 4, 5, 7, 13, 15, 16, 17, 63, 64}
    blocks = {-(-M // P.COLSUM_ROWS) for M in P.COLSUM_M}
    assert blocks == {1, 2, 4, 6, 34}                                                  # both sides of 4 (the residues) and of 32 (the unroll)
    for name in P.COLSUM_CASES:
        c = P.colsum_case(name)                                                        # asserts the 2^24 precondition
        assert np.array_equal(P.colsum_restated(c["x"], c["start"]), c["want"]) and np.any(c["start"] != 0)
        assert np.all(c["flat"][c["offset"]:].reshape(c["M"], c["ld"])[:, c["N"]:] == 100)
    for name, (M, N, ld, off) in P.COLSUM_CASES.items():              # N % 8 != 0 alone: a ragged last vector beside vector threads
        if name not in ("M333-N512-ld515", "M333-N512-offset1"):
            assert ld % 8 == 0 and ld >= N and off == 0, name
    assert P.COLSUM_CASES["M333-N770"][2] == 776 and P.COLSUM_CASES["M1-N7"][2] == 8
    c = P.colsum_case("M333-N512-ld515")
    assert c["ld"] % 8 != 0 and P.colsum_case("M333-N512-offset1")["offset"] == 1


def test_l2_and_loss_cases_hold_every_row_kind():
    assert {P.l2_case(f"M1-C{C}")["kinds"][0] for C in P.L2_C} == set(P.L2_KINDS)
    nine = P.l2_case("M9-C1028")
    assert set(nine["kinds"]) == set(P.L2_KINDS) and nine["clamped"].sum() >= 4
    ex = P.cos_case("exact-K256-E256")
    cosv = ex["stats"][:, 0]
    assert {"same", "opposite", "orthogonal"} <= set(ex["kinds"]) and cosv[0] == 1.0 and cosv[1] == -1.0 and cosv[2] == 0.0
    assert np.array_equal(cosv * 256, np.rint(cosv * 256)) and np.all(ex["stats"][:, 1:] == 1.0 / 16)
    for name in P.BCE_CASES:
        c = P.bce_case(name)
        assert c["ldz"] > c["ns"] and c["ldd"] > c["ns"] and np.all(np.isnan(c["logits"][:, c["ns"]:]))
        assert np.all(c["dz"][:, c["ns"]:] == 0) and np.all(c["dz_b"][:, c["ns"]:] == 0)
        if c["K"] >= 3:
            assert {-1, 0, c["ns"] - 1} <= set(c["tgt"].tolist())
    assert {int(P.bce_case(f"seeded-K1-ns{ns}")["tgt"][0]) for ns in P.BCE_NS} == {-1, 0, 63}
    big = P.bce_case("seeded-K257-ns100")
    assert np.abs(big["logits"][:, :100] * 14.3).max() > 59


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("kind", P.UNARY)
def test_fp32_restatement_of_every_unary_form_is_inside_the_bound_on_the_whole_domain(kind):
    pat = P.PATTERNS[P.FINITE][None, :]
    x = _x32(pat)
    got = _bf(P.unary32(kind, x))
    want, e = P.table(kind)
    W = want[pat]
    _ok(kind, got, W, 0.5 * P.bf16_spacing(W) + e[pat] + P.FLOOR, x)
    share = P.share_differing(got, W)
    assert share <= P.ACT_MAX_SHARE / 2, share                       # room for a kernel's own exp / erf


def test_parent_quickgelu_gradient_is_nan_on_exactly_the_overflowing_inputs():
    x = _x32(P.PATTERNS[P.FINITE])
    parent, fixed = P.unary32("quick_grad", x, form="parent"), P.unary32("quick_grad", x)
    with np.errstate(over="ignore"):
        overflow = ~np.isfinite(F32(1.702) * x)
    assert int(overflow.sum()) == 210 and float(np.abs(x[overflow]).min()) > 2.0e38
    assert np.array_equal(~np.isfinite(parent), overflow) and np.all(np.isnan(parent[overflow]))
    assert np.all(np.isfinite(fixed))
    for kind in P.UNARY:
        assert np.all(np.isfinite(P.unary32(kind, x))), kind
    same = ~overflow                                                  # away from the overflow the two forms agree to a few roundings
    assert np.abs(parent[same].astype(F64) - fixed[same]).max() <= 8 * P.U * 1.2


@pytest.mark.parametrize("shape", P.ACT_SHAPES, ids=[s[0] for s in P.ACT_SHAPES])
def test_fp32_restatement_with_companions_is_inside_the_bound(shape):
    _, M, N, _, ones = shape
    pat = P.patterns(M, N)
    x1 = _x32(pat)
    x2, dh = P.companions(pat, 3, ones), P.companions(pat, 5, ones)
    x2f, dhf = x2.astype(F32), dh.astype(F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for kind in ("gelu", "quick"):
            want, bound = P.expect_act_bwd(kind, pat, dh)
            got = _bf(dhf * P.unary32(kind + "_grad", x1))
            _ok(f"{kind}_bwd", got, want, bound, x1)
            assert P.share_message(kind, P.share_differing(got, want), pat.size) is None
        want, bound = P.expect_swiglu_fwd(pat, x2)
        got = _bf(P.unary32("silu", x1) * x2f)
        _ok("swiglu_fwd", got, want, bound, x1)
        assert P.share_message("swiglu_fwd", P.share_differing(got, want), pat.size) is None
        sig = one / (one + P._exp32(-x1))
        got = np.concatenate([_bf(dhf * x2f * (sig + x1 * sig * (one - sig))), _bf(dhf * x1 * sig)], 1)
        want, bound = P.expect_swiglu_bwd(pat, x2, dh)
        _ok("swiglu_bwd", got, want, bound, np.concatenate([x1, x1], 1))
        assert P.share_message("swiglu_bwd", P.share_differing(got, want), got.size) is None


def test_bounds_reject_planted_activation_errors():
    pat = P.PATTERNS[P.FINITE][None, :]
    x = _x32(pat)
    for kind in ("quick", "quick_grad"):                              # 1.7 for 1.702
        W, e = (t[pat] for t in P.table(kind))
        _rejects(f"{kind} with 1.7", _bf(P.unary32(kind, x, c=1.7)), W, 0.5 * P.bf16_spacing(W) + e + P.FLOOR)
    W, e = (t[pat] for t in P.table("gelu"))
    bound = 0.5 * P.bf16_spacing(W) + e + P.FLOOR
    _rejects("tanh GELU", _bf(P.unary32("gelu", x, tanh=True)), W, bound)
    v = P.unary32("gelu", x)                                          # truncation for round-to-nearest-even at the output
    _rejects("truncated GELU", P.bf16_to_f32(P.trunc_bits(v)).astype(F64), W, bound)
    for kind in ("quick_grad", "silu_grad"):                          # a finite but wrong gradient on the largest inputs, where 1.702 x overflows
        W, e = (t[pat] for t in P.table(kind))
        bound = 0.5 * P.bf16_spacing(W) + e + P.FLOOR
        good = _bf(P.unary32(kind, x))
        top = np.abs(x[0]) >= 2.0e38
        assert int(top.sum()) == 210 and float(np.abs(W[0, top & (x[0] > 0)] - 1).max()) == 0.0
        for wrong in (0.0, 0.5, 1.0):
            got = good.copy()
            got[0, top & ((x[0] > 0) == (wrong != 1.0))] = wrong           # 0 or 0.5 for the true 1, 1 for the true 0
            msg = _rejects(f"{kind} = {wrong} on the largest inputs", got, W, bound)
            assert "105 of" in msg, msg
        assert float((bound / np.maximum(np.abs(W), 2.0 ** -7))[0, np.abs(x[0]) > 128].max()) < 2.0 ** -7     # half a spacing of 1 (2^-8) and 2^-14: nowhere vacuous
    W, e = (t[pat] for t in P.table("gelu"))
    bound = 0.5 * P.bf16_spacing(W) + e + P.FLOOR
    nan = _bf(v).copy()
    nan[0, 77] = np.nan                                               # an element the kernel never wrote
    assert "non-finite" in P.compare("unwritten", nan, W, bound)[0]
    off = _bf(v).copy()                                               # 2 % of the elements one bf16 step off: inside no bound, and over the share cap
    idx = np.arange(0, off.size, 50)
    off[0, idx] += P.bf16_spacing(off[0, idx])
    assert P.share_message("share", P.share_differing(off, W), off.size) is not None


# ------------------------------------------------------------------------------------------------ cast
def test_cast_case_holds_the_ties_and_rejects_other_roundings():
    bits = P.cast_inputs()
    x = bits.view(F32)
    assert bits.size % 8 == 0 and len(set(bits.tolist())) == bits.size
    low = bits & 0xFFFF
    ties = low == 0x8000
    finite = np.isfinite(x)
    assert int((ties & finite & ((bits >> 16) & 1 == 0)).sum()) > 30000 and int((ties & finite & ((bits >> 16) & 1 == 1)).sum()) > 30000
    for special in (0x00000001, 0x00008000, 0x007FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x7FC00000, 0xFF7F8000):
        assert special in bits, hex(special)
    rne = P.rne_bits(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    ok = ~np.isnan(x)
    assert np.array_equal(rne[ok], want[ok])                          # the bit trick against torch's own conversion
    assert rne[bits == 0x7F7F7FFF][0] == 0x7F7F and rne[bits == 0x7F7F8000][0] == 0x7F80 and rne[bits == 0x00008000][0] == 0
    assert P.cast_mismatch("rne", bits, rne) is None
    assert P.cast_mismatch("truncation", bits, P.trunc_bits(x)) is not None
    half_up = np.where(ok, ((bits.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16), rne)
    msg = P.cast_mismatch("round half up", bits, half_up)
    assert msg is not None and int((half_up != rne).sum()) == int((ties & ok & ((bits >> 16) & 1 == 0)).sum())
    nan_lost = rne.copy()
    nan_lost[np.isnan(x)] = 0x7F80
    assert P.cast_mismatch("NaN to inf", bits, nan_lost) is not None


# ------------------------------------------------------------------------------------------------ column sums
def test_column_sum_bound_rejects_a_dropped_last_row():
    for name, block in (("M333-N520", 5), ("M65-N8", 1), ("M1-N7", 0)):
        c = P.colsum_case(name)
        col = next(n for n in range(c["N"]) if c["x"][min(c["M"], (block + 1) * 64) - 1, n] != 0)
        got = P.colsum_restated(c["x"], c["start"], drop=(block, col))
        msg = _rejects(name, got, c["want"], 0.0)
        assert f"column {col}" in msg and "1 of" in msg


# ------------------------------------------------------------------------------------------------ L2 norm
@pytest.mark.parametrize("name", list(P.L2_CASES))
def test_l2norm_restatement_is_inside_the_bounds(name):
    c = P.l2_case(name)
    inv, y, dx = P.l2_restated(c["x"], c["dy"], c["y32"], c["inv32"])
    for key, got in (("inv", inv), ("y", y), ("dx", dx)):
        _ok(f"{name}.{key}", got, c[key], c[key + "_b"])
    if c["exact"]:
        assert float(c["inv_b"].max()) == 0.0 and float(c["dx_b"].max()) == 0.0


def test_l2norm_bounds_reject_a_missing_eps_clamp():
    c = P.l2_case("M5-C256")
    assert "zero" in c["kinds"] and "tiny" in c["kinds"]
    inv, y, _ = P.l2_restated(c["x"], c["dy"], c["y32"], c["inv32"], clamp=False)
    assert "non-finite" in P.compare("inv", inv, c["inv"], c["inv_b"])[0] and "non-finite" in P.compare("y", y, c["y"], c["y_b"])[0]
    zero, tiny = c["kinds"].index("zero"), c["kinds"].index("tiny")
    _rejects("tiny row", inv[tiny], c["inv"][tiny], c["inv_b"][tiny])
    unclamped = P.l2_ref(c["x"][[tiny]], c["dy"][[tiny]], clamp=False)
    _rejects("tiny row dx", unclamped["dx"], c["dx"][[tiny]], c["dx_b"][[tiny]])
    assert c["inv"][zero] == 1.0 / P.L2_EPS and np.all(c["y"][zero] == 0) and np.all(np.isfinite(c["dx"][zero])) and np.any(c["dx"][zero] != 0)


# ------------------------------------------------------------------------------------------------ cosine loss
@pytest.mark.parametrize("name", list(P.COS_CASES))
def test_cosine_restatement_is_inside_the_bounds(name):
    c = P.cos_case(name)
    stats, loss, ds = P.cos_restated(c["s"], c["t"], c["stats32"], c["weight"], c["grad_scale"])
    _ok(f"{name}.stats", stats, c["stats"], c["stats_b"])
    _ok(f"{name}.loss", [loss], np.array([c["loss"]]), c["loss_b"])
    _ok(f"{name}.ds", ds, c["ds"], c["ds_b"])
    _, _, ds_up = P.cos_restated(c["s"], c["t"], c["stats32"], c["weight"], c["grad_scale"], upstream=P.COS_UPSTREAM)
    _ok(f"{name}.ds_up", ds_up, c["ds_up"], c["ds_up_b"])


def test_cosine_bounds_reject_a_missing_final_inverse_norm():
    for name in ("K5-E252", "exact-K4-E256", "K600-E512"):
        c = P.cos_case(name)
        _, _, ds = P.cos_restated(c["s"], c["t"], c["stats32"], c["weight"], c["grad_scale"], final_is=False)
        _rejects(name, ds, c["ds"], c["ds_b"])
    c = P.cos_case("K257-E260")                                       # one row of K left out of the mean
    stats, _, _ = P.cos_restated(c["s"], c["t"], c["stats32"], c["weight"], c["grad_scale"])
    short = F32(c["weight"]) * (F32(1) - stats[:256, 0].sum(dtype=F32) / F32(257))
    _rejects("loss over K - 1 rows", [short], np.array([c["loss"]]), c["loss_b"])


# ------------------------------------------------------------------------------------------------ federated BCE
@pytest.mark.parametrize("name", list(P.BCE_CASES))
def test_fed_bce_restatement_is_inside_the_bounds(name):
    c = P.bce_case(name)
    z = c["logits"][:, :c["ns"]]
    row, loss, dz = P.bce_restated(z, c["tgt"], c["ldd"], c["temp"], c["weight"])
    _ok(f"{name}.row", row, c["row"], c["row_b"])
    _ok(f"{name}.loss", [loss], np.array([c["loss"]]), c["loss_b"])
    _ok(f"{name}.dz", dz, c["dz"], c["dz_b"])
    _, _, dz_up = P.bce_restated(z, c["tgt"], c["ldd"], c["temp"], c["weight"], upstream=P.BCE_UPSTREAM)
    _ok(f"{name}.dz_up", dz_up, c["dz_up"], c["dz_up_b"])
    if c["zero"]:
        assert np.allclose(c["row"], c["ns"] * np.log(2.0), rtol=1e-15) and float(c["dz_b"].max()) == 0.0
        t = np.arange(c["ns"])[None, :] == c["tgt"][:, None]
        assert np.array_equal(c["dz"][:, :c["ns"]], 0.125 * 16.0 * (0.5 - t))


def test_fed_bce_bounds_reject_a_target_column_off_by_one():
    for name in ("seeded-K5-ns64", "zero-K3-ns65", "seeded-K257-ns100"):
        c = P.bce_case(name)
        z = c["logits"][:, :c["ns"]]
        wrong = P.bce_ref(z, c["tgt"], c["ldd"], c["temp"], c["weight"], shift=1)
        _rejects(f"{name}.dz", wrong["dz"], c["dz"], c["dz_b"])
        if not c["zero"]:                                            # with logits 0 the loss does not depend on the target
            _rejects(f"{name}.row", wrong["row"], c["row"], c["row_b"])
