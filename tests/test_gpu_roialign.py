"""`-m gpu`: the distillation head's RoIAlign on the MI355X, element by element (cs_roialign_fwd's plain pooling form and cs_roialign_bwd,
HipOps.roialign_fwd / roialign_bwd), against the float64 restatement of tests/_roialign_ref.py.

Every case of its list (which case reaches which path of the kernels: that module's docstring): the lattice cases bit for bit -- pooled
rows, the gradient added onto an integer prefill, the CLS row, the tokens after the grid and the images without a box -- and the random
ones inside the bound derived there per element, (n + 5) u S forward and (n + 6) u S + u |result| backward.  Off the power-of-two grids
the compiler decides whether a box's map coordinate is one fma or a rounded product and a subtraction: a launch must sit inside the
bound of ONE of the two forms with all its boxes, and the forward and the backward gather must have taken the same one, or the backward is
not the adjoint of the forward.  Then the adjoint identity <fwd(F), dP> = <F, bwd(dP)> from the device outputs, the 7 x 5 outputs as the
5 x 7 outputs of the transposed problem, 600 boxes (three chunks of the backward's compaction) per element and twice with equal bits,
a second backward onto the first one's output, and permuted box rows.  Measured fractions of the bound: profiles/roialign_parity.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _roialign_ref as R  # noqa: E402

F32 = torch.float32
_device = {}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _fwd(hip, c, rois=None):
    rois = c["rois"] if rois is None else rois
    pooled = torch.full((len(rois), c["E"]), float("nan"), dtype=F32, device="cuda")
    hip.roialign_fwd(torch.from_numpy(c["feat"]).cuda(), torch.from_numpy(rois).cuda(), pooled, c["h"], c["w"], c["tok_off"])
    return pooled.cpu().numpy()


def _bwd(hip, c, onto, rois=None, dP=None, launches=1):
    """-> dfeat [B, Ntok, E] after `launches` launches onto a copy of `onto`."""
    rois = c["rois"] if rois is None else rois
    dP = c["dP"] if dP is None else dP
    dfeat = torch.from_numpy(onto).cuda().clone()
    r, g = torch.from_numpy(rois).cuda(), torch.from_numpy(np.ascontiguousarray(dP)).cuda()
    for _ in range(launches):
        hip.roialign_bwd(g, r, dfeat, c["h"], c["w"], c["tok_off"])
    return dfeat.cpu().numpy()


def _outputs(hip, name):
    """The case's device outputs, computed once and shared (read-only): pooled, dfeat onto the prefill, dzero onto zeros."""
    if name not in _device:
        c = R.build_case(name)
        _device[name] = dict(pooled=_fwd(hip, c), dfeat=_bwd(hip, c, c["prefill"]), dzero=_bwd(hip, c, np.zeros_like(c["prefill"])))
    return _device[name]


def _forms(c, o):
    """{form: (forward, backward, backward onto zeros) fractions of that form's bound}, and the forms that hold each launch whole."""
    frac = {f: (R.forward_fraction(c, f, o["pooled"]), R.backward_fraction(c, f, o["dfeat"]),
                R.backward_fraction(c, f, o["dzero"], prefill=np.zeros_like(c["prefill"]))) for f in R.FORMS}
    fwd = [f for f in R.FORMS if frac[f][0] <= 1]
    bwd = [f for f in R.FORMS if frac[f][1] <= 1 and frac[f][2] <= 1]
    return frac, fwd, bwd


def _form_of(hip, name):
    """The coordinate form the case's launches are held to: the one whose bound holds both (any on a power-of-two grid)."""
    c, o = R.build_case(name), _outputs(hip, name)
    _, fwd, bwd = _forms(c, o)
    both = [f for f in fwd if f in bwd]
    assert both, f"{name}: no coordinate form holds the forward and the backward (forward {fwd}, backward {bwd})"
    return both[0]


# ------------------------------------------------------------------------------------------------ lattice: bits
@pytest.mark.parametrize("name", R.LATTICE)
def test_lattice_cases_give_the_expected_bits(hip, name):
    c, o = R.build_case(name), _outputs(hip, name)
    assert c["exact"], "the lattice case is not exact in fp32: its draw is wrong"
    ref = c["ref"]["rounded"]
    assert o["pooled"].shape == (c["K"], c["E"])
    R.same_bits(o["pooled"], ref["fwd"]["out"], f"{name} pooled")
    R.same_bits(o["dfeat"], R.expected_tokens(c, "rounded"), f"{name} dfeat")          # the whole tensor: CLS row, trailing tokens, empty images
    outside = np.ones(c["prefill"].shape, bool)
    R.grid_of(c, outside)[...] = False
    for b in c["empty"]:
        outside[b] = True
    assert outside.any() and np.array_equal(o["dfeat"].view(np.int32)[outside], c["prefill"].view(np.int32)[outside])
    if c["K"] > 1:                                                             # the order of the box rows changes no bit
        p = np.random.RandomState(7).permutation(c["K"])
        rois, dP = np.ascontiguousarray(c["rois"][p]), np.ascontiguousarray(c["dP"][p])
        assert np.array_equal(_bwd(hip, c, c["prefill"], rois=rois, dP=dP).view(np.int32), o["dfeat"].view(np.int32))
        assert np.array_equal(_fwd(hip, c, rois=rois).view(np.int32), o["pooled"][p].view(np.int32))


# ------------------------------------------------------------------------------------------------ random: the bound per element
@pytest.mark.parametrize("name", R.RANDOM_POW2)
def test_random_cases_on_power_of_two_grids_are_inside_the_bound(hip, name):
    c, o = R.build_case(name), _outputs(hip, name)
    assert R.violations(c) == 0 and c["ref"]["fused"] is c["ref"]["rounded"]
    f, b, z = _forms(c, o)[0]["rounded"]
    print(f"PARITY {name}: forward {f:.3f} backward {b:.3f} (onto zeros {z:.3f}) of the bound")
    assert f <= 1 and b <= 1 and z <= 1


@pytest.mark.parametrize("name", R.RANDOM_OTHER)
def test_random_cases_on_other_grids_hold_one_coordinate_form(hip, name):
    """Every element of a launch inside the bound of one form, the same for all its boxes -- and the same for both kernels."""
    c, o = R.build_case(name), _outputs(hip, name)
    assert R.violations(c) == 0 and R.distinguishable(c) == (True, True)       # at most one form can hold a launch
    frac, fwd, bwd = _forms(c, o)
    for form in R.FORMS:
        f, b, z = frac[form]
        print(f"PARITY {name} [{form}]: forward {f:.3f} backward {b:.3f} (onto zeros {z:.3f}) of the bound")
    print(f"FORM {name}: forward {fwd} backward {bwd}")
    assert len(fwd) == 1, f"{name}: the forward is inside the bound of {fwd or 'neither form'}: {frac}"
    assert len(bwd) == 1, f"{name}: the backward is inside the bound of {bwd or 'neither form'}: {frac}"
    assert fwd == bwd, f"{name}: the forward computes the {fwd[0]} coordinate, the backward the {bwd[0]} one: not its adjoint"


# ------------------------------------------------------------------------------------------------ adjoint identity
@pytest.mark.parametrize("name", R.LATTICE + R.RANDOM)
def test_backward_is_the_adjoint_of_the_forward(hip, name):
    c, o = R.build_case(name), _outputs(hip, name)
    lhs = float((o["pooled"].astype(np.float64) * c["dP"]).sum())
    rhs = float((R.grid_of(c, c["feat"]).astype(np.float64) * R.grid_of(c, o["dzero"])).sum())
    if c["lattice"]:
        assert lhs == rhs, (name, lhs, rhs)                                    # sums of exact fp32 numbers, far below 2^53 quanta
        return
    ref = c["ref"][_form_of(hip, name)]
    zero = np.zeros((c["B"], c["h"], c["w"], c["E"]), np.float32)
    tol = float((ref["fwd"]["bound"] * np.abs(c["dP"])).sum() + (R.backward_bound(ref["bwd"], zero) * np.abs(R.grid_of(c, c["feat"]))).sum())
    print(f"ADJOINT {name}: |<fwd(F), dP> - <F, bwd(dP)>| = {abs(lhs - rhs):.3e}, {abs(lhs - rhs) / tol:.3f} of the two bounds' sum")
    assert abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------ h and w
def test_swap_pair_gives_the_transposed_outputs(hip):
    """7 x 5 is 5 x 7 with map and boxes transposed: the same terms in another order, so the two launches differ by at most the two
    bounds (which are equal)."""
    a, b = (R.build_case(n) for n in R.SWAP_PAIR)
    oa, ob = (_outputs(hip, n) for n in R.SWAP_PAIR)
    form = _form_of(hip, R.SWAP_PAIR[0])
    assert _form_of(hip, R.SWAP_PAIR[1]) == form
    ra, rb = a["ref"][form], b["ref"][form]
    worst = R.fraction(ob["pooled"], oa["pooled"].astype(np.float64), ra["fwd"]["bound"] + rb["fwd"]["bound"])
    ga, gb = R.grid_of(a, oa["dfeat"]), R.grid_of(b, ob["dfeat"]).transpose(0, 2, 1, 3)
    bound = R.backward_bound(ra["bwd"], R.grid_of(a, a["prefill"])) + R.backward_bound(rb["bwd"], R.grid_of(b, b["prefill"])).transpose(0, 2, 1, 3)
    worst_b = R.fraction(gb, ga.astype(np.float64), np.where(ra["bwd"]["mag"] == 0, 0.0, bound))
    print(f"SWAP: forward {worst:.3f} backward {worst_b:.3f} of the two bounds' sum")
    assert worst <= 1 and worst_b <= 1
    assert not np.array_equal(ob["pooled"], 0 * ob["pooled"])


# ------------------------------------------------------------------------------------------------ many boxes, accumulation
@pytest.mark.parametrize("name", R.MANY_BOXES)
def test_six_hundred_boxes_per_element_and_twice_with_equal_bits(hip, name):
    """Three chunks of the backward's compaction: boxes of the second and third chunk are needed to stay inside the bound
    (tests/test_roialign_ref_cpu.py proves that on the reference)."""
    c, o = R.build_case(name), _outputs(hip, name)
    assert c["K"] == 600
    if c["lattice"]:
        R.same_bits(o["dfeat"], R.expected_tokens(c, "rounded"), f"{name} dfeat")
    else:
        assert R.backward_fraction(c, _form_of(hip, name), o["dfeat"]) <= 1
    again = _bwd(hip, c, c["prefill"])
    assert np.array_equal(again.view(np.int32), o["dfeat"].view(np.int32))
    assert np.array_equal(_fwd(hip, c).view(np.int32), o["pooled"].view(np.int32))


@pytest.mark.parametrize("name", R.LATTICE + R.RANDOM)
def test_second_backward_accumulates(hip, name):
    """A second launch onto the first one's output: prefill + twice the gradient.  An element whose reference gradient has no term keeps
    the prefill's bits (backward_fraction returns inf otherwise)."""
    c = R.build_case(name)
    twice = _bwd(hip, c, c["prefill"], launches=2)
    if c["lattice"]:
        R.same_bits(twice, R.expected_tokens(c, "rounded", times=2), f"{name} dfeat after two launches")
        return
    frac = R.backward_fraction(c, _form_of(hip, name), twice, times=2)
    print(f"PARITY {name}: two launches {frac:.3f} of the bound")
    assert frac <= 1
