"""CPU: the numpy restatement of the distillation head's RoIAlign (tests/_roialign_ref.py) held to the oracle (oracle/roi_align_ref.py)
and to answers derived by hand, and the conditions its committed cases must meet, without a GPU.

The oracle walks every sample's four taps; the restatement first folds the samples of an axis into Wy / Wx in fp32, as the kernels do.
A folded weight is a sum of at most 2 g fp32 numbers (g samples of the axis), so it differs from the oracle's unfolded one by at most
(2 g - 1) u relative, and a product Wy Wx by (2 gh + 2 gw) u: the comparisons below allow (2 (gh + gw) + 2) u sum |w f| / count, the + 2
for the oracle's own fp32 output and the float64 summation orders."""
import numpy as np
import pytest
import torch

import _roialign_ref as R
from oracle.roi_align_ref import roi_align_1x1, roi_align_1x1_loops

SMALL = ["rnd_5x7", "rnd_7x5", "rnd_24x24", "rnd_14x14_b70", "lat_8x8_one", "lat_8x16_b70"]
CH = 4                                                                         # channels the scalar oracle is run on


def _pixel_rois(c):
    """What RefOps._rois_pixels hands the oracle: the normalised corners times the grid side, rounded to fp32 -- the `rounded` form."""
    r = torch.from_numpy(c["rois"]).clone()
    r[:, [1, 3]] *= c["w"]
    r[:, [2, 4]] *= c["h"]
    return r


def _folding(c):
    g = c["ref"]["rounded"]["geo"]
    return 2 * (np.maximum(g["gh"], 0) + np.maximum(g["gw"], 0)) + 2


@pytest.mark.parametrize("name", SMALL)
def test_forward_equals_the_oracles_scalar_loops(name):
    c = R.build_case(name)
    f = c["ref"]["rounded"]["fwd"]
    fmap = torch.from_numpy(np.ascontiguousarray(R.grid_of(c, c["feat"])[..., :CH]))
    want = roi_align_1x1_loops(fmap, _pixel_rois(c)).double().numpy()
    tol = _folding(c)[:, None] * R.U * f["mag"][:, :CH]
    assert (np.abs(f["out"][:, :CH] - want) <= tol).all()
    assert (want[f["mag"][:, 0] == 0] == 0).all() and f["out"].any()


@pytest.mark.parametrize("name", SMALL)
def test_backward_equals_autograd_through_the_oracle(name):
    c = R.build_case(name)
    b = c["ref"]["rounded"]["bwd"]
    probe = torch.zeros(c["B"], c["h"], c["w"], CH, dtype=torch.float64, requires_grad=True)
    out = roi_align_1x1(probe, _pixel_rois(c).double())
    (g,) = torch.autograd.grad(out, probe, torch.from_numpy(c["dP"][:, :CH]).double())
    tol = float(_folding(c).max()) * R.U * b["mag"][..., :CH]
    assert (np.abs(b["d"][..., :CH] - g.numpy()) <= tol).all()
    assert (g.numpy()[b["mag"][..., :CH] == 0] == 0).all() and b["d"].any()


@pytest.mark.parametrize("name", R.LATTICE)
def test_lattice_cases_are_exact_in_fp32(name):
    """Every term a multiple of 2^-10, every magnitude sum (two launches and the prefill) below 2^14, and an np.float32 evaluation of
    both directions with the float64 one's bits: the expected output of a lattice case is a bit pattern."""
    c = R.build_case(name)
    assert c["exact"] and c["pow2"] and c["ref"]["fused"] is c["ref"]["rounded"]
    g = c["ref"]["rounded"]["geo"]
    if c["K"]:
        assert set(np.unique(g["count"])) <= {2.0 ** i for i in range(7)}
        assert (g["Wy"].sum(1) < g["gh"]).any() and (g["Wx"].sum(1) < g["gw"]).any()      # samples were dropped on both axes
        assert (g["Wy"] > 1).any() or (g["Wx"] > 1).any()                                   # and samples were clamped onto a border cell


@pytest.mark.parametrize("name", R.RANDOM)
def test_random_cases_meet_the_redraw_rule(name):
    c = R.build_case(name)
    assert R.violations(c) == 0
    g = c["ref"]["rounded"]["geo"]
    assert all(np.array_equal(g[k], c["ref"]["fused"]["geo"][k]) for k in ("gh", "gw", "b"))
    if c["K"] >= 12:                                                           # every kind of box is there
        assert ((g["gh"] <= 0) | (g["gw"] <= 0)).any() and ((g["gh"] == 1) & (g["gw"] == 1)).any()
        assert ((g["gh"] == c["h"]) & (g["gw"] == c["w"])).any() and ((g["rh"] == 0) | (g["rw"] == 0)).any() and ((g["rh"] < 0) | (g["rw"] < 0)).any()
        assert (c["rois"][:, 1:] < 0).any() and (c["rois"][:, 1:] > 1).any()


@pytest.mark.parametrize("name", R.RANDOM_OTHER)
def test_the_two_coordinate_forms_can_be_told_apart(name):
    """Off the power-of-two grids some element of each direction has the two forms' references further apart than both bounds together:
    a launch inside the bound of one form is outside the other's."""
    c = R.build_case(name)
    assert not c["pow2"] and c["ref"]["fused"] is not c["ref"]["rounded"]
    assert R.distinguishable(c) == (True, True)


def test_the_redraw_rule_sees_what_it_should():
    assert R.violates([0, 0.0, 0.0, 1.0, 1.0], 14, 14) == "extent"              # the whole map: an integer extent
    assert R.violates([0, 0.1, 0.1, 0.1, 0.5], 14, 14) is None                 # zero-size: the exact 0 is let through
    assert R.violates([0, 0.1, 0.1, 0.1 + 1e-6, 0.5], 14, 14) == "extent"
    centre = (-1.0 + 5e-4 + 0.5) / 14                                           # 0.3 cells wide: one sample, 5e-4 above -1
    assert R.violates([0, centre - 0.15 / 14, 0.1, centre + 0.15 / 14, 0.5], 14, 14) == "sample"
    centre = (14.0 - 5e-4 + 0.5) / 14                                           # and 5e-4 below the map's size, on y
    assert R.violates([0, 0.1, centre - 0.15 / 14, 0.5, centre + 0.15 / 14], 14, 14) == "sample"
    assert R.violates([0, 0.1, 0.2, 0.5, 0.2 + (1.0 - 2e-4) / 14], 14, 14) in ("grid", "extent")       # an extent 2e-4 below 1: ceil may flip


def test_transposing_map_and_boxes_maps_the_swap_pair_onto_itself():
    a, b = (R.build_case(n) for n in R.SWAP_PAIR)
    assert (a["h"], a["w"]) == (b["w"], b["h"]) == (5, 7)
    back = R.transpose_case_inputs(b)
    assert np.array_equal(back["rois"], a["rois"]) and np.array_equal(back["feat"], a["feat"]) and np.array_equal(back["prefill"], a["prefill"])
    for form in R.FORMS:
        ra, rb = a["ref"][form], b["ref"][form]
        assert np.array_equal(ra["geo"]["Wy"].view(np.int32), rb["geo"]["Wx"].view(np.int32))
        assert np.array_equal(ra["geo"]["Wx"].view(np.int32), rb["geo"]["Wy"].view(np.int32))
        assert np.array_equal(ra["fwd"]["n"], rb["fwd"]["n"]) and np.array_equal(ra["bwd"]["n"], rb["bwd"]["n"].transpose(0, 2, 1, 3))
        assert np.abs(ra["fwd"]["out"] - rb["fwd"]["out"]).max() <= 1e-13 * ra["fwd"]["mag"].max()
        assert np.abs(ra["bwd"]["d"] - rb["bwd"]["d"].transpose(0, 2, 1, 3)).max() <= 1e-13 * ra["bwd"]["mag"].max()
    assert not np.array_equal(a["ref"]["fused"]["geo"]["Wy"][:, :5], a["ref"]["fused"]["geo"]["Wx"][:, :5])     # h and w are told apart


# ------------------------------------------------------------------------------------------------ answers by hand
def _one_box(box, h, w, fmap):
    geo = R.geometry(np.array([[0] + list(box)], np.float32), h, w, "rounded")
    return geo, R.forward_ref(fmap[None, ..., None].astype(np.float32), geo)["out"][0, 0]


def test_constant_map_pools_to_the_constant_times_the_kept_samples():
    """8 x 8 map of 2.5.  x from -2.25 to 1.75 in map space: 4 samples at -1.75 (below -1: dropped), -0.75 (clamped onto cell 0), 0.25, 1.25
    -> 3 kept; y from 5.25 to 9.25: samples at 5.75, 6.75, 7.75 (clamped onto the last cell), 8.75 (above 8: dropped) -> 3 kept.
    count = 16: 2.5 * 9 / 16."""
    box = [(-2.25 + 0.5) / 8, (5.25 + 0.5) / 8, (1.75 + 0.5) / 8, (9.25 + 0.5) / 8]
    geo, out = _one_box(box, 8, 8, np.full((8, 8), 2.5))
    assert (int(geo["gh"][0]), int(geo["gw"][0]), float(geo["count"][0])) == (4, 4, 16.0)
    assert geo["Wx"][0].tolist() == [1.75, 1.0, 0.25, 0, 0, 0, 0, 0] and geo["Wy"][0].tolist() == [0, 0, 0, 0, 0, 0.25, 1.0, 1.75]
    assert out == 2.5 * 9 / 16
    _, inside = _one_box([0.2, 0.3, 0.7, 0.6], 14, 14, np.full((14, 14), 2.5))
    assert abs(inside - 2.5) < 1e-6                                             # nothing dropped: the constant


def test_map_linear_in_x_pools_to_its_value_at_the_box_centre():
    """Bilinear interpolation reproduces a linear function and the samples are symmetric about the centre; the box stays inside
    [0, size - 1] in map space, where nothing is dropped or clamped.  Cell c holds the value at map coordinate c."""
    h, w = 5, 14
    fmap = np.broadcast_to(0.75 * np.arange(w)[None, :] - 2.0, (h, w))
    for box in ([0.21, 0.3, 0.83, 0.7], [0.5, 0.2, 0.52, 0.8], [0.1, 0.15, 0.9, 0.85]):
        cx = (box[0] + box[2]) / 2 * w - 0.5
        _, out = _one_box(box, h, w, fmap)
        assert abs(out - (0.75 * cx - 2.0)) < 1e-5, box
    fy = np.broadcast_to(0.75 * np.arange(h)[:, None] - 2.0, (h, w))           # and in y on the same boxes: h and w are not mixed up
    cy = (0.3 + 0.7) / 2 * h - 0.5
    assert abs(_one_box([0.21, 0.3, 0.83, 0.7], h, w, fy)[1] - (0.75 * cy - 2.0)) < 1e-5


# ------------------------------------------------------------------------------------------------ the case list reaches what it says
def test_case_list_covers_the_shapes():
    lat = [R.CASES[n] for n in R.LATTICE]
    rnd = [R.CASES[n] for n in R.RANDOM]
    assert {c[1] for c in lat} == {(8, 8), (16, 16), (8, 16), (16, 8)}
    assert {c[1] for c in rnd} >= {(5, 7), (7, 5), (3, 16), (4, 17), (14, 14), (24, 24)} and R.RANDOM_POW2
    for cases in (lat, rnd):
        assert {c[2] for c in cases} >= {4, 260, 1024, 1028}
        assert {c[3] for c in cases} >= {1, 256, 257, 600}
        assert {c[5] for c in cases} == {0, 1} and 70 in {c[4] for c in cases}
    assert 0 in {c[3] for c in lat}
    for name in R.CASES:
        c = R.build_case(name)
        img = c["rois"][:, 0].astype(int)
        assert c["Ntok"] > c["tok_off"] + c["h"] * c["w"]                       # tokens after the grid
        assert c["B"] == 1 or (1 not in img and not c["ref"]["rounded"]["bwd"]["mag"][1].any())
        if c["B"] == 70:
            assert len(set(img)) <= 12 and c["K"] == 12
        if c["K"] >= 256:
            assert all((img[s:s + 64] == c["spread"]).any() for s in range(0, c["K"], 64)) and sorted(img) != list(img)


@pytest.mark.parametrize("name", R.MANY_BOXES)
def test_boxes_of_the_later_chunks_are_needed(name):
    """The gradient of the first 256 boxes alone is outside the bound of the whole gradient somewhere: a backward that stopped after
    its first chunk would be seen."""
    c = R.build_case(name)
    form = "rounded"
    geo = {k: (v[:256] if k != "form" else v) for k, v in c["ref"][form]["geo"].items()}
    part = R.backward_ref(c["dP"][:256], geo, c["B"], c["h"], c["w"])
    full = c["ref"][form]["bwd"]
    off = np.abs(part["d"] - full["d"]) > 2 * R.backward_bound(full, R.grid_of(c, c["prefill"]))
    assert off[c["spread"]].any() and off.mean() > 0.2
