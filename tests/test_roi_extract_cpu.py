"""CPU: the detector's RoI extractor (clipself_amd/roi_extractor.py, include/clipself_roi.h) without a GPU.

Known answers of the contract by hand; the two forms of the numpy restatement (tests/_roi_extract_ref.py) against each other; the torch
route, forward and autograd backward, against the restatement on the GPU file's case list -- bit for bit on the lattice cases, inside the
derived bound on the random ones; the reference's two extractor dicts and the unsupported options; every -1 case of the header through
the raw entry points (the header itself is held by tests/test_cabi_symbols.py)."""

import numpy as np
import pytest
import torch

import _roi_extract_ref as R

NAN, INF = float("nan"), float("inf")
STRIDES = [4, 8, 16, 32]


def _nchw(m):
    """[B, h, w, C] numpy -> [B, C, h, w] torch (channel-last strides)."""
    return torch.from_numpy(m).permute(0, 3, 1, 2)


def _pool(maps, rois, P=7, sampling_ratio=0, strides=STRIDES, finest_scale=56):
    """The torch route -> [K, P, P, C] numpy."""
    from clipself_amd import roi_extractor
    out = roi_extractor.roi_extract_torch([_nchw(m) for m in maps], torch.tensor(rois, dtype=torch.float32).reshape(-1, 5), P,
                                          sampling_ratio, strides, finest_scale)
    return out.permute(0, 2, 3, 1).numpy()


def _pyramid(fn, img=128, B=1, C=4, strides=STRIDES):
    """maps [B, h, w, C] with value fn(x_pixel, y_pixel) at each cell centre (cell i of stride s is centred at (i + 0.5) * s)."""
    maps = []
    for s in strides:
        n = img // s
        c = (np.arange(n) + 0.5) * s
        v = fn(c[None, :], c[:, None]) + np.zeros((n, n))
        maps.append(np.broadcast_to(v[None, :, :, None], (B, n, n, C)).astype(np.float32).copy())
    return maps


# ------------------------------------------------------------------------------------------------ known answers
def test_constant_map_pools_to_the_constant():
    maps = _pyramid(lambda x, y: 2.5)
    rois = [[0, 10.3, 20.7, 50.1, 90.2], [0, 3, 3, 120, 125], [0, 40, 40, 47, 47]]
    for P, sr in [(7, 0), (14, 0), (1, 0), (7, 2)]:
        out = _pool(maps, rois, P, sr, finest_scale=14)
        assert np.abs(out - 2.5).max() < 1e-5, (P, sr)


def test_linear_ramp_pools_to_its_value_at_the_bin_centres():
    """Bilinear interpolation reproduces a linear function and the samples of a bin are symmetric about its centre, so a bin holds
    f(bin centre); the boxes stay half a cell inside the map, where nothing is clamped."""
    a, b = 0.25, -0.5
    maps = _pyramid(lambda x, y: a * x + b * y)
    rois = np.array([[0, 12.0, 20.0, 60.0, 100.0], [0, 30.0, 30.0, 44.0, 51.0], [0, 16.0, 16.0, 112.0, 112.0]], np.float32)
    for P in (7, 14):
        out = _pool(maps, rois, P, finest_scale=14)
        for k, (_, x0, y0, x1, y1) in enumerate(rois):
            cx = x0 + (np.arange(P) + 0.5) * (x1 - x0) / P
            cy = y0 + (np.arange(P) + 0.5) * (y1 - y0) / P
            want = a * cx[None, :] + b * cy[:, None]
            assert np.abs(out[k, :, :, 0] - want).max() < 1e-3, (P, k)


def test_a_box_wholly_outside_pools_to_zero():
    maps = _pyramid(lambda x, y: 1.0)
    out = _pool(maps, [[0, 140, 140, 180, 180], [0, -60, 10, -10, 60], [0, 10, 300, 60, 350]], finest_scale=14)
    assert (out == 0).all()


def test_level_choice():
    from clipself_amd.roi_extractor import SingleRoIExtractor
    box = lambda s: [0, 10, 10, 10 + s, 10 + s]
    rois = np.array([box(112), box(111.9), box(448), box(1e4), [0, 50, 10, 10, 60], box(55.9), box(56), box(224), box(223.9)], np.float32)
    want = [1, 0, 3, 3, 0, 0, 0, 2, 1]
    assert R.roi_levels(rois, 4, 56).tolist() == want
    ex = SingleRoIExtractor(dict(type="RoIAlign", output_size=7, sampling_ratio=0), 4, STRIDES)
    assert ex.map_roi_levels(torch.from_numpy(rois), 4).tolist() == want
    assert ex.map_roi_levels(torch.from_numpy(rois), 2).tolist() == [min(v, 1) for v in want]
    maps = _pyramid(lambda x, y: 1.0, img=512)
    out = _pool(maps, rois[4:5], finest_scale=56)                              # negative area: level 0 and no samples
    assert (out == 0).all()


def test_level_boundaries_of_the_lattice_cases():
    """7 * 2^m squares at finest_scale 14: scale / 14 is exactly 2^(m - 1), and 2^j + 1e-6 stays above 2^j in fp32 up to j = 3 (1e-6 is four
    ulps of 2, one ulp of 8), so the + 1e-6 puts the box on the upper level."""
    rois = np.array([[0, 0, 0, 7 * 2.0 ** m, 7 * 2.0 ** m] for m in range(6)], np.float32)
    assert R.roi_levels(rois, 4, 14).tolist() == [0, 0, 1, 2, 3, 3]
    for j in range(4):
        assert np.float32(2.0 ** j) + np.float32(1e-6) > np.float32(2.0 ** j)


# ------------------------------------------------------------------------------------------------ the restatement's two forms
@pytest.mark.parametrize("sr", [0, 2])
def test_scalar_loops_equal_the_vectorised_form(sr):
    r = np.random.RandomState(3)
    grids = R.image_grids(64, 96, STRIDES)
    B, C, P = 2, 4, 3
    maps = [r.randn(B, h, w, C).astype(np.float32) for h, w in grids]
    rois = R.random_rois(12, B, 64, 96, 5)
    rois[3, 0], rois[4, 1], rois[5, 3] = 2, NAN, 1e6                            # hostile rows take the same path in both forms
    dout = r.randn(len(rois), P, P, C).astype(np.float32)
    fv, fl = R.forward_vec(maps, rois, STRIDES, P, sr, 14), R.forward_loops(maps, rois, STRIDES, P, sr, 14)
    assert np.abs(fv["out"] - fl).max() < 1e-13 and (fv["out"][3:6] == 0).all()
    bv, bl = R.backward_vec(dout, rois, grids, STRIDES, B, P, sr, 14), R.backward_loops(dout, rois, grids, STRIDES, B, P, sr, 14)
    for a, b in zip(bv["dmaps"], bl):
        assert np.abs(a - b).max() < 1e-13


# ------------------------------------------------------------------------------------------------ the torch route is the restatement
@pytest.mark.parametrize("name", R.LATTICE + R.RANDOM)
def test_torch_route_equals_the_restatement(name):
    from clipself_amd import roi_extractor
    c = R.build_case(name)
    if c["lattice"]:
        assert c["fwd"]["exact"] and c["bwd"]["exact"], "the lattice case is not exact in fp32: its draw is wrong"
    else:
        assert (R.level_margin(c["rois"], c["finest_scale"]) > 1e-4).all(), "a box sits on a level boundary: choose another seed"
    if c["K"] >= 300 and c["finest_scale"] == 14:
        assert len(set(c["fwd"]["levels"].tolist())) == len(c["strides"]), "finest_scale 14 reaches every level inside the image"
    feats = [_nchw(m).clone().requires_grad_(True) for m in c["maps"]]
    rois = torch.from_numpy(c["rois"])
    assert roi_extractor.map_roi_levels_torch(rois, len(feats), c["finest_scale"]).tolist() == c["fwd"]["levels"].tolist()
    out = roi_extractor.roi_extract(feats, rois, c["P"], c["sampling_ratio"], c["strides"], c["finest_scale"])
    assert out.shape == (c["K"], c["C"], c["P"], c["P"]) and out.dtype == torch.float32
    out.backward(_nchw(c["dout"]))
    grads = [(f.grad if f.grad is not None else torch.zeros_like(f)).permute(0, 2, 3, 1).numpy() for f in feats]
    R.check(c, out.detach().permute(0, 2, 3, 1).numpy(), grads, "torch route")


# ------------------------------------------------------------------------------------------------ configs and the module
BBOX_EXTRACTOR = dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                      featmap_strides=[4, 8, 16, 32])
MASK_EXTRACTOR = dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0), out_channels=256,
                      featmap_strides=[4, 8, 16, 32])


@pytest.mark.parametrize("cfg,P", [(BBOX_EXTRACTOR, 7), (MASK_EXTRACTOR, 14)])
@pytest.mark.parametrize("strides", [[4, 8, 16, 32], [3.5, 7, 14, 28]])
def test_the_references_extractor_dicts_build(cfg, P, strides):
    from clipself_amd import roi_extractor
    cfg = dict(cfg, featmap_strides=strides)
    assert cfg.pop("type") == "SingleRoIExtractor"
    ex = roi_extractor.SingleRoIExtractor(**cfg)
    assert ex.num_inputs == 4 and ex.output_size == P and ex.sampling_ratio == 0 and ex.finest_scale == 56 and ex.out_channels == 256
    img = 112
    feats = [torch.randn(2, 256, int(img / s), int(img / s), generator=torch.Generator().manual_seed(i)) for i, s in enumerate(strides)]
    rois = roi_extractor.bbox2roi([torch.tensor([[5., 6, 40, 50, 0.9], [10, 10, 100, 90, 0.8]]), torch.tensor([[0., 0, 30, 20, 0.7]])])
    assert rois.tolist() == [[0, 5, 6, 40, 50], [0, 10, 10, 100, 90], [1, 0, 0, 30, 20]]
    out = ex(feats + [torch.zeros(2, 256, 1, 1)], rois)                        # a fifth map (the RPN's extra level) is ignored: x[:num_inputs]
    assert out.shape == (3, 256, P, P) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert ex(feats, torch.zeros(0, 5)).shape == (0, 256, P, P)


def test_unsupported_options_raise_naming_the_option():
    from clipself_amd.roi_extractor import SingleRoIExtractor
    layer = dict(type="RoIAlign", output_size=7, sampling_ratio=0)
    for kw, word in [(dict(roi_layer=dict(layer, aligned=False)), "aligned"), (dict(roi_layer=dict(layer, pool_mode="max")), "pool_mode"),
                     (dict(roi_layer=dict(layer, type="RoIPool")), "RoIPool"), (dict(roi_layer=dict(layer, type="DeformRoIPoolPack")), "type"),
                     (dict(roi_layer=layer, featmap_strides=[4, 8, 16, 32, 64]), "levels"), (dict(roi_layer=dict(layer, output_size=15)), "output_size"),
                     (dict(roi_layer=dict(layer, sampling_ratio=9)), "sampling_ratio"), (dict(roi_layer=dict(layer, output_size=(7, 14))), "output_size")]:
        with pytest.raises(ValueError, match=word):
            SingleRoIExtractor(**dict(dict(out_channels=8, featmap_strides=STRIDES), **kw))
    ex = SingleRoIExtractor(dict(layer, use_torchvision=True, aligned=True, pool_mode="avg"), 8, STRIDES)      # accepted and ignored
    feats = [torch.zeros(1, 8, 64 // s, 64 // s) for s in STRIDES]
    with pytest.raises(ValueError, match="roi_scale_factor"):
        ex(feats, torch.zeros(1, 5), roi_scale_factor=1.5)
    with pytest.raises(ValueError):
        ex(feats[:3], torch.zeros(1, 5))
    with pytest.raises(ValueError):
        ex(feats, torch.zeros(1, 4))


def test_hostile_boxes_pool_to_zero_on_the_torch_route():
    maps = _pyramid(lambda x, y: 1.0, B=2)
    rois = [[-1, 10, 10, 50, 50], [2, 10, 10, 50, 50], [NAN, 10, 10, 50, 50], [0, NAN, 10, 50, 50], [0, 10, 10, INF, 50], [0, -INF, 10, INF, 50],
            [0, 50, 10, 10, 50], [0, 0, 0, 1e6, 1e6], [1, 10, 10, 50, 50]]
    out = _pool(maps, rois, finest_scale=14)
    assert (out[:8] == 0).all() and np.abs(out[8] - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the C ABI
def test_limits_are_refused_without_a_device():
    """Argument checks come before any launch, so the -1 cases can be seen here: no pointer is touched."""
    from clipself_amd import hip
    lib = hip.load_library()
    assert lib.csr_roi_extract_workspace(-1) == 0 and lib.csr_roi_extract_workspace(300) == 300 * 64 + 300 * 4 + 32768

    def call(L=4, B=2, C=8, K=10, P=7, sr=0, fs=56.0, ldo=8, h=16, w=16, ld=8, scale=0.25, ptr=1 << 20, bwd=False, ws=1 << 20):
        arr = (hip.RoiLevel * max(L, 1))(*[hip.RoiLevel(ptr, ld, h, w, scale) for _ in range(max(L, 1))])
        if bwd:
            return lib.csr_roi_extract_bwd(1 << 20, ldo, 1 << 20, K, P, sr, fs, arr, L, B, C, ws, None)
        return lib.csr_roi_extract_fwd(arr, L, B, C, 1 << 20, K, P, sr, fs, 1 << 20, ldo, None)

    for kw, word in [(dict(L=0), b"L ="), (dict(L=5), b"L ="), (dict(B=0), b"B ="), (dict(C=6), b"C ="), (dict(C=0), b"C ="), (dict(K=-1), b"K ="),
                     (dict(P=15), b"P ="), (dict(P=0), b"P ="), (dict(sr=9), b"sampling_ratio"), (dict(sr=-1), b"sampling_ratio"),
                     (dict(fs=0.0), b"finest_scale"), (dict(fs=NAN), b"finest_scale"), (dict(ldo=4), b"ldo"), (dict(ldo=10), b"ldo"),
                     (dict(h=513), b"grid"), (dict(w=0), b"grid"), (dict(ld=4), b"row stride"), (dict(scale=0.0), b"spatial_scale"),
                     (dict(scale=INF), b"spatial_scale"), (dict(ptr=(1 << 20) + 4), b"aligned"), (dict(bwd=True, ws=None), b"workspace")]:
        for bwd in ((True,) if kw.get("bwd") else (False, True)):
            assert call(**dict(kw, bwd=bwd)) == -1, kw
            assert word in lib.cs_last_error(), (kw, lib.cs_last_error())
    assert call(K=0) == 0 and call(K=0, bwd=True) == 0                      # nothing to do is not an error, and launches nothing
