"""`-m gpu`: the detector's RoI extractor on the MI355X (csr_roi_extract_fwd / csr_roi_extract_bwd, HipOps.roi_extract_*,
clipself_amd/roi_extractor.py).

Every case of tests/_roi_extract_ref.CASES, forward and backward, against the float64 numpy restatement: the lattice cases (integer maps
and gradients, box sides 7 * 2^m on quarter-stride origins) bit for bit -- every weight is dyadic and every sum exact in fp32 in any
order, which the restatement checks on its own terms -- and the random ones (real-valued corners, strides 3.5 .. 28, sampling_ratio 0
and 2) inside the bound derived there, (taps + 4) 2^-24 sum |w f| / count per element; a wrong level shows as a wrong output, and the
random draws keep scale / finest_scale 1e-4 away from every power of two.  Shapes are the smallest that reach every path of
roi_extract.hip: C = 4 / 64 / 260 (one float4, one wave, two channel chunks of the backward with a ragged second one), P = 1 / 7 / 14,
K = 0 / 1 / 5 / 300 (the backward scans boxes 64 at a time), 24 x 40 maps against an h / w swap, 3 x 5 maps below one 4 x 4 tile, one
image without a box, shuffled rows.  Then hostile boxes, equal bits from equal inputs, the -1 cases through the wrapper, read / write
extents inside the poisoned halos of tests/_extents.py, and the module on CUDA tensors against its torch route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _roi_extract_ref as R  # noqa: E402
from _extents import run_case  # noqa: E402

F32 = torch.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _rows(m):
    """[B, h, w, C] numpy -> its 2-D view [B * h * w, C] on the device."""
    return torch.from_numpy(np.ascontiguousarray(m)).cuda().reshape(-1, m.shape[-1])


def _run(hip, c, rois=None, dout=None):
    """-> (out [K, P, P, C], dmaps: L arrays [B, h, w, C]) of the two entry points on compact tensors, as numpy."""
    rois = c["rois"] if rois is None else rois
    dout = c["dout"] if dout is None else dout
    K, P, C, B = len(rois), c["P"], c["C"], c["B"]
    scales = [1.0 / s for s in c["strides"]]
    r = torch.from_numpy(rois).cuda()
    out = torch.full((K * P * P, C), NAN, dtype=F32, device="cuda")
    hip.roi_extract_fwd([_rows(m) for m in c["maps"]], c["grids"], scales, r, out, B, P, c["sampling_ratio"], c["finest_scale"])
    dmaps = [torch.zeros(B * h * w, C, dtype=F32, device="cuda") for h, w in c["grids"]]
    hip.roi_extract_bwd(_rows(dout), r, dmaps, c["grids"], scales, B, P, c["sampling_ratio"], c["finest_scale"])
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(K, P, P, C), [d.cpu().numpy().reshape(B, h, w, C) for d, (h, w) in zip(dmaps, c["grids"])]


@pytest.mark.parametrize("name", R.LATTICE + R.RANDOM)
def test_kernels_equal_the_restatement(hip, name):
    """Worst fraction of the bound measured on the MI355X: profiles/roi_extract_parity.md."""
    c = R.build_case(name)
    if c["lattice"]:
        assert c["fwd"]["exact"] and c["bwd"]["exact"]
    else:
        excluded = int((R.level_margin(c["rois"], c["finest_scale"]) <= 1e-4).sum())
        assert excluded == 0, f"{excluded} boxes sit within 1e-4 of a level boundary"
    out, dmaps = _run(hip, c)
    if c["empty_image"] is not None:
        assert all(not d[c["empty_image"]].any() for d in dmaps)
    f, b = R.check(c, out, dmaps, "kernels")
    print(f"PARITY {name}: forward {f:.3f} backward {b:.3f} of the bound")


def test_more_images_than_bins(hip):
    """The backward sorts boxes into (image % 1024, level) bins: images 3 and 1027 share one, and a tile must take only its own."""
    B, C, P, K = 1030, 4, 7, 12
    r = np.random.RandomState(21)
    rois = R.random_rois(K, 1, 8, 8, 22, smin=2.0, smax=8.0)
    rois[:, 0] = [3, 1027, 0, 1029, 1027, 3, 1024, 0, 1, 1025, 3, 1027]
    c = dict(name="many_images", lattice=False, strides=[4], grids=[(2, 2)], B=B, C=C, P=P, K=K, sampling_ratio=0, finest_scale=56, rois=rois,
             maps=[r.randn(B, 2, 2, C).astype(np.float32)], dout=r.randn(K, P, P, C).astype(np.float32), empty_image=2)
    c["fwd"] = R.forward_vec(c["maps"], rois, c["strides"], P, 0, 56)
    c["bwd"] = R.backward_vec(c["dout"], rois, c["grids"], c["strides"], B, P, 0, 56)
    out, dmaps = _run(hip, c)
    R.check(c, out, dmaps, "kernels")
    assert dmaps[0][3].any() and dmaps[0][1027].any() and not np.array_equal(dmaps[0][3], dmaps[0][1027])


def test_no_boxes(hip):
    c = dict(R.build_case("lattice_wide"))
    out, dmaps = _run(hip, c, rois=np.zeros((0, 5), np.float32), dout=np.zeros((0, c["P"], c["P"], c["C"]), np.float32))
    assert out.shape[0] == 0 and all(not d.any() for d in dmaps)


def test_hostile_boxes_pool_to_zero_and_send_no_gradient(hip):
    c = dict(R.build_case("random_big"))
    good = c["rois"][:40].copy()
    box = good[0, 1:].tolist()
    hostile = np.array([[-1] + box, [c["B"]] + box, [NAN] + box, [0, NAN] + box[1:], [0, box[0], box[1], INF, box[3]],
                        [0, -INF, box[1], INF, box[3]], [0, box[0], NAN, box[2], INF], [0, box[2], box[1], box[0], box[3]],
                        [0, 0, 0, 1e6, 1e6], [0, -1e6, 10, 20, 30], [0, 3e38, 3e38, 3.2e38, 3.2e38]], np.float32)
    rois = np.concatenate([good[:20], hostile, good[20:]])
    dout = c["dout"][:len(rois)]
    c.update(rois=rois, K=len(rois), dout=dout, fwd=R.forward_vec(c["maps"], rois, c["strides"], c["P"], 0, c["finest_scale"]),
             bwd=R.backward_vec(dout, rois, c["grids"], c["strides"], c["B"], c["P"], 0, c["finest_scale"]))
    out, dmaps = _run(hip, c)
    assert not out[20:20 + len(hostile)].any()
    R.check(c, out, dmaps, "kernels, hostile rows")                            # finite everywhere, and the other rows are still right
    keep = np.r_[0:20, 20 + len(hostile):len(rois)]
    _, alone = _run(hip, c, rois=rois[keep], dout=dout[keep])
    for a, b in zip(dmaps, alone):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))              # the hostile rows sent nothing


def test_two_backward_launches_give_equal_bits(hip):
    for name in ("random_big", "random_l14"):
        c = R.build_case(name)
        (o1, d1), (o2, d2) = _run(hip, c), _run(hip, c)
        assert np.array_equal(o1.view(np.int32), o2.view(np.int32))
        for a, b in zip(d1, d2):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), name


def test_arguments_outside_the_limits_are_refused_and_touch_nothing(hip):
    B, h, w, K = 1, 8, 8, 3
    rois = torch.tensor([[0, 2.0, 2, 20, 20]] * K, device="cuda")

    def attempt(C=8, P=7, L=1):
        maps = [torch.ones(B * h * w, C, device="cuda") for _ in range(L)]
        out = torch.full((K * P * P, C), 7.0, device="cuda")
        dmaps = [torch.full((B * h * w, C), 7.0, device="cuda") for _ in range(L)]
        args = ([(h, w)] * L, [0.25] * L)
        with pytest.raises((RuntimeError, ValueError)):
            hip.roi_extract_fwd(maps, *args, rois, out, B, P)
        with pytest.raises((RuntimeError, ValueError)):
            hip.roi_extract_bwd(torch.ones_like(out), rois, dmaps, *args, B, P)
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and all(bool((d == 7).all()) for d in dmaps)

    attempt(C=6)
    attempt(P=15)
    attempt(L=5)
    with pytest.raises(ValueError):                                            # a map that is not [B * h * w, C]
        hip.roi_extract_fwd([torch.ones(B * h * w + 1, 8, device="cuda")], [(h, w)], [0.25], rois, torch.zeros(K * 49, 8, device="cuda"), B, 7)


@pytest.mark.parametrize("pad", [8, 64])
def test_extents_inside_poisoned_halos(hip, pad):
    c = R.build_case("lattice_big")
    K, P, C, B = c["K"], c["P"], c["C"], c["B"]
    scales = [1.0 / s for s in c["strides"]]
    seeds = [torch.from_numpy(np.random.RandomState(7 + l).randint(-8, 9, (B * h * w, C)).astype(np.float32)) for l, (h, w) in enumerate(c["grids"])]

    def fn(ops, a):
        rois = a.inp(torch.from_numpy(c["rois"]))
        maps = [a.inp(torch.from_numpy(m).reshape(-1, C), a.ld(C, 4)) for m in c["maps"]]
        out = a.out((K * P * P, C), F32, a.ld(C, 4), name="out")
        ops.roi_extract_fwd(maps, c["grids"], scales, rois, out, B, P, c["sampling_ratio"], c["finest_scale"])
        dout = a.inp(torch.from_numpy(c["dout"]).reshape(-1, C), a.ld(C, 4))
        dmaps = [a.out((B * h * w, C), F32, a.ld(C, 4), init=s, name=f"dmaps{l}") for l, ((h, w), s) in enumerate(zip(c["grids"], seeds))]
        ops.roi_extract_bwd(dout, rois, dmaps, c["grids"], scales, B, P, c["sampling_ratio"], c["finest_scale"],
                            workspace=a.ws(ops.roi_extract_workspace(K)))
        return dict(out=out, **{f"dmaps{l}": d for l, d in enumerate(dmaps)})

    problems = run_case(hip, fn, "cuda", pad, key="roi_extract[lattice_big]")
    assert not problems, "\n".join(problems)


def test_module_on_cuda_tensors_against_its_torch_route(hip, monkeypatch):
    from clipself_amd import roi_extractor
    c = R.build_case("random_l14")
    calls = []
    real_f, real_b = type(hip).roi_extract_fwd, type(hip).roi_extract_bwd
    monkeypatch.setattr(type(hip), "roi_extract_fwd", lambda self, *a, **k: (calls.append("fwd"), real_f(self, *a, **k))[1])
    monkeypatch.setattr(type(hip), "roi_extract_bwd", lambda self, *a, **k: (calls.append("bwd"), real_b(self, *a, **k))[1])
    ex = roi_extractor.SingleRoIExtractor(dict(type="RoIAlign", output_size=c["P"], sampling_ratio=c["sampling_ratio"]), c["C"], c["strides"],
                                          finest_scale=c["finest_scale"], ops=hip)
    rois = torch.from_numpy(c["rois"])
    nchw = [torch.from_numpy(m).permute(0, 3, 1, 2).contiguous() for m in c["maps"]]           # what an FPN of nn.Conv2d hands over
    up = torch.from_numpy(c["dout"]).permute(0, 3, 1, 2).contiguous()
    res = {}
    for tag, dev, fmt in [("cpu", "cpu", torch.contiguous_format), ("nchw", "cuda", torch.contiguous_format), ("cl", "cuda", torch.channels_last)]:
        feats = [f.clone().to(dev).contiguous(memory_format=fmt).requires_grad_(True) for f in nchw]
        out = ex(feats, rois.to(dev))
        out.backward(up.to(dev))
        res[tag] = (out.detach(), [f.grad if f.grad is not None else torch.zeros_like(f) for f in feats])
    assert calls == ["fwd", "bwd", "fwd", "bwd"]                                # CUDA tensors ran the kernels, the CPU copy did not
    out = res["cl"][0]
    assert out.shape == (c["K"], c["C"], c["P"], c["P"]) and out.is_contiguous(memory_format=torch.channels_last)
    assert all(g.shape == f.shape and g.is_contiguous(memory_format=torch.channels_last) for g, f in zip(res["cl"][1], nchw))
    assert torch.equal(res["nchw"][0], res["cl"][0]) and all(torch.equal(a, b) for a, b in zip(res["nchw"][1], res["cl"][1]))
    nhwc = lambda t: t.permute(0, 2, 3, 1).cpu().numpy()
    for tag in ("cl", "cpu"):                                                   # both routes inside the bound of the same restatement
        R.check(c, nhwc(res[tag][0]), [nhwc(g) for g in res[tag][1]], f"module [{tag}]")
    bf = [f.cuda().to(torch.bfloat16).requires_grad_(True) for f in nchw]       # force_fp32: bf16 maps are cast, the result is fp32
    out16 = ex(bf, rois.cuda())
    out16.sum().backward()
    assert out16.dtype == torch.float32 and bf[0].grad.dtype == torch.bfloat16 and bool(torch.isfinite(out16).all())
