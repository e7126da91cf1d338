"""`-m gpu`: open-vocabulary box scores in one launch (cs_roialign_fwd's scoring form, HipOps.box_scores) on the MI355X.

Scores against the float64 restatement of the reference's tail inside the derived per-element bound on log out (tests/_ov_head_ref.py);
pooling of pixel boxes bit for bit against the normalised-box kernel; the old call form bit for bit against outputs recorded before the
signature grew (tests/golden/roialign_oldform.npz); read / write extents inside the poisoned halos of tests/_extents.py; boxes an RPN may
emit (bad image index, absurd or non-finite extent) scored as empty boxes; equal bits from equal inputs; and OpenVocabBoxScores(fused=True)
fed by the backbone's own dense map, in place.  Shapes are the smallest at which the kernel can go wrong: odd E / 4, E = 512 (two boxes
per pooling pass), C of 1, below / at / above one wave and one workgroup of class threads, K of 0, 1 and across the 16-box groups."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _backbone_ref import FIXTURES, OUT_INDICES, backbone_cfg, load_fixture  # noqa: E402
from _extents import run_case  # noqa: E402
from _ov_head_ref import F32, check, check_pooled, make_case, needle_case, reference, split_exponents  # noqa: E402

B = 2
NAN = float("nan")
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _tokens(feat, tok_off):
    """[B, h, w, E] -> the token-major map [B, tok_off + h*w, E] on the device, NaN in the CLS row."""
    Bn, h, w, E = feat.shape
    t = torch.full((Bn, tok_off + h * w, E), NAN)
    t[:, tok_off:] = feat.reshape(Bn, h * w, E)
    return t.cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _score(hip, feat, rois, embed, scale, T, det, expo, tok_off, want_pooled=True):
    """One launch on padded rows (ldd = C + 3, lds = C + 5, sentinel / NaN in the padding) -> scores [K, C], pooled [K, E] | None."""
    _, h, w, E = feat.shape
    K, C = len(rois), embed.shape[0]
    scores = torch.full((K, C + 5), -7.0, device="cuda")
    d = None
    if det is not None:
        d = torch.full((K, C + 3), NAN, device="cuda")
        d[:, :C] = det.cuda()
        d = d[:, :C]
    pooled = torch.full((K, E), -7.0, device="cuda") if want_pooled else None
    hip.box_scores(_tokens(feat, tok_off), rois.cuda(), embed.cuda(), scores[:, :C], h, w, tok_off, scale, T, det_logits=d,
                   expo=None if det is None else expo.cuda(), pooled=pooled)
    torch.cuda.synchronize()
    assert bool((scores[:, C:] == -7.0).all()), "the padding of the scores' rows was written"
    return scores[:, :C].cpu(), None if pooled is None else pooled.cpu()


# (grid, E, C, K, tok_off, 1 / box_scale)
SHAPES = [((8, 8), 64, 1, 1, 0, 16), ((8, 8), 64, 5, 9, 1, 16), ((5, 7), 68, 66, 33, 1, 14), ((5, 7), 68, 67, 33, 0, 14),
          ((8, 8), 512, 66, 33, 0, 16), ((5, 7), 512, 1204, 9, 1, 16), ((8, 8), 64, 1204, 33, 0, 14), ((5, 7), 68, 5, 0, 1, 14),
          # E + C past what 16 / 8 / 4 boxes per workgroup hold in LDS: groups of 8, 4 and 1
          ((8, 8), 512, 2048, 9, 1, 16), ((5, 7), 68, 4900, 5, 0, 14), ((8, 8), 64, 10000, 3, 1, 16)]
_REF = {}


def _case(shape):
    """Inputs and the two references (blend, VLM-only) of a shape: computed once, shared, never modified."""
    if shape not in _REF:
        (h, w), E, C, K, tok_off, stride = shape
        feat, rois, embed, det = make_case(B, h, w, E, C, K, 100 + E + C + K, stride)
        expo = split_exponents(C, 0.2, 0.45)
        T, scale = 100.0, float(np.float32(1.0) / np.float32(stride))
        _REF[shape] = (feat, rois, embed, det, expo, T, scale, reference(feat, rois, scale, embed, T, det, expo),
                       reference(feat, rois, scale, embed, T))
    return _REF[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-E{s[1]}-C{s[2]}-K{s[3]}-off{s[4]}-s{s[5]}")
def test_scores_within_the_derived_bound(hip, shape):
    assert hip.BOX_SCORES
    feat, rois, embed, det, expo, T, scale, ref_blend, ref_vlm = _case(shape)
    name = f"grid {shape[0]} E {shape[1]} C {shape[2]} K {shape[3]} off {shape[4]} stride {shape[5]}"
    got, pooled = _score(hip, feat, rois, embed, scale, T, det, expo, shape[4])
    check_pooled(name, pooled, ref_blend)
    check(name + " blend", got, ref_blend)
    got, pooled = _score(hip, feat, rois, embed, scale, T, None, None, shape[4], want_pooled=False)
    check(name + " vlm-only", got, ref_vlm)
    if shape[3]:
        assert torch.allclose(got.sum(1), torch.ones(shape[3]), atol=1e-4)


def test_known_answers_on_the_hardware(hip):
    import math
    C, j, T, E = 7, 3, 5.0, 64
    feat = torch.zeros(B, 8, 8, E)
    feat[..., j] = 1.0
    embed = torch.eye(E)[:C].contiguous()
    rois = torch.tensor([[0.0, 10, 20, 90, 100], [1.0, 3, 5, 17, 11], [1.0, 0, 0, 128, 128]])
    got, _ = _score(hip, feat, rois, embed, 1 / 16, T, None, None, 1)
    pj = math.exp(T) / (math.exp(T) + C - 1)
    assert torch.allclose(got[:, j].double(), torch.full((3,), pj, dtype=torch.float64), rtol=1e-5)
    check("basis map", got, reference(feat, rois, 1 / 16, embed, T))
    feat, rois, embed = needle_case(B, 8, 8, 64)
    got, _ = _score(hip, feat, rois, embed, 1 / 16, 100.0, None, None, 0)
    assert got.argmax(1).tolist() == [1, 0, 0] and float(got[0, 1]) > 0.99 and float(got[1, 1]) < 1e-6
    check("needle", got, reference(feat, rois, 1 / 16, embed, 100.0))


@pytest.mark.parametrize("E", [64, 512])
def test_pixel_box_pooling_equals_the_normalised_box_kernel_bit_for_bit(hip, E):
    """box_scale = 1/16 on a 16 x 16 map (a 256-pixel image) and boxes on whole pixels: pixel * 1/16 and (pixel / 256) * 16 are the same
    float, so the new form must reproduce the existing kernel's pooling in every bit -- from box_scores and from roialign_fwd(box_scale=)."""
    g = torch.Generator().manual_seed(E)
    K = 21
    feat = torch.randn(B, 16, 16, E, generator=g)
    lo = torch.randint(-8, 200, (K, 2), generator=g).float()
    rois = torch.cat([(torch.arange(K) % B).float()[:, None], lo, lo + torch.randint(1, 120, (K, 2), generator=g).float()], dim=1)
    normed = rois.clone()
    normed[:, 1:] /= 256.0
    tokens = _tokens(feat, 1)
    want = torch.empty(K, E, device="cuda")
    hip.roialign_fwd(tokens, normed.cuda(), want, 16, 16, 1)
    got = torch.empty(K, E, device="cuda")
    hip.roialign_fwd(tokens, rois.cuda(), got, 16, 16, 1, box_scale=1 / 16)
    assert torch.equal(_bits(got), _bits(want))
    embed = torch.randn(5, E, generator=g)
    _, pooled = _score(hip, feat, rois, embed, 1 / 16, 100.0, None, None, 1)
    assert torch.equal(_bits(pooled), _bits(want)) and float(want.abs().max()) > 0


def test_old_call_form_gives_the_recorded_bits(hip):
    """roialign_fwd through the grown signature against the outputs the same call gave before the change (recorded on an MI355X)."""
    with np.load(GOLDEN / "roialign_oldform.npz") as g:
        for name in "abc":
            _, gh, gw, E, off, K = (int(v) for v in g[f"{name}_shape"])
            pooled = torch.full((K, E), NAN, device="cuda")
            hip.roialign_fwd(torch.from_numpy(g[f"{name}_feat"]).cuda(), torch.from_numpy(g[f"{name}_rois"]).cuda(), pooled, gh, gw, off)
            assert torch.equal(_bits(pooled), torch.from_numpy(g[f"{name}_pooled"]).view(torch.int32)), f"case {name}"


def _halo_case(shape, with_det):
    (h, w), E, C, K, tok_off, stride = shape
    feat, rois, embed, det, expo, T, scale = _case(shape)[:7]

    def fn(ops, a):
        t = torch.full((B, tok_off + h * w, E), NAN)
        t[:, tok_off:] = feat.reshape(B, h * w, E)
        scores = a.out((K, C), F32, ld=a.ld(C), name="scores")
        pooled = a.out((K, E), F32, name="pooled")
        ops.box_scores(a.inp(t), a.inp(rois), a.inp(embed), scores, h, w, tok_off, scale, T,
                       det_logits=a.inp(det, a.ld(C)) if with_det else None, expo=a.inp(expo) if with_det else None, pooled=pooled)
        return {"scores": scores, "pooled": pooled}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("with_det", [True, False], ids=["blend", "vlm-only"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5]], ids=["E64-C5", "E68-C67", "E512-C1204"])
def test_launch_stays_inside_its_extents(hip, shape, with_det, pad):
    key = f"box_scores[{shape},{with_det}]"
    problems = run_case(hip, _halo_case(shape, with_det), "cuda", pad, key=key)
    assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_boxes_an_rpn_may_emit_are_scored_as_empty(hip):
    (h, w), E, C = (8, 8), 64, 5
    feat, _, embed, det = make_case(B, h, w, E, C, 8, 77, 16)
    expo = split_exponents(C, 0.2, 0.45)
    rois = torch.tensor([[-1.0, 8, 8, 72, 72], [float(B), 8, 8, 72, 72], [0.0, 0, 0, 1e9, 40], [1.0, 8, NAN, 72, 72], [0.0, 90, 20, 30, 70],
                         [1.0, float("inf"), 8, float("inf"), 72], [1.0, 300, 300, 340, 350], [0.0, 8, 8, 72, 72]])
    vlm, pooled = _score(hip, feat, rois, embed, 1 / 16, 100.0, None, None, 1)
    assert torch.equal(pooled[:7], torch.zeros(7, E)) and float(pooled[7].abs().max()) > 0
    assert all(torch.equal(_bits(vlm[k]), _bits(vlm[0])) for k in range(7))             # the empty-box row, bit for bit
    assert torch.allclose(vlm[0], torch.full((C,), 1.0 / C), rtol=1e-6) and not torch.equal(vlm[7], vlm[0])
    check("rpn boxes vlm-only", vlm, reference(feat, rois, 1 / 16, embed, 100.0))
    got, _ = _score(hip, feat, rois, embed, 1 / 16, 100.0, det, expo, 1)
    check("rpn boxes blend", got, reference(feat, rois, 1 / 16, embed, 100.0, det, expo))


def test_equal_inputs_give_equal_bits(hip):
    feat, rois, embed, det, expo, T, scale = _case(SHAPES[5])[:7]
    a = _score(hip, feat, rois, embed, scale, T, det, expo, 1)
    b = _score(hip, feat, rois, embed, scale, T, det, expo, 1)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_entry_point_refuses_bad_forms(hip):
    f, r, p = torch.zeros(1, 17, 8, device="cuda"), torch.zeros(2, 5, device="cuda"), torch.zeros(2, 8, device="cuda")
    a, s, d, e = torch.zeros(3, 8, device="cuda"), torch.zeros(2, 3, device="cuda"), torch.zeros(2, 3, device="cuda"), torch.zeros(3, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()

    def call(pooled=p, scale=0.0625, Bn=1, embed=a, C=3, det=d, ldd=3, expo=e, scores=s, lds=3):
        return hip.lib.cs_roialign_fwd(P(f), P(r), P(pooled), 2, 17, 4, 4, 8, 1, scale, Bn, P(embed), C, 100.0, P(det), ldd, P(expo), P(scores), lds, None)
    assert call() == 0 and call(pooled=None) == 0 and call(det=None, expo=None) == 0 and call(embed=None, det=None, scores=None) == 0
    torch.cuda.synchronize()
    assert call(C=0) == -1 and b"C=0" in hip.lib.cs_last_error()
    assert call(ldd=2) == -1 and b"ldd" in hip.lib.cs_last_error()
    assert call(lds=2) == -1 and b"lds" in hip.lib.cs_last_error()
    assert call(expo=None) == -1 and b"expo" in hip.lib.cs_last_error()
    assert call(scores=None) == -1 and call(embed=None) == -1 and call(embed=None, det=None, scores=None, pooled=None) == -1
    assert call(scale=-1.0) == -1 and call(C=50000, ldd=50000, lds=50000) == -1 and b"LDS" in hip.lib.cs_last_error()


# ------------------------------------------------------------------------------------------------ the module on the backbone
def test_module_scores_the_backbones_own_map_in_place(hip, monkeypatch, tmp_path):
    from clipself_amd import fvit
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import factory
    from clipself_amd.ov_head import OpenVocabBoxScores
    from oracle.ops_ref import RefOps
    cfg = backbone_cfg()
    real = factory.get_tower_cfg
    monkeypatch.setattr(factory, "get_tower_cfg", lambda n: cfg if n == cfg.name else real(n))
    images, _, _, seed = load_fixture(FIXTURES[0])
    ckpt = tmp_path / "seed.pt"
    torch.save(seeded_visual_state(cfg, seed), ckpt)
    backbone = fvit.EvaCLIPViT(cfg.name, str(ckpt), out_indices=OUT_INDICES).cuda().eval()
    fmap = backbone(images.cuda())[-1]
    Bn, E, h, w = fmap.shape
    stride = backbone.patch_size
    assert (Bn, E, h, w) == (2, 64, 4, 4) and stride == 8
    _, rois, embed, det = make_case(Bn, h, w, E, 21, 19, 5, stride)
    head = OpenVocabBoxScores(embed, alpha=0.3, featmap_stride=stride, ops=hip, fused=True).cuda().eval()
    seen = []
    real_scores = hip.box_scores
    monkeypatch.setattr(hip, "box_scores", lambda feat, *a, **k: (seen.append((feat.data_ptr(), tuple(feat.stride()))), real_scores(feat, *a, **k))[1])
    det_dev, rois_dev = det.cuda(), rois.cuda()
    head(det_dev, fmap, rois_dev)                                                       # builds the cached [C, E] rows and exponents
    del seen[:]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = head(det_dev, fmap, rois_dev)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < fmap.numel() * 4, "a map-sized allocation: the map was copied"
    assert seen == [(fmap.data_ptr(), ((h * w + 1) * E, w * E, E, 1))]                   # the tower's token-major map past CLS, in place
    nhwc = fmap.detach().permute(0, 2, 3, 1).cpu().contiguous()
    ref = reference(nhwc, rois, 1.0 / stride, head._embed_rows().cpu(), head.vlm_temperature, det, head.exponents().cpu())
    check("module fused", got, ref)
    fallback = OpenVocabBoxScores(embed, alpha=0.3, featmap_stride=stride, ops=RefOps(), fused=False).eval()
    check("module fallback", fallback(det, fmap.cpu(), rois), reference(nhwc, rois, 1.0 / stride, head._embed_rows().cpu(), head.vlm_temperature,
                                                                         det, head.exponents().cpu(), pool_terms="samples"))
    # a contiguous NCHW map from elsewhere: one permute-copy, the same scores
    assert torch.equal(_bits(head(det.cuda(), fmap.contiguous(), rois.cuda())), _bits(got))
