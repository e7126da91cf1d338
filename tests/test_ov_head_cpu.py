"""CPU: clipself_amd.ov_head.OpenVocabBoxScores on its fallback route (the CPU reference backend + torch) against the float64 restatement
of the reference's scoring tail (tests/_ov_head_ref.py), known answers in closed form, loading and errors, the teeth of the bound, and the
bookkeeping of cs_roialign_fwd's grown argument list.  The map is 8 x 8 at stride 16, so that the fallback's conversion of pixel boxes to
the normalised form is exact (ov_head.py's module docstring)."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _ov_head_ref import F32, check, make_case, needle_case, reference, split_exponents, worst_ratio
from oracle.ops_ref import RefOps

ROOT = Path(__file__).resolve().parent.parent
B, H, W, E, STRIDE = 2, 8, 8, 64, 16
NAMES = [f"class{i}" for i in range(65)]                   # + 'background' = 66, OV-COCO's count


def _module(embed, **kw):
    from clipself_amd.ov_head import OpenVocabBoxScores
    kw.setdefault("ops", RefOps())
    return OpenVocabBoxScores(embed, **kw).eval()


def _nchw(feat):
    return feat.permute(0, 3, 1, 2)


def _ovcoco(seed=1, K=12, **kw):
    feat, rois, embed, det = make_case(B, H, W, E, 66, K, seed, STRIDE)
    w = split_exponents(66, 0.2, 0.45)
    seen = [n for i, n in enumerate(NAMES) if float(w[i]) == np.float32(0.2)]
    m = _module(embed, seen_classes=seen, all_classes=NAMES, alpha=0.2, beta=0.45, **kw)
    assert torch.equal(m.exponents(), w) and bool(m.base_idx[-1]) and int(m.novel_idx.sum()) == int((w != w[0]).sum())
    return m, feat, rois, det


def _reference_of(m, feat, rois, det, embed=None):
    embed = m.all_embed.detach().float().t().contiguous() if embed is None else embed
    return reference(feat, rois, 1.0 / STRIDE, embed, m.vlm_temperature, det, None if det is None else m.exponents(), pool_terms="samples")


EMPTY_BOXES = torch.tensor([[-1.0, 8, 8, 72, 72], [2.0, 8, 8, 72, 72], [0.0, 0, 0, 1e9, 40], [1.0, 8, float("nan"), 72, 72],
                            [0.0, 90, 20, 30, 70], [1.0, 300, 300, 340, 350], [0.0, 8, 8, 72, 72]])      # ..., x1 < x0, off the map, a valid one


def _cases():
    m, feat, rois, det = _ovcoco()
    yield "ov-coco", m, feat, rois, det
    feat, rois, embed, det = make_case(B, H, W, E, 21, 9, 2, STRIDE)
    yield "transfer", _module(embed, alpha=0.3, fixed_temperature=50.0), feat, rois, det
    m, feat, rois, det = _ovcoco(seed=3, learn_bg=True)
    with torch.no_grad():
        m.bg_embedding.add_(0.05 * torch.randn(E, 1, generator=torch.Generator().manual_seed(4)))
    yield "learn_bg", m, feat, rois, det
    m, feat, rois, det = _ovcoco(seed=5)
    yield "vlm-only", m, feat, rois, None
    m, feat, _, det = _ovcoco(seed=6, K=len(EMPTY_BOXES))
    yield "empty boxes", m, feat, EMPTY_BOXES, det


CASES = {name: rest for name, *rest in _cases()}


@pytest.mark.parametrize("name", CASES)
def test_fallback_route_equals_the_restatement(name):
    m, feat, rois, det = CASES[name]
    assert not m.fused
    ref = _reference_of(m, feat, rois, det)
    got = m(det, _nchw(feat), rois)
    assert got.dtype == F32 and tuple(got.shape) == (len(rois), m.all_embeddings.shape[1])
    check(name, got, ref)
    if det is None:
        assert torch.allclose(got.sum(1), torch.ones(len(rois)), atol=1e-4)
    if name == "empty boxes":
        C = got.shape[1]
        uniform = reference(feat, rois[:1], 1.0 / STRIDE, m.all_embed.detach().t().contiguous(), m.vlm_temperature).out
        assert torch.allclose(uniform, torch.full((1, C), 1.0 / C, dtype=torch.float64), atol=0, rtol=1e-14)
        vlm = m(None, _nchw(feat), rois)
        assert torch.equal(vlm[:6], torch.full((6, C), 1.0 / C)) and not torch.equal(vlm[6], vlm[0])
        assert torch.equal(m.vlm_box_feats(_nchw(feat), rois)[:6], torch.zeros(6, E))


def test_learn_bg_changes_the_background_column_only():
    m, feat, rois, det = CASES["learn_bg"]
    assert torch.equal(m.all_embed[:, :-1], m.all_embeddings[:, :-1]) and not torch.equal(m.all_embed[:, -1], m.all_embeddings[:, -1])
    assert abs(float(m.all_embed[:, -1].detach().norm()) - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------ known answers
def test_basis_map_and_orthonormal_classes_give_the_closed_form():
    C, j, T = 7, 3, 5.0
    feat = torch.zeros(B, H, W, E)
    feat[..., j] = 1.0
    embed = torch.eye(E)[:C].contiguous()
    rois = torch.tensor([[0.0, 10, 20, 90, 100], [1.0, 3, 5, 17, 11], [1.0, 0, 0, 128, 128]])
    m = _module(embed, vlm_temperature=T)
    ref = reference(feat, rois, 1.0 / STRIDE, embed, T, pool_terms="samples")
    pj = math.exp(T) / (math.exp(T) + C - 1)
    want = torch.full((3, C), (1 - pj) / (C - 1), dtype=torch.float64)
    want[:, j] = pj
    assert torch.allclose(ref.out, want, rtol=1e-12, atol=0)                            # the restatement itself
    check("basis map", m(None, _nchw(feat), rois), ref)


def test_needle_class_wins_on_its_box_and_loses_beside_it():
    feat, rois, embed = needle_case(B, H, W, E)
    m = _module(embed)
    got = m(None, _nchw(feat), rois)
    assert got.argmax(1).tolist() == [1, 0, 0]
    assert float(got[0, 1]) > 0.99 and float(got[1, 1]) < 1e-6 and float(got[2, 1]) < 1e-6
    check("needle", got, reference(feat, rois, 1.0 / STRIDE, embed, m.vlm_temperature, pool_terms="samples"))


# ------------------------------------------------------------------------------------------------ loading and errors
def test_embedding_files_and_reference_state_dict_load(tmp_path):
    _, _, embed, _ = make_case(B, H, W, E, 66, 1, 7, STRIDE)
    names = NAMES + ["background"]
    np.save(tmp_path / "embed.npy", embed.numpy())
    torch.save({n: embed[i] for i, n in reversed(list(enumerate(names)))}, tmp_path / "embed.pt")
    (tmp_path / "all.json").write_text(__import__("json").dumps(NAMES))
    (tmp_path / "seen.json").write_text(__import__("json").dumps(NAMES[::2]))
    want = F.normalize(embed.t().contiguous(), dim=0)
    for src in (embed, str(tmp_path / "embed.npy"), str(tmp_path / "embed.pt")):
        m = _module(src, seen_classes=str(tmp_path / "seen.json"), all_classes=str(tmp_path / "all.json"))
        assert tuple(m.all_embeddings.shape) == (E, 66) and torch.equal(m.all_embeddings, want)
        assert m.all_classes == names and int(m.base_idx.sum()) == 34 and bool(m.base_idx[-1])
        assert isinstance(m.detect_temperature, torch.nn.Parameter) and float(m.detect_temperature) == 50.0
    with pytest.raises(ValueError):
        _module(str(tmp_path / "embed.pt"))                                           # a dict needs the row order
    with pytest.raises(ValueError):
        _module(embed[:5], all_classes=NAMES)
    # the entry of a reference head's state dict: all_embeddings [E, C]
    other = F.normalize(torch.randn(E, 66, generator=torch.Generator().manual_seed(8)), dim=0)
    before = m._embed_rows()
    assert m._embed_rows() is before                                                    # cached while the source is unchanged
    missing = m.load_state_dict({"all_embeddings": other}, strict=False)
    assert missing.unexpected_keys == [] and torch.equal(m.all_embeddings, other)
    assert torch.equal(m._embed_rows(), other.t()) and m._embed_rows().is_contiguous()
    x = torch.randn(4, E, generator=torch.Generator().manual_seed(9), requires_grad=True)
    logits = m.class_logits(x)
    assert torch.allclose(logits, F.normalize(x, dim=-1) @ other * 50.0, atol=1e-5)
    logits.sum().backward()
    assert x.grad is not None and m.detect_temperature.grad is not None


def test_fused_needs_the_capability_and_forward_needs_eval():
    m, feat, rois, det = CASES["ov-coco"]
    with pytest.raises(NotImplementedError, match="BOX_SCORES"):
        _module(torch.eye(8), fused=True)
    assert not _module(torch.eye(8), fused=None).fused
    m.train()
    try:
        with pytest.raises(AssertionError):
            m(det, _nchw(feat), rois)
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------ the bound has teeth
@pytest.mark.parametrize("name", CASES)
def test_restatement_stays_inside_its_own_bound(name):
    m, feat, rois, det = CASES[name]
    ref = _reference_of(m, feat, rois, det)
    worst, bad = worst_ratio(ref.out.float(), ref)                                      # the float64 scores rounded to fp32
    assert bad == 0 and worst < 1.0, (name, worst)


def test_bf16_embeddings_break_the_bound():
    broken = []
    for name, (m, feat, rois, det) in CASES.items():
        ref = _reference_of(m, feat, rois, det)
        rows = m.all_embed.detach().float().t().contiguous()
        worst, bad = worst_ratio(_reference_of(m, feat, rois, det, embed=rows.bfloat16().float()).out, ref)
        print(f"bf16 embeddings, {name}: worst err / bound {worst:.1f}, {bad} scores past it")
        if bad:
            broken.append(name)
    assert "ov-coco" in broken and "transfer" in broken and "vlm-only" in broken, broken


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def _header_args(symbol):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "clipself_hip.h").read_text(), flags=re.S)
    return [a.strip() for a in re.search(symbol + r"\s*\(([^)]*)\)", text).group(1).split(",")]


def test_signature_table_matches_the_header():
    from clipself_amd import hip
    args = _header_args("cs_roialign_fwd")
    assert len(hip.SIGNATURES["cs_roialign_fwd"][1]) == len(args) == 20
    assert [a.split()[-1].lstrip("*") for a in args[9:]] == ["box_scale", "B", "class_embed", "C", "vlm_temp", "det_logits", "ldd", "expo", "scores",
                                                            "lds", "stream"]
    assert hip.HipOps.BOX_SCORES and len(hip.SIGNATURES) == 51


class _Recorder:
    def __init__(self):
        self.calls = []

    def cs_roialign_fwd(self, *args):
        self.calls.append(args)
        return 0


def _bare_ops():
    from clipself_amd import hip
    ops = hip.HipOps.__new__(hip.HipOps)
    ops.lib, ops._chk, ops._stream = _Recorder(), (lambda *ts: None), (lambda: 0)
    return ops


def test_old_form_call_passes_the_neutral_trailing_values():
    ops = _bare_ops()
    feat, rois, pooled = torch.zeros(2, 65, 64), torch.zeros(3, 5), torch.zeros(3, 64)
    ops.roialign_fwd(feat, rois, pooled, 8, 8, 1)
    assert ops.lib.calls[-1] == (feat.data_ptr(), rois.data_ptr(), pooled.data_ptr(), 3, 65, 8, 8, 64, 1, 0.0, 0, None, 0, 0.0, None, 0, None, None, 0, 0)
    ops.roialign_fwd(feat, rois, pooled, 8, 8, 1, box_scale=0.0625)
    assert ops.lib.calls[-1][9:11] == (0.0625, 2) and ops.lib.calls[-1][11:] == (None, 0, 0.0, None, 0, None, None, 0, 0)
    with pytest.raises(TypeError):
        ops.roialign_fwd(feat, rois, pooled, 8, 8, 1, 0.0625)                           # keyword only


def test_box_scores_wrapper_lays_out_the_call():
    ops = _bare_ops()
    dense = torch.zeros(2, 65, 64)
    view = dense[:, 1:].reshape(2, 8, 8, 64)                                            # the tower's map past CLS, in place
    rois, embed, scores = torch.zeros(5, 5), torch.zeros(7, 64), torch.zeros(5, 12)[:, :7]
    det, expo = torch.zeros(5, 9)[:, :7], torch.zeros(7)
    ops.box_scores(view, rois, embed, scores, 8, 8, 0, 0.0625, 100.0, det_logits=det, expo=expo)
    assert ops.lib.calls[-1] == (view.data_ptr(), rois.data_ptr(), None, 5, 65, 8, 8, 64, 0, 0.0625, 2, embed.data_ptr(), 7, 100.0,
                                 det.data_ptr(), 9, expo.data_ptr(), scores.data_ptr(), 12, 0)
    assert view.data_ptr() == dense.data_ptr() + 64 * 4
    with pytest.raises(AssertionError):
        ops.box_scores(view, rois, embed, scores, 8, 8, 0, 0.0625, 100.0, det_logits=det)          # det_logits without expo
    with pytest.raises(AssertionError):
        ops.box_scores(view.permute(0, 2, 1, 3), rois, embed, scores, 8, 8, 0, 0.0625, 100.0)      # not the token-major layout
