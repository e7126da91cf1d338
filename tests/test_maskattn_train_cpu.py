"""CPU: training through mask-attention pooling (extract_type='v1' / encode_masks(mask_attn=True)) of the OpenAI-CLIP ViT family.

(1) the restatement's autograd (oracle/clip_vit_ref.extract_roi_features_v1) against gradients captured from the real reference
    (tests/golden/tiny_openai_maskattn_grad*.npz, made by tools/gen_golden_maskattn_grad.py);
(2) the engine schedule -- ClipVitEngine.mask_attn_pool(need_grad=True) / backward_mask_attn -- through CLIP(cfg, ops=RefOpsExtra()) and
    CLIPSelf() with args.extract_type = "v1" against the same vectors;
(3) RefOpsExtra.attn_bwd(extra) itself against fp64 autograd of the masked attention;
(4) the capability attribute that decides whether a tower trains through 'v1'."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _maskattn_ref import (RECIPES, RefOpsExtra, batch_for, build_pair, exact_passenger_grads, load_gold, oracle_grads, recipe_of, run_recipe)
from clipself_amd.config import tiny_openai_cfg
from clipself_amd.init import seeded_visual_state
from oracle.ops_ref import RefOps


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_gold(golden_dir)


def _grad_keys(gold, tag):
    return [(k, k[len(tag) + 5:]) for k in gold if k.startswith(tag + "grad/")]


# ------------------------------------------------------------------------------------------------ (1) oracle vs the reference
@pytest.mark.parametrize("tag", RECIPES)
def test_oracle_autograd_matches_reference_gradients(gold, tag):
    rec = recipe_of(gold, tag)
    cfg = tiny_openai_cfg(rec["quick"])
    assert gold[tag + "losses"][0] >= 0.5                          # a well-conditioned loss: the teacher comes from another seed
    loss, grads = oracle_grads(cfg, rec, batch_for(rec, 0))
    assert abs(loss - gold[tag + "losses"][0]) < 5e-6
    assert [str(n) for n in gold[tag + "grad_none"]] == ["logit_scale"]
    assert {n for n in grads if n.startswith("visual.")} == {str(n) for n in gold[tag + "trainable"]}
    keys = _grad_keys(gold, tag)
    assert len(keys) == {"blocks/": 6, "stem/": 9, "stem64/": 9, "all/": 32, "q/blocks/": 3}[tag]
    for k, n in keys:
        assert rel(grads[n], gold[k]) < 1e-4, n                   # the bound of test_oracle_three_steps_grads_and_adamw


# ------------------------------------------------------------------------------------------------ (2) engine schedule
@pytest.mark.parametrize("tag", RECIPES)
def test_engine_recipes_match_reference(gold, tag):
    rec = recipe_of(gold, tag)
    cfg = tiny_openai_cfg(rec["quick"])
    student, teacher = build_pair(cfg, rec, RefOpsExtra(), RefOps())
    eng, fired = student.visual.engine, []
    losses, first = run_recipe(student, teacher, rec, rec["steps"], hook=fired.append)
    # hooks in backward_dense's order, every step
    order = (["head"] if tag == "all/" else []) + list(range(cfg.layers - 1, -1, -1)) + (["stem"] if tag not in ("blocks/", "q/blocks/") else [])
    assert fired == order * rec["steps"]
    assert np.allclose(losses, gold[tag + "losses"], atol=5e-3), (losses, gold[tag + "losses"])
    # the trainable / frozen sets: exactly the reference's tensors carry a gradient (logit_scale has none there either)
    assert sorted(n for n in first if n.startswith("visual.")) == sorted(str(n) for n in gold[tag + "trainable"])
    assert "logit_scale" not in first and [str(n) for n in gold[tag + "grad_none"]] == ["logit_scale"]
    for k, n in _grad_keys(gold, tag):
        r = rel(first[n].reshape(gold[k].shape), gold[k])
        assert r < 2e-2, f"{n}: rel {r:.3e}"                       # measured <= 6.4e-3 through the reference ops (bf16-forward oracle: 3.9e-3)
    # unlike 'v2', the last block attends: the q and k rows of its in_proj receive a gradient
    C, last = cfg.width, f"visual.transformer.resblocks.{cfg.layers - 1}.attn.in_proj_"
    assert float(first[last + "weight"][:C].abs().max()) > 0 and float(first[last + "weight"][C:2 * C].abs().max()) > 0
    assert float(first[last + "bias"][:C].abs().max()) > 0
    if tag != "q/blocks/":
        assert float(np.abs(gold[tag + "grad/" + last + "bias"][:2 * C]).max()) > 0
    sd0 = seeded_visual_state(cfg, rec["seed_w"])
    finals = [k for k in gold if k.startswith(tag + "final/")]
    assert len(finals) == {"blocks/": 0, "q/blocks/": 0, "stem/": 5, "stem64/": 5, "all/": 8}[tag]
    for k in finals:
        n = k[len(tag) + 6:]
        w0 = sd0[n].reshape(gold[k].shape)                           # the UPDATE of three AdamW steps against the reference's
        assert rel(eng.p[n].reshape(gold[k].shape) - w0, torch.as_tensor(gold[k]) - w0) < 6e-2, n
    frozen = [n for n in eng.public_names() if n not in set(eng.trainable_names())]
    for n in frozen:
        assert torch.equal(eng.p[n], sd0[n].reshape(eng.p[n].shape)), n


def _setup(gold, tag="blocks/", ops=None):
    rec = recipe_of(gold, tag)
    cfg = tiny_openai_cfg(rec["quick"])
    student, teacher = build_pair(cfg, rec, ops or RefOpsExtra(), RefOps())
    return rec, cfg, student, teacher


def test_image_without_valid_boxes(gold):
    """One image of the batch has no valid box at all: its passengers are all padding -- the rois tensor the method builds has no row for
    it, extract_roi_features splits it into an empty list -- and contribute nothing: loss and gradients are those of the oracle on the other
    image alone (the restatement itself takes no image without masks)."""
    from clipself_amd.training.clipself import CLIPSelf
    rec, cfg, student, teacher = _setup(gold, "stem/")
    images, boxes, crops = batch_for(rec, 0)
    boxes[0, :, -1] = 0
    batch = (images, boxes, crops * (boxes[..., -1] > 0.5)[..., None, None, None])
    args = SimpleNamespace(multiscale=False, extract_type="v1", cosine_weight=1.0)
    out, _, _ = CLIPSelf()(batch, student, teacher, None, "cpu", None, False, args)
    out["loss_cosine"].backward()
    want_loss, want = oracle_grads(cfg, rec, tuple(t[1:] for t in batch))
    assert abs(float(out["loss_cosine"].detach()) - want_loss) < 5e-3
    grads = {n: p.grad for n, p in student.named_parameters() if p.grad is not None}
    for n in ("visual.positional_embedding", "visual.class_embedding", "visual.transformer.resblocks.1.attn.in_proj_weight",
              "visual.transformer.resblocks.0.mlp.c_fc.weight"):
        assert rel(grads[n].reshape(want[n].shape), want[n]) < 2e-2, n
    # the list form of the boxes gives the same features as the [K, 5] rois tensor
    with torch.no_grad():
        rois = torch.cat([torch.full((2, 1), 1.0), boxes[1, :2, :4]], dim=1)
        a = student.encode_pseudo_boxes(images, rois, extract_type="v1")
        b = student.encode_pseudo_boxes(images, [boxes[0, :0, :4], boxes[1, :2, :4]], extract_type="v1")
    assert a.shape == (2, cfg.embed_dim) and torch.equal(a, b)


def test_v2_forward_between_v1_forward_and_backward(gold):
    rec, cfg, student, teacher = _setup(gold)
    images, boxes, _ = batch_for(rec, 0)
    lists = [b[b[:, -1] > 0.5, :4] for b in boxes]
    eng = student.visual.engine

    def grads(interleave):
        eng.zero_grad()
        feats = student.encode_pseudo_boxes(images, lists, extract_type="v1")
        if interleave:
            v2 = student.encode_pseudo_boxes(images, lists, extract_type="v2")      # leaves its own context behind
            assert eng._ctx is not None
        feats.square().sum().backward()
        out = eng.grad.clone()
        if interleave:
            assert eng._ctx is not None                                        # untouched by the v1 backward ...
            eng.zero_grad()
            v2.sum().backward()                                                # ... and still good for its own
            assert eng._ctx is None and float(eng.grad.abs().max()) > 0
        return out

    assert torch.equal(grads(False), grads(True))
    assert eng._ctx_mask is None
    with pytest.raises(RuntimeError):
        eng.backward_mask_attn(torch.zeros(5, cfg.embed_dim))


def test_encode_masks_mask_attn_is_differentiable(gold):
    rec, cfg, student, _ = _setup(gold)
    images, _, _ = batch_for(rec, 0)
    gen = torch.Generator().manual_seed(5)
    masks = [torch.rand(3, 4, 4, generator=gen) > 0.5, torch.rand(1, 4, 4, generator=gen) > 0.5]
    pooled = student.encode_masks(images, masks, normalize=True, mask_attn=True)
    assert pooled.requires_grad and pooled.shape == (4, cfg.embed_dim)
    pooled[:, 0].sum().backward()
    p = dict(student.named_parameters())["visual.transformer.resblocks.1.attn.in_proj_weight"]
    assert p.grad is not None and float(p.grad.abs().max()) > 0
    with torch.no_grad():                                                      # the inference path computes the same features
        assert rel(student.encode_masks(images, masks, normalize=True, mask_attn=True), pooled.detach()) < 1e-2


# ------------------------------------------------------------------------------------------------ (3) the reference op itself
@pytest.mark.parametrize("image", [True, False])
def test_ref_ops_extra_attn_bwd_is_the_gradient(image):
    B, Q, Ntok, H, scale = 2, 5, 17, 2, 64 ** -0.5
    C, ops = H * 64, RefOpsExtra()
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g)
    qkv = rnd(B * Ntok, 3 * C).to(torch.bfloat16)
    qm, dom = (rnd(B * Q, C) * 2).to(torch.bfloat16), rnd(B * Q, C).to(torch.bfloat16)
    allow = (torch.rand(B * Q, Ntok, generator=g) < 0.5).to(torch.uint8)
    allow[:, 0] = 1
    allow[0] = 1                        # all-allowed
    allow[1, 1:] = 0                    # CLS only
    allow[2] = 0                        # no key at all
    dom[3] = 0                          # zero upstream gradient
    cos, sin = torch.ones(16, 64), torch.zeros(16, 64)
    om, lsem = torch.empty(B * Q, C, dtype=torch.bfloat16), torch.empty(B * H, Q)
    ops.attn_query_fwd(qm, qkv[:, C:], allow, om, B, Q, Ntok, H, scale, lse=lsem)
    plain = torch.empty_like(om)
    RefOps().attn_query_fwd(qm, qkv[:, C:], allow, plain, B, Q, Ntok, H, scale)
    keep = torch.ones(B * Q, dtype=torch.bool)
    keep[2] = False                                                            # the frozen RefOps answers NaN for a row without keys
    assert torch.equal(om[keep], plain[keep]) and float(om[2].abs().max()) == 0.0
    assert bool(torch.isinf(lsem.view(B, H, Q)[0, :, 2]).all()) and bool((lsem.view(B, H, Q)[0, :, 2] > 0).all())
    assert int(torch.isinf(lsem).sum()) == H
    o, lse, dout = torch.empty(B * Ntok, C, dtype=torch.bfloat16), torch.empty(B * H, Ntok), rnd(B * Ntok, C).to(torch.bfloat16)
    ops.attn_fwd(qkv, cos, sin, o, lse, B, Ntok, H, scale)
    dqkv, dq = torch.full((B * Ntok, 3 * C), 9.0, dtype=torch.bfloat16), torch.empty(B * Q, C, dtype=torch.bfloat16)
    extra = dict(q=qm, o=om, dout=dom, lse=lsem, allow=allow, dq=dq, Q=Q)
    ws = torch.empty(ops.attn_bwd_workspace(B, Ntok, H, Q), dtype=torch.uint8)
    if image:
        ops.attn_bwd(qkv, o, dout, lse, cos, sin, dqkv, ws, B, Ntok, H, scale, extra=extra)
    else:
        ops.attn_bwd(qkv, None, None, None, cos, sin, dqkv, ws, B, Ntok, H, scale, extra=extra)
    heads = lambda t, rows: t.double().reshape(B, rows, H, 64).permute(0, 2, 1, 3)
    back = lambda t, rows: t.permute(0, 2, 1, 3).reshape(B * rows, C)
    dqp, dkp, dvp = exact_passenger_grads(heads(qm, Q), heads(qkv[:, C:2 * C], Ntok), heads(qkv[:, 2 * C:], Ntok), heads(dom, Q),
                                          allow.view(B, Q, Ntok).bool(), scale)
    want = torch.cat([torch.zeros(B * Ntok, C, dtype=torch.float64), back(dkp, Ntok), back(dvp, Ntok)], dim=1)
    if image:
        qi, ki, vi = (heads(qkv[:, j * C:(j + 1) * C], Ntok).requires_grad_(True) for j in range(3))
        oi = torch.softmax((qi @ ki.transpose(-1, -2)) * scale, dim=-1) @ vi
        want = want + torch.cat([back(t, Ntok) for t in torch.autograd.grad(oi, (qi, ki, vi), heads(dout, Ntok))], dim=1)
    # bf16 roundings of p, dS and of the outputs: the bound test_gpu_ops holds the attention backward to against fp64
    assert rel(dq, back(dqp, Q)) < 1e-2 and rel(dqkv, want) < 1e-2
    assert not torch.isnan(dqkv).any() and float(dq[2].abs().max()) == 0.0 and float(dq[3].abs().max()) == 0.0
    if not image:
        assert float(dqkv[:, :C].abs().max()) == 0.0
    # without extra rows the call is RefOps' own
    a, b = torch.empty(B * Ntok, 3 * C, dtype=torch.bfloat16), torch.empty(B * Ntok, 3 * C, dtype=torch.bfloat16)
    ops.attn_bwd(qkv, o, dout, lse, cos, sin, a, ws, B, Ntok, H, scale)
    RefOps().attn_bwd(qkv, o, dout, lse, cos, sin, b, ws, B, Ntok, H, scale)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):                                            # passengers are never rotated: identity tables only
        ops.attn_bwd(qkv, o, dout, lse, cos * 0.5, sin, a, ws, B, Ntok, H, scale, extra=extra)


# ------------------------------------------------------------------------------------------------ (4) capability
def test_capability_attribute_decides(gold):
    from clipself_amd import hip
    assert hip.HipOps.ATTN_EXTRA_QUERIES is True and RefOpsExtra.ATTN_EXTRA_QUERIES is True      # class attributes: no device needed
    assert not hasattr(RefOps, "ATTN_EXTRA_QUERIES")
    rec, cfg, student, _ = _setup(gold, ops=RefOps())
    images, boxes, _ = batch_for(rec, 0)
    lists = [b[b[:, -1] > 0.5, :4] for b in boxes]
    with pytest.raises(NotImplementedError, match="'ref'"):                    # the refusal names the backend
        student.encode_pseudo_boxes(images, lists, extract_type="v1")
    with torch.no_grad():
        student.encode_pseudo_boxes(images, lists, extract_type="v1")
    # the wrapper's identity-table check (no GPU: the object is built around the logic)
    ops = hip.HipOps.__new__(hip.HipOps)
    cos, sin, bad = torch.ones(16, 64), torch.zeros(16, 64), torch.full((16, 64), 0.1)       # (the check is cached per table address)
    ops._check_identity_tables(cos, sin)
    with pytest.raises(ValueError):
        ops._check_identity_tables(cos, bad)
