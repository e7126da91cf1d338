"""`-m gpu`: training through mask-attention pooling (extract_type='v1') on the HIP kernels.

(1) op level: cs_attn_query_fwd's log-sum-exp and cs_attn_bwd's `extra` rows against tests/_maskattn_ref.RefOpsExtra and an fp64 evaluation;
(2) the same op inside the poisoned-halo harness (tests/_extents.run_case on cases defined here);
(3) model level: the recipes of tests/golden/tiny_openai_maskattn_grad*.npz (captured from the real reference by
    tools/gen_golden_maskattn_grad.py) through CLIP(cfg) on HipOps and CLIPSelf(), bit-reproducibility, and a ViT-B/16 step against fp32
    autograd of the oracle.
Bounds and the measurements behind them: profiles/maskattn_train_parity.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from _maskattn_ref import (RECIPES, RefOpsExtra, batch_for, build_pair, exact_passenger_grads, load_gold, oracle_grads, recipe_of,  # noqa: E402
                           run_recipe)
from test_gpu_ops import BF, F32, TOL_BF, rel, rnd  # noqa: E402

SCALE = 64 ** -0.5
# (B, Q, Ntok, H): less than one tile | .. | the ragged 7th 32-key tile | Q past a 32-row tile, head group 6 | cs_attn_bwd's multi-chunk path and
# a second key block | several key blocks: the fixed-order dq sum
SHAPES = [(1, 1, 17, 1), (2, 3, 17, 2), (2, 3, 197, 2), (3, 33, 197, 12), (2, 5, 226, 2), (1, 20, 785, 4)]


def _log(line):
    print(line)                                         # every figure before its assert (pytest -s shows them)


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


_DATA = {}


def _data(B, Q, Ntok, H):
    """Seeded CPU inputs of one shape and everything computed from them once: the references' outputs and the fp64 sums."""
    key = (B, Q, Ntok, H)
    if key in _DATA:
        return _DATA[key]
    ref, C, g = RefOpsExtra(), H * 64, int(round((Ntok - 1) ** 0.5))
    cos, sin = torch.ones(g * g, 64), torch.zeros(g * g, 64)
    qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=50)
    qkv[:, :2 * C] *= 2.0
    qkv = qkv.to(BF)
    o, lse = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
    ref.attn_fwd(qkv, cos, sin, o, lse, B, Ntok, H, SCALE)
    dout = rnd((B * Ntok, C), BF, seed=51)
    # passengers: q as the first C columns of a q|k|v matrix whose other columns must never be read (NaN)
    qm = torch.full((B * Q, 3 * C), float("nan"), dtype=BF)
    qm[:, :C] = rnd((B * Q, C), BF, 2.0, seed=52)
    dom = rnd((B * Q, C), BF, seed=53)
    allow = (torch.rand(B * Q, Ntok, generator=torch.Generator().manual_seed(54)) < 0.5).to(torch.uint8)
    allow[:, 0] = 1
    kinds = ["all", "cls", "none", "zero_dout"]
    for r in range(min(B * Q, 4)):                      # the first rows: all-allowed, CLS-only, no key at all, zero upstream gradient
        if kinds[r] == "all":
            allow[r] = 1
        elif kinds[r] == "cls":
            allow[r, 1:] = 0
        elif kinds[r] == "none":
            allow[r] = 0
        else:
            dom[r] = 0
    om, lsem = torch.empty(B * Q, C, dtype=BF), torch.empty(B * H, Q)
    ref.attn_query_fwd(qm[:, :C], qkv[:, C:], allow, om, B, Q, Ntok, H, SCALE, lse=lsem)
    ws = torch.empty(4, dtype=torch.uint8)
    extra = lambda dq: dict(q=qm[:, :C], o=om, dout=dom, lse=lsem, allow=allow, dq=dq, Q=Q)
    dq_ref, dqkv_ref = torch.zeros(B * Q, C, dtype=BF), torch.zeros(B * Ntok, 3 * C, dtype=BF)
    ref.attn_bwd(qkv, o, dout, lse, cos, sin, dqkv_ref, ws, B, Ntok, H, SCALE, extra=extra(dq_ref))
    dq_ref2, dqkv_ref_noimg = torch.zeros(B * Q, C, dtype=BF), torch.full((B * Ntok, 3 * C), 7.0, dtype=BF)
    ref.attn_bwd(qkv, None, None, None, cos, sin, dqkv_ref_noimg, ws, B, Ntok, H, SCALE, extra=extra(dq_ref2))
    # fp64 sums on the bf16 inputs: the image tokens' own dK | dV and the passengers'
    heads = lambda t, rows: t.double().reshape(B, rows, H, 64).permute(0, 2, 1, 3)
    back = lambda t, rows: t.permute(0, 2, 1, 3).reshape(B * rows, C)
    qi, ki, vi = (heads(qkv[:, j * C:(j + 1) * C], Ntok).requires_grad_(True) for j in range(3))
    oi = torch.softmax((qi @ ki.transpose(-1, -2)) * SCALE, dim=-1) @ vi
    _, dki, dvi = torch.autograd.grad(oi, (qi, ki, vi), heads(dout, Ntok))
    _, dkp, dvp = exact_passenger_grads(heads(qm[:, :C], Q), heads(qkv[:, C:2 * C], Ntok), heads(qkv[:, 2 * C:], Ntok), heads(dom, Q),
                                        allow.view(B, Q, Ntok).bool(), SCALE)
    kv_img = torch.cat([back(dki, Ntok), back(dvi, Ntok)], dim=1)
    kv_all = kv_img + torch.cat([back(dkp, Ntok), back(dvp, Ntok)], dim=1)
    _DATA[key] = dict(cos=cos, sin=sin, qkv=qkv, o=o, lse=lse, dout=dout, qm=qm, dom=dom, allow=allow, om=om, lsem=lsem, dq_ref=dq_ref,
                      dqkv_ref=dqkv_ref, dqkv_ref_noimg=dqkv_ref_noimg, kv_img=kv_img, kv_all=kv_all)
    return _DATA[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_passenger_attention_forward_lse_and_backward(hip, shape):
    B, Q, Ntok, H = shape
    C, d = H * 64, _data(*shape)
    cu = {k: v.cuda() for k, v in d.items() if k in ("cos", "sin", "qkv", "o", "lse", "dout", "qm", "dom", "allow", "om", "lsem")}
    ldo = C + 8                                                          # a padded row stride for o / dout of the passengers
    pad = lambda t: torch.full((t.shape[0], ldo), float("nan"), dtype=BF, device="cuda")
    q, kv = cu["qm"][:, :C], cu["qkv"][:, C:]
    # ---- forward: out and lse; out bit-equal with and without lse
    out0, out1, lse = pad(cu["om"])[:, :C], pad(cu["om"])[:, :C], torch.full((B * H, Q), -1.0, device="cuda")
    hip.attn_query_fwd(q, kv, cu["allow"], out0, B, Q, Ntok, H, SCALE)
    hip.attn_query_fwd(q, kv, cu["allow"], out1, B, Q, Ntok, H, SCALE, lse=lse)
    assert torch.equal(out0.view(torch.int16), out1.view(torch.int16))
    r_out = rel(out1, d["om"])
    inf = torch.isinf(d["lsem"])
    assert torch.equal(torch.isinf(lse).cpu() & (lse.cpu() > 0), inf), "lse = +inf exactly for the rows that allow no key"
    e_lse = float((lse.cpu()[~inf] - d["lsem"][~inf]).abs().max())
    assert not torch.isnan(out1).any() and (B * Q < 3 or float(out1[2].abs().max()) == 0.0)      # the row without keys: zeros
    # ---- backward
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H, Q), dtype=torch.uint8, device="cuda")
    om, dom = pad(cu["om"])[:, :C], pad(cu["dom"])[:, :C]
    om.copy_(cu["om"])
    dom.copy_(cu["dom"])

    def launch(image=True, with_extra=True):
        dqm = torch.full((B * Q, 3 * C), 3.0, dtype=BF, device="cuda")   # dq as the q columns of the passengers' d(q|k|v) rows
        dqkv = torch.full((B * Ntok, 3 * C), 5.0, dtype=BF, device="cuda")
        extra = dict(q=q, o=om, dout=dom, lse=cu["lsem"], allow=cu["allow"], dq=dqm[:, :C], Q=Q) if with_extra else None
        img = (cu["o"], cu["dout"], cu["lse"]) if image else (None, None, None)
        hip.attn_bwd(cu["qkv"], *img, cu["cos"], cu["sin"], dqkv, ws, B, Ntok, H, SCALE, **(dict(extra=extra) if with_extra else {}))
        torch.cuda.synchronize()
        return dqkv, dqm

    plain, _ = launch(with_extra=False)
    full, dqm = launch()
    again, dqm2 = launch()
    noimg, dqm3 = launch(image=False)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(full), bits(again)) and torch.equal(bits(dqm), bits(dqm2)), "two launches differ"
    assert torch.equal(bits(full[:, :C]), bits(plain[:, :C])), "the image rows' q columns changed with extra rows"
    assert torch.equal(bits(dqm[:, C:]), bits(torch.full_like(dqm[:, C:], 3.0))), "passenger rows: only the q columns may be written"
    assert not torch.isnan(full).any() and not torch.isnan(dqm[:, :C]).any()
    r_dq = rel(dqm[:, :C], d["dq_ref"])
    e_plain, e_full = rel(plain[:, C:], d["kv_img"]), rel(full[:, C:], d["kv_all"])
    assert float(noimg[:, :C].abs().max()) == 0.0 and torch.equal(bits(dqm3[:, :C]), bits(dqm[:, :C]))
    r_noimg = rel(noimg[:, C:], d["dqkv_ref_noimg"][:, C:])
    if B * Q > 3:
        assert float(dqm[3, :C].abs().max()) == 0.0 and float(dqm[2, :C].abs().max()) == 0.0     # zero dout / no key: exact zeros
    _log(f"op {shape}: out rel {r_out:.3e} lse maxabs {e_lse:.3e} dq rel {r_dq:.3e} k|v vs fp64: without passengers {e_plain:.3e} "
         f"with {e_full:.3e} (ratio {e_full / e_plain:.2f}) image-less k|v rel {r_noimg:.3e}")
    assert r_out <= TOL_BF and r_dq <= TOL_BF and r_noimg <= TOL_BF          # measured <= 1.4e-5 / 5.6e-5 / 1.6e-5 (profiles/maskattn_train_parity.md)
    # fp32 scores of 64 bf16 products, |s| = O(10): 64 * 2^-24 * |s| ~ 4e-5 per score, and one v_exp / v_log pair per row
    assert e_lse <= 2e-4                                                      # measured <= 2.9e-6
    # measured ratio 1.03 ... 1.13
    assert e_full <= 2 * e_plain, "passengers may add one fp32 sum and one more rounding to the k|v columns"


# ------------------------------------------------------------------------------------------------ (2) extents
def _extents_case(B, Q, Ntok, H, image):
    def fn(ops, a):
        C, d = H * 64, _data(B, Q, Ntok, H)
        ldo = a.ld(C, 8)
        qkv = a.inp(d["qkv"], a.ld(3 * C, 8))
        qm = a.inp(d["qm"], a.ld(3 * C, 8))
        allow = a.inp(d["allow"])
        out = a.out((B * Q, C), BF, ldo)
        lse = a.out((B * H, Q), F32)
        ops.attn_query_fwd(qm[:, :C], qkv[:, C:], allow, out, B, Q, Ntok, H, SCALE, lse=lse)
        dqkv = a.out((B * Ntok, 3 * C), BF, a.ld(3 * C, 8), init=torch.zeros(B * Ntok, 3 * C, dtype=BF))
        dqm = a.out((B * Q, 3 * C), BF, a.ld(3 * C, 8), init=torch.zeros(B * Q, 3 * C, dtype=BF))
        extra = dict(q=qm[:, :C], o=a.inp(d["om"], ldo), dout=a.inp(d["dom"], ldo), lse=a.inp(d["lsem"]), allow=allow, dq=dqm[:, :C], Q=Q)
        img = (a.inp(d["o"], ldo), a.inp(d["dout"], ldo), a.inp(d["lse"])) if image else (None, None, None)
        ops.attn_bwd(qkv, *img, a.inp(d["cos"]), a.inp(d["sin"]), dqkv, a.ws(ops.attn_bwd_workspace(B, Ntok, H, Q)), B, Ntok, H, SCALE,
                     extra=extra)
        return {"out": out, "lse": lse, "dqkv": dqkv, "dqm": dqm}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("image", [True, False], ids=["image", "imageless"])
@pytest.mark.parametrize("size", [(2, 3, 17, 2), (2, 3, 226, 2)], ids=lambda s: "x".join(map(str, s)))
def test_passenger_attention_extents(hip, size, image, pad):
    name = f"attn_extra[{size},{image}]"
    problems = run_case(hip, _extents_case(*size, image), "cuda", pad, key=name)
    assert not problems, f"{name} (row strides + {pad}):\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ (3) model level
@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_gold(golden_dir)


# per-tensor gradient error against the reference's fixture: 2x the worst measured on the MI355X (profiles/maskattn_train_parity.md section 2:
# 4.00e-3, 5.72e-3, 6.35e-3, 5.72e-3, 3.91e-3), all under the hard cap 3e-2 of the v2 twin test_tiny_openai_vit_step_matches_reference_goldens.
# Yardstick: the bf16-forward oracle sits at 3.0e-3 ... 3.9e-3 from the same vectors.
GRAD_BOUND = {"blocks/": 8.0e-3, "stem/": 1.15e-2, "stem64/": 1.27e-2, "all/": 1.15e-2, "q/blocks/": 7.9e-3}
assert max(GRAD_BOUND.values()) <= 3e-2


@pytest.mark.parametrize("tag", RECIPES)
def test_recipes_match_reference_goldens(gold, tag):
    from clipself_amd.config import tiny_openai_cfg
    from clipself_amd.init import seeded_visual_state
    rec = recipe_of(gold, tag)
    cfg = tiny_openai_cfg(rec["quick"])
    student, teacher = build_pair(cfg, rec, None, None)
    assert student.visual.engine.ops.ATTN_EXTRA_QUERIES
    losses, first = run_recipe(student, teacher, rec, rec["steps"], device="cuda")
    _log(f"model {tag} losses {losses} vs {gold[tag + 'losses'].tolist()}")
    assert sorted(n for n in first if n.startswith("visual.")) == sorted(str(n) for n in gold[tag + "trainable"])
    worst, checked = ("", 0.0), 0
    for k in gold:
        if k.startswith(tag + "grad/"):
            n = k[len(tag) + 5:]
            r = rel(first[n].reshape(gold[k].shape), torch.from_numpy(gold[k]))
            worst = max(worst, (n, r), key=lambda x: x[1])
            checked += 1
    glob = rel(torch.cat([first[k[len(tag) + 5:]].reshape(-1).cpu() for k in gold if k.startswith(tag + "grad/")]),
               torch.cat([torch.from_numpy(gold[k]).reshape(-1) for k in gold if k.startswith(tag + "grad/")]))
    _log(f"model {tag} worst gradient {worst[0]} rel {worst[1]:.3e}, over all {checked} tensors {glob:.3e}")
    assert checked >= 3 and worst[1] < GRAD_BOUND[tag], worst
    assert np.allclose(losses, gold[tag + "losses"], atol=1e-3)               # measured <= 5.4e-4 (profiles/maskattn_train_parity.md)
    sd0 = seeded_visual_state(cfg, rec["seed_w"])
    for k in gold:
        if k.startswith(tag + "final/"):
            n = k[len(tag) + 6:]
            w0 = sd0[n].reshape(gold[k].shape)
            r = rel(student.visual.engine.p[n].reshape(gold[k].shape).cpu() - w0, torch.from_numpy(gold[k]) - w0)
            _log(f"model {tag} final update {n} rel {r:.3e}")
            assert r < 6e-2, (n, r)                     # the v2 twin's bound on this model (test_openai_vit_cpu.py); measured <= 4.5e-2 (conv1)


def test_two_identical_steps_give_bit_equal_gradients(gold):
    from clipself_amd.config import tiny_openai_cfg
    rec = recipe_of(gold, "all/")
    cfg = tiny_openai_cfg()
    grads = []
    for _ in range(2):
        student, teacher = build_pair(cfg, rec, None, None)
        run_recipe(student, teacher, rec, 1, device="cuda")
        grads.append(student.visual.engine.grad.clone())
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)) and float(grads[0].abs().max()) > 0


def test_vitb16_step_matches_fp32_oracle_autograd():
    """ViT-B/16, 2 images x 8 boxes, 224^2, every block unlocked, teacher from another seed: one v1 step against fp32 autograd of
    oracle/clip_vit_ref.extract_roi_features_v1."""
    from clipself_amd.config import get_tower_cfg
    from clipself_amd.init import synthetic_batch
    import _maskattn_ref as M
    cfg = get_tower_cfg("ViT-B-16")
    rec = dict(seed_w=0, seed_t=1, seed_b=1234, lock=True, unlocked=cfg.layers, lr=1e-5, wd=0.1, warmup=1000, total=10000, image_size=224)
    batch = synthetic_batch(2, 8, 224, 224, seed=rec["seed_b"])
    want_loss, want = oracle_grads(cfg, rec, batch)
    student, teacher = build_pair(cfg, rec, None, None)
    orig = M.batch_for
    M.batch_for = lambda rec_, step: batch
    try:
        losses, first = run_recipe(student, teacher, rec, 1, device="cuda")
    finally:
        M.batch_for = orig
    worst, sq_e, sq_n = ("", 0.0), 0.0, 0.0
    for n, gw in want.items():
        if n == "logit_scale":
            continue
        r = rel(first[n].reshape(gw.shape), gw)
        worst = max(worst, (n, r), key=lambda x: x[1])
        sq_e += float((first[n].reshape(gw.shape).cpu().double() - gw.double()).pow(2).sum())
        sq_n += float(gw.double().pow(2).sum())
    _log(f"vitb16 v1: loss {losses[0]:.6f} vs {want_loss:.6f}; worst gradient {worst[0]} rel {worst[1]:.3e}; over all {(sq_e / sq_n) ** 0.5:.3e}")
    assert abs(losses[0] - want_loss) < 1e-3            # measured 1.6e-5
    assert worst[1] < 1.32e-2, worst                    # 2x the measured 6.57e-3 (profiles/maskattn_train_parity.md section 3); cap 3e-2
