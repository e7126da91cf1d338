"""`-m gpu`: the image-token attention kernels without rotary tables (cos_t == sin_t == NULL; include/clipself_hip.h, cs_attn_fwd).

(1) by value against identity tables (cos 1, sin 0) of the same library, at the smallest square token counts that reach each kernel form;
(2) token counts that are no square grid + 1 -- an argument error with tables -- and the smallest sequence (2 tokens) against RefOps with
    identity tables of [Ntok - 1, 64], at the bounds of test_gpu_ops.py::test_attention_fwd_bwd;
(3) cs_attn_bwd's extra query rows ("passengers") with NULL tables, the image-less launch included;
(4) argument errors; (5) read / write extents in poisoned halos (tests/_extents.run_case); (6) the OpenAI-ViT engine with the flag on and off.
Figures are printed before they are asserted (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from oracle.ops_ref import RefOps  # noqa: E402
from test_gpu_ops import BF, F32, rel, rnd  # noqa: E402

SCALE = 64 ** -0.5
# (B, Ntok, H), Ntok - 1 a square.  17 / 65: one and three key tiles of attn_fwd8_kernel<false>; 170: its ragged sixth tile; 197: attn_fwd8_kernel<true>
# (the 14 x 14 grid); 226: attn_fwd2_kernel and the several-chunk backward with ONE key in the second chunk; 257: 33 keys there, three heads;
# 401: a ragged second chunk; 785: four chunks, a sequence's last tile riding on a split block (set_schedule needs >= 256 queries), the
# backward whose rope_qk_kernel prepass the NULL form skips
SQUARE = [(3, 17, 2), (2, 65, 2), (2, 170, 2), (2, 197, 2), (2, 226, 2), (1, 257, 3), (1, 401, 2), (1, 785, 2)]
# every path of the NULL form that tables cannot reach: 2 tokens, below / inside / at the end of the one-image forward (200: <true>, 224: its
# last full tile), 225: one key in the second chunk, 250 and 449: ragged chunks of the several-chunk kernels
NON_SQUARE = [2, 100, 200, 224, 225, 250, 449]


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    ops = HipOps()
    assert ops.ATTN_NO_ROPE
    return ops


_MEMO = {}


def _data(B, Ntok, H):
    """Seeded inputs as in test_attention_fwd_bwd (q and k scaled by 2) and, computed once, RefOps' forward and backward with identity tables."""
    key = (B, Ntok, H)
    if key not in _MEMO:
        C = H * 64
        qkv = rnd((B * Ntok, 3 * C), F32, 1.0, seed=30)
        qkv[:, :2 * C] *= 2.0
        qkv = qkv.to(BF)
        dout = rnd((B * Ntok, C), BF, seed=31)
        cos, sin = torch.ones(Ntok - 1, 64), torch.zeros(Ntok - 1, 64)
        ref = RefOps()
        o, lse = torch.empty(B * Ntok, C, dtype=BF), torch.empty(B * H, Ntok)
        ref.attn_fwd(qkv, cos, sin, o, lse, B, Ntok, H, SCALE)
        dqkv = torch.zeros(B * Ntok, 3 * C, dtype=BF)
        ref.attn_bwd(qkv, o, dout, lse, cos, sin, dqkv, None, B, Ntok, H, SCALE)
        _MEMO[key] = dict(qkv=qkv, dout=dout, cos=cos, sin=sin, o=o, lse=lse, dqkv=dqkv)
    return _MEMO[key]


def _nan(shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _same(name, a, b):
    """torch.equal semantics: equal by value (-0.0 == +0.0: the one difference the identity rotation may make), no NaN anywhere."""
    n = int((a != b).sum())
    print(f"{name}: {n} of {a.numel()} elements differ")
    assert torch.equal(a, b), f"{name}: {n} of {a.numel()} elements differ between NULL tables and identity tables"


# ------------------------------------------------------------------------------------------------ (1) by value against identity tables
@pytest.mark.parametrize("shape", SQUARE, ids=lambda s: "x".join(map(str, s)))
def test_null_tables_equal_identity_tables_by_value(hip, shape):
    B, Ntok, H = shape
    C, d = H * 64, _data(*shape)
    qkv, dout, cos, sin = (d[k].cuda() for k in ("qkv", "dout", "cos", "sin"))
    tag = f"norope[{B},{Ntok},{H}]"
    res = {}
    for name, (c, s) in (("ident", (cos, sin)), ("null", (None, None))):
        out, lse, out2 = _nan((B * Ntok, C)), _nan((B * H, Ntok), F32), _nan((B * Ntok, C))
        hip.attn_fwd(qkv, c, s, out, lse, B, Ntok, H, SCALE)
        hip.attn_fwd(qkv, c, s, out2, None, B, Ntok, H, SCALE)
        out3, lse3, part = _nan((B * Ntok, C)), _nan((B * H, Ntok), F32), _nan((H, B * Ntok, 2), F32)
        hip.attn_fwd_stats(qkv, c, s, out3, lse3, part, B, Ntok, H, SCALE)
        q_cls = qkv.view(B, Ntok, 3 * C)[:, 0, :C].contiguous()
        cls = _nan((B, C))
        hip.attn_cls_fwd(q_cls, qkv[:, C:], c, s, cls, B, Ntok, H, SCALE)
        res[name] = dict(out=out, lse=lse, out_nolse=out2, out_stats=out3, lse_stats=lse3, stats_part=part, cls=cls)
    # the backward of both forms is fed the SAME o / lse (the identity-table forward's)
    o, lse = res["ident"]["out"], res["ident"]["lse"]
    nbytes = hip.attn_bwd_workspace(B, Ntok, H)
    ws = {}
    for name, (c, s) in (("ident", (cos, sin)), ("null", (None, None))):
        ws[name] = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        dqkv = _nan((B * Ntok, 3 * C))
        hip.attn_bwd(qkv, o, dout, lse, c, s, dqkv, ws[name], B, Ntok, H, SCALE)
        res[name]["dqkv"] = dqkv
    torch.cuda.synchronize()
    for k in res["ident"]:
        assert not torch.isnan(res["null"][k]).any(), f"{tag}.{k}: NaN (an element was not written)"
        _same(f"{tag}.{k}", res["null"][k], res["ident"][k])
    assert torch.equal(res["null"]["out"], res["null"]["out_nolse"]) and torch.equal(res["null"]["out"], res["null"]["out_stats"])
    # against the reference too, at test_attention_fwd_bwd's bounds (the by-value comparison alone would pass two forms that are wrong together)
    r_o, r_l, r_g = rel(res["null"]["out"], d["o"]), rel(res["null"]["lse"], d["lse"]), rel(res["null"]["dqkv"], d["dqkv"])
    print(f"{tag}: vs RefOps o {r_o:.3e} lse {r_l:.3e} dqkv (own forward's o / lse) {r_g:.3e}")
    assert r_o <= 4e-3 and r_l <= 1e-4
    if Ntok > 7 * 32:
        # several key chunks: with tables, rope_qk_kernel writes the rotated q | k image behind dsum [B*H, Ntok] f32 (256-byte aligned) in the
        # workspace; the NULL form reads q | k from qkv itself and must leave that region alone -- and, above, computed the same dqkv
        img0 = (B * H * Ntok * 4 + 255) // 256 * 256
        assert img0 < nbytes
        assert bool((ws["null"][img0:] == 0xFF).all()), "NULL tables: the q | k image of the workspace was written (the prepass ran)"
        assert not bool((ws["ident"][img0:] == 0xFF).all()), "identity tables: the prepass did not write its image (the test lost its contrast)"


# ------------------------------------------------------------------------------------------------ (2) non-square token counts against RefOps
@pytest.mark.parametrize("Ntok", NON_SQUARE)
def test_any_token_count_matches_reference(hip, Ntok):
    B, H = 2, 2
    C, d = H * 64, _data(B, Ntok, H)
    g = int(round((Ntok - 1) ** 0.5))
    square = g * g == Ntok - 1
    assert not square or Ntok == 2                              # 2 tokens: the smallest sequence (a 1 x 1 grid), every other count has no grid
    qkv, dout = d["qkv"].cuda(), d["dout"].cuda()
    out, lse = _nan((B * Ntok, C)), _nan((B * H, Ntok), F32)
    hip.attn_fwd(qkv, None, None, out, lse, B, Ntok, H, SCALE)
    out2 = _nan((B * Ntok, C))
    hip.attn_fwd(qkv, None, None, out2, None, B, Ntok, H, SCALE)
    # backward: both sides start from the reference forward's o / lse, as in test_attention_fwd_bwd
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
    dqkv = _nan((B * Ntok, 3 * C))
    hip.attn_bwd(qkv, d["o"].cuda(), dout, d["lse"].cuda(), None, None, dqkv, ws, B, Ntok, H, SCALE)
    torch.cuda.synchronize()
    tag = f"norope[{B},{Ntok},{H}]"
    figs = dict(o=(out, d["o"], 4e-3), lse=(lse, d["lse"], 1e-4), dq=(dqkv[:, :C], d["dqkv"][:, :C], 1e-3),
                dk=(dqkv[:, C:2 * C], d["dqkv"][:, C:2 * C], 1e-3), dv=(dqkv[:, 2 * C:], d["dqkv"][:, 2 * C:], 1e-3))
    errs = {k: rel(got, want) for k, (got, want, _) in figs.items()}
    print(f"{tag}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k, (got, _, tol) in figs.items():
        assert torch.isfinite(got.float()).all(), f"{tag}.{k}: non-finite output"
        assert errs[k] <= tol, f"{tag}.{k}: rel {errs[k]:.3e} > {tol:.1e}"
    assert torch.equal(out, out2)
    # with tables this token count stays what it was: an argument error in the forward
    if not square:
        t = torch.ones(Ntok - 1, 64, device="cuda")
        rc = hip.lib.cs_attn_fwd(qkv.data_ptr(), t.data_ptr(), t.data_ptr(), out2.data_ptr(), None, B, Ntok, H, 3 * C, C, SCALE, None)
        assert rc == -1 and b"square" in hip.lib.cs_last_error()


# ------------------------------------------------------------------------------------------------ (3) passengers
def test_passenger_backward_accepts_null_tables(hip):
    B, Q, Ntok, H = 2, 3, 65, 2
    C, d = H * 64, _data(B, Ntok, H)
    qkv, dout, o, lse, cos, sin = (d[k].cuda() for k in ("qkv", "dout", "o", "lse", "cos", "sin"))
    qm = rnd((B * Q, C), BF, 2.0, seed=52).cuda()
    dom = rnd((B * Q, C), BF, seed=53).cuda()
    allow = (torch.rand(B * Q, Ntok, generator=torch.Generator().manual_seed(54)) < 0.5).to(torch.uint8)
    allow[:, 0] = 1
    allow[1, 1:] = 0                                            # a CLS-only passenger
    allow = allow.cuda()
    om, lsem = _nan((B * Q, C)), _nan((B * H, Q), F32)
    hip.attn_query_fwd(qm, qkv[:, C:], allow, om, B, Q, Ntok, H, SCALE, lse=lsem)
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H, Q), dtype=torch.uint8, device="cuda")

    def launch(tables, image):
        dq, dqkv = _nan((B * Q, C)), _nan((B * Ntok, 3 * C))
        img = (o, dout, lse) if image else (None, None, None)
        hip.attn_bwd(qkv, *img, *tables, dqkv, ws, B, Ntok, H, SCALE, extra=dict(q=qm, o=om, dout=dom, lse=lsem, allow=allow, dq=dq, Q=Q))
        torch.cuda.synchronize()
        assert not torch.isnan(dq).any() and not torch.isnan(dqkv).any()
        return dqkv, dq

    for image in (True, False):
        a, b = launch((cos, sin), image), launch((None, None), image)
        _same(f"passengers image={image} dqkv", b[0], a[0])
        _same(f"passengers image={image} extra.dq", b[1], a[1])
        assert float(b[1].abs().max()) > 0 and float(b[0][:, C:].abs().max()) > 0
    assert float(b[0][:, :C].abs().max()) == 0.0                # the image-less launch: dqkv = [0 | dK | dV]


# ------------------------------------------------------------------------------------------------ (4) argument errors
def test_one_null_table_and_one_token_are_argument_errors(hip):
    B, Ntok, H = 1, 17, 1
    C = 64
    sentinel = 3.0
    qkv = rnd((Ntok, 3 * C), BF, seed=1).cuda()
    t = torch.ones(Ntok - 1, 64, device="cuda")
    lse = torch.zeros(H, Ntok, device="cuda")
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H), dtype=torch.uint8, device="cuda")
    lib, p = hip.lib, (lambda x: None if x is None else x.data_ptr())
    for cos, sin in ((t, None), (None, t)):
        out = torch.full((Ntok, 3 * C), sentinel, dtype=BF, device="cuda")
        part = torch.full((H, Ntok, 2), sentinel, device="cuda")
        calls = {
            "cs_attn_fwd": lambda: lib.cs_attn_fwd(p(qkv), p(cos), p(sin), p(out), None, B, Ntok, H, 3 * C, 3 * C, SCALE, None),
            "cs_attn_fwd_stats": lambda: lib.cs_attn_fwd_stats(p(qkv), p(cos), p(sin), p(out), None, p(part), B, Ntok, H, 3 * C, 3 * C, SCALE, None),
            "cs_attn_cls_fwd": lambda: lib.cs_attn_cls_fwd(p(qkv), p(qkv[:, C:]), p(cos), p(sin), p(out), B, Ntok, H, 3 * C, 3 * C, 3 * C, SCALE, None),
            "cs_attn_bwd": lambda: lib.cs_attn_bwd(p(qkv), p(qkv), p(qkv), p(lse), p(cos), p(sin), p(out), p(ws), B, Ntok, H, 3 * C, 3 * C, SCALE,
                                                   None, None),
        }
        for name, call in calls.items():
            rc = call()
            text = lib.cs_last_error().decode()
            print(f"{name}(cos={'set' if cos is not None else 'NULL'}, sin={'set' if sin is not None else 'NULL'}): rc {rc}, {text!r}")
            # (cs_attn_fwd_stats shares cs_attn_fwd's argument checks and reports under that name)
            assert rc == -1 and name.replace("_stats", "") in text and "NULL" in text
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()) and bool((part == sentinel).all()), "a kernel ran on an argument error"
        for fn in (lambda: hip.attn_fwd(qkv, cos, sin, out[:, :C], None, B, Ntok, H, SCALE),
                   lambda: hip.attn_bwd(qkv, out[:, :C], out[:, :C], lse, cos, sin, out, ws, B, Ntok, H, SCALE)):
            with pytest.raises(ValueError):
                fn()
    out = torch.full((1, C), sentinel, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.attn_fwd(qkv[:1], None, None, out, None, 1, 1, 1, SCALE)
    with pytest.raises(RuntimeError, match="bad shape"):
        hip.attn_bwd(qkv[:1], out, out, lse, None, None, torch.empty_like(qkv[:1]), ws, 1, 1, 1, SCALE)
    with pytest.raises(RuntimeError, match="bad sizes"):
        hip.attn_cls_fwd(qkv[:1, :C], qkv[:1, C:], None, None, out, 1, 1, 1, SCALE)
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


# ------------------------------------------------------------------------------------------------ (5) extents
def _extents_case(B, Ntok, H, form):
    def fn(ops, a):
        C, d = H * 64, _data(B, Ntok, H)
        qkv = a.inp(d["qkv"], a.ld(3 * C, 8))
        ldo = a.ld(C, 8)
        if form == "bwd":
            dqkv = a.out((B * Ntok, 3 * C), BF, a.ld(3 * C, 8))
            ops.attn_bwd(qkv, a.inp(d["o"], ldo), a.inp(d["dout"], ldo), a.inp(d["lse"]), None, None, dqkv,
                         a.ws(ops.attn_bwd_workspace(B, Ntok, H)), B, Ntok, H, SCALE)
            return {"dqkv": dqkv}
        if form == "cls":
            q = a.inp(d["qkv"].view(B, Ntok, 3 * C)[:, 0, :C].contiguous(), a.ld(C, 8))
            out = a.out((B, C), BF, ldo)
            ops.attn_cls_fwd(q, qkv[:, C:], None, None, out, B, Ntok, H, SCALE)
            return {"out": out}
        out, lse = a.out((B * Ntok, C), BF, ldo), a.out((B * H, Ntok), F32)
        ops.attn_fwd(qkv, None, None, out, lse, B, Ntok, H, SCALE)
        out2, lse2, part = a.out((B * Ntok, C), BF, ldo), a.out((B * H, Ntok), F32), a.out((H, B * Ntok, 2), F32)
        ops.attn_fwd_stats(qkv, None, None, out2, lse2, part, B, Ntok, H, SCALE)
        return {"out": out, "lse": lse, "out_stats": out2, "lse_stats": lse2, "stats_part": part}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("form", ["fwd", "cls", "bwd"])
@pytest.mark.parametrize("size", [(2, 197, 2), (1, 250, 2), (1, 449, 2)], ids=lambda s: "x".join(map(str, s)))
def test_null_table_extents(hip, size, form, pad):
    name = f"attn_norope_{form}[{size}]"
    problems = run_case(hip, _extents_case(*size, form), "cuda", pad, key=name)
    assert not problems, f"{name} (row strides + {pad}):\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ (6) engine level
def _flag(models, on):
    for m in models:
        ops = m.visual.engine.ops
        assert type(ops).__name__ == "HipOps" and type(m.visual.engine).__name__ == "ClipVitEngine"
        if not on:
            ops.ATTN_NO_ROPE = False                            # on the instance: ClipVitEngine.rope_tables asks the object
        assert (m.visual.engine.rope_tables(4)[0] is None) == on


def _v2_run(on):
    from types import SimpleNamespace
    from clipself_amd.config import tiny_openai_cfg
    from clipself_amd.init import seeded_visual_state, synthetic_batch
    from clipself_amd.open_clip.model import CLIP
    from clipself_amd.training.clipself import CLIPSelf
    from clipself_amd.training.optim import FlatAdamW
    from clipself_amd.training.train import train_step
    cfg = tiny_openai_cfg()
    student, teacher = CLIP(cfg, trainable=True), CLIP(cfg, trainable=False)
    for m in (student, teacher):
        m.visual.engine.load_state(seeded_visual_state(cfg, 11))
    student.lock_image_tower(unlocked_groups=cfg.layers)
    student.train()
    teacher.eval()
    _flag((student, teacher), on)
    batch = synthetic_batch(2, 3, cfg.image_size, cfg.image_size, seed=21)
    images, _, crops = batch
    with torch.no_grad():
        t = teacher.encode_image(crops.flatten(0, 1).cuda())    # the folded schedule + the CLS-only last block
        dense = student.encode_dense(images.cuda(), keep_shape=False)
    opt = FlatAdamW(student, lr=1e-3, weight_decay=0.1)
    args = SimpleNamespace(device="cuda", precision="amp", distributed=False, skip_scheduler=True, grad_clip_norm=None, multiscale=False,
                           extract_type="v2", cosine_weight=1.0)
    out, _, _ = train_step(student, CLIPSelf(), batch, opt, None, 0, teacher, args)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.grad is not None}
    return dict(teacher=t.clone(), dense=dense.clone(), loss=out["loss"].detach().clone(), **{"grad/" + n: v for n, v in grads.items()})


def _v1_run(on, golden_dir):
    from _maskattn_ref import build_pair, load_gold, recipe_of, run_recipe
    from clipself_amd.config import tiny_openai_cfg
    rec = recipe_of(load_gold(golden_dir), "all/")              # the whole tower trains: every block's attn_bwd(extra=), the stem
    student, teacher = build_pair(tiny_openai_cfg(), rec, None, None)
    _flag((student, teacher), on)
    losses, first = run_recipe(student, teacher, rec, 1, device="cuda")
    torch.cuda.synchronize()
    return dict(loss=torch.tensor(losses), **{"grad/" + n: v for n, v in first.items()})


def _engine_equal(a, b, what, least):
    assert a.keys() == b.keys() and len(a) >= least, (what, len(a))
    for k in a:
        assert torch.isfinite(a[k].float()).all(), f"{what} {k}: non-finite"
        assert torch.equal(a[k], b[k]), f"{what} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} elements differ with ATTN_NO_ROPE on / off"
    print(f"{what}: {len(a)} tensors equal with ATTN_NO_ROPE on / off")


def test_engine_encode_image_and_v2_step_do_not_depend_on_the_flag(hip):
    a, b = _v2_run(True), _v2_run(False)
    assert float(a["teacher"].abs().max()) > 0 and float(a["loss"]) > 0
    _engine_equal(a, b, "tiny OpenAI ViT: encode_image, dense map, v2 loss and gradients", 3 + 12)


def test_engine_v1_step_does_not_depend_on_the_flag(hip, golden_dir):
    a, b = _v1_run(True, golden_dir), _v1_run(False, golden_dir)
    assert float(a["loss"][0]) > 0
    _engine_equal(a, b, "tiny OpenAI ViT: v1 (mask_attn_pool) loss and gradients", 1 + 12)
