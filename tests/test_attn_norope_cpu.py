"""Attention without rotary tables for the OpenAI-CLIP ViT family, the parts that need no GPU: the engine's hook (`ClipVitEngine.rope_tables`
returns (None, None) on a backend that advertises ATTN_NO_ROPE, identity tables elsewhere and under CLIPSELF_ATTN_IDENTITY_ROPE=1), the
argument logic of the HipOps wrappers (None/None skips the table checks, one None raises before any launch), and that neither the EVA02
engine nor the OpenAI engine on the CPU reference changed.  The kernels themselves: tests/test_gpu_attn_norope.py."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from clipself_amd import hip
from clipself_amd.config import tiny_cfg, tiny_openai_cfg
from clipself_amd.engine import EvaEngine
from clipself_amd.engine_openai import ClipVitEngine
from clipself_amd.init import seeded_visual_state, synthetic_batch
from oracle.ops_ref import RefOps

SWITCH = "CLIPSELF_ATTN_IDENTITY_ROPE"


class StubOps(RefOps):
    """A backend that advertises the null-table attention forms (what HipOps does), on the CPU."""
    ATTN_NO_ROPE = True


def _identity(cos, sin, g):
    return (tuple(cos.shape) == (g * g, 64) and tuple(sin.shape) == (g * g, 64) and cos.dtype == torch.float32
            and bool((cos == 1).all()) and bool((sin == 0).all()))


def test_hook_returns_no_tables_on_a_backend_with_the_flag(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert hip.HipOps.ATTN_NO_ROPE is True
    eng = ClipVitEngine(tiny_openai_cfg(), StubOps(), trainable=False)
    for g in (4, 7, 14):
        assert eng.rope_tables(g) == (None, None)
    eng.ops.ATTN_NO_ROPE = False                               # set on the instance: the hook asks the object, per call
    assert _identity(*eng.rope_tables(4), 4)


def test_hook_returns_identity_tables_on_refops_and_under_the_switch(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert not hasattr(RefOps, "ATTN_NO_ROPE")
    ref = ClipVitEngine(tiny_openai_cfg(), RefOps(), trainable=False)
    stub = ClipVitEngine(tiny_openai_cfg(), StubOps(), trainable=False)
    for g in (4, 8):
        assert _identity(*ref.rope_tables(g), g)
    monkeypatch.setenv(SWITCH, "1")
    for g in (4, 8):
        assert _identity(*stub.rope_tables(g), g) and _identity(*ref.rope_tables(g), g)
    monkeypatch.setenv(SWITCH, "0")                            # read where the hook decides: no restart, no cached decision
    assert stub.rope_tables(4) == (None, None)


class _Lib:
    """Stands in for the ctypes library: records every entry point it is asked to run."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 16 if name.endswith("_workspace") else 0
        return fn


def _wrapper_ops(monkeypatch):
    ops = hip.HipOps.__new__(hip.HipOps)
    ops.lib = _Lib()
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)

    def no_check(*a, **k):
        raise AssertionError("a table check ran on a call without tables")
    monkeypatch.setattr(ops, "_check_rope_tables", no_check)
    monkeypatch.setattr(ops, "_check_identity_tables", no_check)
    return ops


def test_wrappers_pass_null_tables_and_skip_the_table_checks(monkeypatch):
    """None/None: no layout check, no identity check (a host read-back each), NULL pointers in the cos_t / sin_t slots of the C call."""
    ops = _wrapper_ops(monkeypatch)
    B, N, H = 2, 12, 2                                         # 11 image tokens: no square grid
    C = H * 64
    bf = torch.bfloat16
    qkv, out, lse = torch.zeros(B * N, 3 * C, dtype=bf), torch.zeros(B * N, C, dtype=bf), torch.zeros(B * H, N)
    ops.attn_fwd(qkv, None, None, out, lse, B, N, H, 0.125)
    ops.attn_fwd_stats(qkv, None, None, out, lse, torch.zeros(H, B * N, 2), B, N, H, 0.125)
    ops.attn_cls_fwd(out[:B], qkv[:, C:], None, None, out[:B], B, N, H, 0.125)
    ws = torch.zeros(64, dtype=torch.uint8)
    ops.attn_bwd(qkv, out, out, lse, None, None, torch.zeros_like(qkv), ws, B, N, H, 0.125)
    Q = 3
    extra = dict(q=torch.zeros(B * Q, C, dtype=bf), o=torch.zeros(B * Q, C, dtype=bf), dout=torch.zeros(B * Q, C, dtype=bf),
                 lse=torch.zeros(B * H, Q), allow=torch.ones(B * Q, N, dtype=torch.uint8), dq=torch.zeros(B * Q, C, dtype=bf), Q=Q)
    ops.attn_bwd(qkv, out, out, lse, None, None, torch.zeros_like(qkv), ws, B, N, H, 0.125, extra=extra)
    ops.attn_bwd(qkv, None, None, None, None, None, torch.zeros_like(qkv), ws, B, N, H, 0.125, extra=extra)       # the image-less launch
    slots = {"cs_attn_fwd": (1, 2), "cs_attn_fwd_stats": (1, 2), "cs_attn_cls_fwd": (2, 3), "cs_attn_bwd": (4, 5)}
    launches = [(n, a) for n, a in ops.lib.calls if n in slots]
    assert [n for n, _ in launches] == ["cs_attn_fwd", "cs_attn_fwd_stats", "cs_attn_cls_fwd", "cs_attn_bwd", "cs_attn_bwd", "cs_attn_bwd"]
    for name, args in launches:
        assert all(args[i] is None for i in slots[name]), name
    assert set(hip.SIGNATURES) >= set(slots) and len(hip.SIGNATURES["cs_attn_bwd"][1]) == 16       # no new symbol, no signature change


def test_wrappers_refuse_one_missing_table_before_any_launch(monkeypatch):
    ops = _wrapper_ops(monkeypatch)
    B, N, H = 1, 17, 1
    bf = torch.bfloat16
    qkv, out, lse = torch.zeros(N, 192, dtype=bf), torch.zeros(N, 64, dtype=bf), torch.zeros(H, N)
    t = torch.ones(N - 1, 64)
    for cos, sin in ((None, t), (t, None)):
        with pytest.raises(ValueError):
            ops.attn_fwd(qkv, cos, sin, out, lse, B, N, H, 0.125)
        with pytest.raises(ValueError):
            ops.attn_fwd_stats(qkv, cos, sin, out, lse, torch.zeros(H, N, 2), B, N, H, 0.125)
        with pytest.raises(ValueError):
            ops.attn_cls_fwd(out[:1], qkv[:, 64:], cos, sin, out[:1], B, N, H, 0.125)
        with pytest.raises(ValueError):
            ops.attn_bwd(qkv, out, out, lse, cos, sin, torch.zeros_like(qkv), torch.zeros(64, dtype=torch.uint8), B, N, H, 0.125)
    assert ops.lib.calls == []


def test_tables_are_still_checked_when_given():
    """With tables nothing changed: the layout check runs (and refuses a non-square grid), the passengers' backward wants the identity."""
    ops = hip.HipOps.__new__(hip.HipOps)
    ops._chk = lambda *ts: None
    with pytest.raises(ValueError):
        ops.attn_fwd(torch.zeros(12, 192, dtype=torch.bfloat16), torch.ones(11, 64), torch.zeros(11, 64), torch.zeros(12, 64, dtype=torch.bfloat16),
                     None, 1, 12, 1, 0.125)
    with pytest.raises(ValueError):
        ops._check_identity_tables(torch.full((16, 64), 0.5), torch.zeros(16, 64))


def test_eva_engine_is_unaffected(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert "ATTN_NO_ROPE" not in vars(EvaEngine) and EvaEngine.rope_tables is not ClipVitEngine.rope_tables
    eng = EvaEngine(tiny_cfg(), StubOps(), trainable=False)
    cos, sin = eng.rope_tables(tiny_cfg().grid)
    g = tiny_cfg().grid
    assert torch.is_tensor(cos) and torch.is_tensor(sin) and tuple(cos.shape) == (g * g, 64)
    assert not bool((cos == 1).all())                          # real rotary tables, flag or no flag
    hip.HipOps.__new__(hip.HipOps)._check_rope_tables(cos, sin, g * g + 1)


def test_openai_engine_on_refops_computes_what_it_did(golden_dir, monkeypatch):
    """RefOps does not advertise the flag, so the CPU engine runs the identity-table path, the code it ran before: one teacher forward and one
    dense forward of the tiny config, equal bit for bit with the switch forcing that path, and inside the existing bounds of
    test_openai_vit_cpu.py against the reference's goldens."""
    monkeypatch.delenv(SWITCH, raising=False)
    g = np.load(golden_dir / "tiny_openai_step.npz")
    rec = json.loads(str(g["recipe"]))
    cfg = tiny_openai_cfg()
    images, _, crops = synthetic_batch(rec["batch"], rec["boxes"], cfg.image_size, cfg.image_size, seed=rec["seed_b"])
    seen = []

    class Spy(RefOps):
        def attn_fwd(self, qkv, cos, sin, *a):
            seen.append((cos, sin))
            return super().attn_fwd(qkv, cos, sin, *a)

    def run():
        eng = ClipVitEngine(cfg, Spy(), trainable=False)
        eng.load_state(seeded_visual_state(cfg, rec["seed_w"]))
        return eng.encode_image(crops.flatten(0, 1), chunk=4), eng.encode_dense(images)[0]

    t0, d0 = run()
    assert seen and all(torch.is_tensor(c) and bool((c == 1).all()) and bool((s == 0).all()) for c, s in seen)
    monkeypatch.setenv(SWITCH, "1")
    t1, d1 = run()
    assert torch.equal(t0, t1) and torch.equal(d0, d1)
    rel = lambda a, b: float((a.double() - torch.as_tensor(b).double()).norm() / torch.as_tensor(b).double().norm())
    assert rel(t0, g["teacher"]) < 2e-2 and rel(d0[:, 1:], g["dense"]) < 2e-2
