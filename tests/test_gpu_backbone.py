"""`-m gpu`: the detector backbone's frozen pass on the MI355X.

Kernel alone (HipOps.tokens_to_nchw, forms 1 / 2 of cs_transpose_bf16): bit for bit against the torch expression it replaces,
x.view(B, N, ldx)[:, 1:, :C].permute(0, 2, 1).contiguous() (fp32) and that + .to(bfloat16), and inside the poisoned halos of tests/_extents.py.
Engine: encode_dense(taps=...) returns the bits of encode_dense() for the map and, per tap, the bits of a torch permute of a clone of the
stream taken after that block by a Python hook around the block schedule.
Parity: taps and map against the golden vectors of the real reference tower (tools/gen_golden_fvit.py), at 3 x the worst MI355X measurement
over both fixtures (profiles/fvit_backbone_parity.md; tests/_backbone_ref.py holds the numbers)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from _backbone_ref import (BOUND_MAP_ONE_MINUS_COS, BOUND_MAP_REL_L2, BOUND_TAP_REL_L2, FIXTURES, OUT_INDICES, backbone_cfg,  # noqa: E402
                           build_tower, load_fixture, one_minus_cos, rel_l2)
from _extents import run_case  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
# (B, h*w, C, ldx): one token | 3x3 grid, ragged token tile | padded rows | several token tiles with a ragged last | unaligned C: scalar tail
SHAPES = [(1, 1, 64, 64), (3, 9, 128, 128), (2, 36, 128, 192), (2, 196, 192, 192), (1, 70, 100, 104)]
# beyond those: a full token tile (16-byte stores) over a ragged channel tile and rows that no 16-byte load can start on | 16-byte loads
# together with 16-byte stores in both output types, two tiles each way: the path of every shipped shape
EXTRA = [(2, 64, 72, 75), (1, 128, 128, 128)]


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _x(B, hw, ldx):
    return torch.randn(B * (hw + 1), ldx, generator=torch.Generator().manual_seed(1000 + hw + ldx))


def _torch_form(x, B, N, C, dtype):
    return x.view(B, N, -1)[:, 1:, :C].permute(0, 2, 1).contiguous().to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,hw,C,ldx", SHAPES + EXTRA)
def test_kernel_is_the_torch_permute_bit_for_bit(hip, B, hw, C, ldx, dtype):
    assert hip.TOKEN_TAPS
    N = hw + 1
    x = _x(B, hw, ldx).cuda()
    x.view(B, N, ldx)[:, 0] = float("nan")                              # the CLS rows are never read
    x[:, C:] = float("nan")                                             # nor the padding columns
    sentinel = 0x7FA5 if dtype == BF else 0x7FA5A5A5
    out = torch.full((B, C, 1, hw), sentinel, dtype={BF: torch.int16, F32: torch.int32}[dtype], device="cuda").view(dtype)
    hip.tokens_to_nchw(x[:, :C], B, N, C, out)
    want = _torch_form(x, B, N, C, dtype).view(B, C, 1, hw)
    it = torch.int16 if dtype == BF else torch.int32
    assert torch.equal(out.view(it), want.view(it)), f"{int((out.view(it) != want.view(it)).sum())} of {out.numel()} elements differ"


def _halo_case(B, hw, C, ldx, dtype):
    def fn(ops, a):
        x = a.inp(_x(B, hw, ldx)[:, :C], a.ld(ldx))
        out = a.out((B, C, 1, hw), dtype)
        ops.tokens_to_nchw(x, B, hw + 1, C, out)
        return {"out": out}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,hw,C,ldx", SHAPES + EXTRA)
def test_kernel_stays_inside_its_extents(hip, B, hw, C, ldx, dtype, pad):
    key = f"tokens_to_nchw[{B},{hw},{C},{ldx},{dtype}]"
    problems = run_case(hip, _halo_case(B, hw, C, ldx, dtype), "cuda", pad, key=key)
    assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_wrapper_and_entry_point_refuse_bad_arguments(hip):
    x = torch.zeros(2 * 5, 8, device="cuda")
    out = torch.zeros(2, 8, 2, 2, device="cuda")
    with pytest.raises(AssertionError):
        hip.tokens_to_nchw(x, 2, 5, 8, out.permute(0, 1, 3, 2)[:, :, :, :1])         # not contiguous / wrong token count
    with pytest.raises(AssertionError):
        hip.tokens_to_nchw(x.to(BF), 2, 5, 8, out)                                   # the stream is fp32
    p = lambda t: t.data_ptr()
    assert hip.lib.cs_transpose_bf16(p(x), 8, p(out), 3, 4, 8, 1, 2, None) == -1      # ld_out != tokens
    assert b"token taps" in hip.lib.cs_last_error()
    assert hip.lib.cs_transpose_bf16(p(x), 8, p(out), 4, 4, 8, 3, 2, None) == -1      # no such form
    assert hip.lib.cs_transpose_bf16(p(x), 4, p(out), 4, 4, 8, 1, 2, None) == -1      # ld_in < C


# ------------------------------------------------------------------------------------------------ engine
def _engine_cases():
    from clipself_amd.config import tiny14_cfg
    return [("mini32", backbone_cfg(), 32, (0, 1, 2, 3)), ("mini48", backbone_cfg(), 48, (0, 1, 2, 3)), ("tiny14", tiny14_cfg(), 42, (0, 1))]


@pytest.mark.parametrize("case", range(3), ids=["mini32", "mini48", "tiny14"])
def test_taps_do_not_move_the_map_and_are_the_stream_after_their_block(hip, case):
    _, cfg, S, taps = _engine_cases()[case]
    tower = build_tower(hip, 13, cfg)
    eng = tower.engine
    images = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(7)).cuda()
    plain, g = eng.encode_dense(images)
    plain = plain.clone()
    # the Python hook: the same schedule, a clone of the stream after every block
    streams, inner = {}, eng._block_fwd

    def hooked(i, x, *a, **k):
        y = inner(i, x, *a, **k)
        streams[i] = y.clone()
        return y
    eng._block_fwd = hooked
    try:
        dense, g2, maps = eng.encode_dense(images, taps=taps)
    finally:
        del eng._block_fwd
    assert g2 == g == S // cfg.patch_size and torch.equal(dense, plain), "taps moved the dense map"
    B, N, C = 2, g * g + 1, cfg.width
    for i, m in zip(taps, maps):
        assert tuple(m.shape) == (B, C, g, g) and m.dtype == F32 and m.is_contiguous()
        assert torch.equal(m, _torch_form(streams[i], B, N, C, F32).view(B, C, g, g)), f"tap of block {i}"
    none, _, maps2 = eng.encode_dense(images, taps=taps, final=False, tap_dtype=BF)
    assert none is None and all(torch.equal(b, m.to(BF)) for b, m in zip(maps2, maps))
    # the tower-level method: the same taps, the [B, E, h, w] view of the same map
    maps3, fmap = tower.forward_intermediates(images, list(taps))
    assert all(torch.equal(a, b) for a, b in zip(maps3, maps)) and torch.equal(fmap, tower.encode_dense(images, keep_shape=True))


# ------------------------------------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_reference_backbone(hip, name):
    images, taps, fmap, seed = load_fixture(name)
    tower = build_tower(hip, seed)
    got_taps, got_map = tower.forward_intermediates(images.cuda(), OUT_INDICES)
    worst = 0.0
    for i, (got, want) in enumerate(zip(got_taps, taps)):
        r = rel_l2(got, want)
        worst = max(worst, r)
        print(f"PARITY {name} tap{i} rel-L2 {r:.4e}")
    r, c = rel_l2(got_map, fmap), one_minus_cos(got_map, fmap)
    print(f"PARITY {name} map rel-L2 {r:.4e} 1-cos {c:.4e}")
    assert worst <= BOUND_TAP_REL_L2, (worst, BOUND_TAP_REL_L2)
    assert r <= BOUND_MAP_REL_L2 and c <= BOUND_MAP_ONE_MINUS_COS, (r, c)


def test_backbone_module_runs_on_the_device(hip, monkeypatch, tmp_path):
    """EvaCLIPViT end to end on HipOps: the tuple of the reference, taps through the torch neck on the tower's device."""
    from clipself_amd import fvit
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import factory
    cfg = backbone_cfg()
    real = factory.get_tower_cfg
    monkeypatch.setattr(factory, "get_tower_cfg", lambda n: cfg if n == cfg.name else real(n))
    images, taps, fmap, seed = load_fixture(FIXTURES[1])
    torch.save(seeded_visual_state(cfg, seed), tmp_path / "w.pt")
    m = fvit.EvaCLIPViT(cfg.name, str(tmp_path / "w.pt"), out_indices=OUT_INDICES).cuda().eval()      # the caller places the neck, as mmdet does
    assert type(m.visual.engine.ops).__name__ == "HipOps"
    outs = m(images.cuda())
    assert [tuple(o.shape) for o in outs] == [(2, 128, 24, 24), (2, 128, 12, 12), (2, 128, 6, 6), (2, 128, 3, 3), (2, 64, 6, 6)]
    assert all(o.is_cuda for o in outs)
    assert rel_l2(outs[2], taps[2]) <= BOUND_TAP_REL_L2 and rel_l2(outs[4], fmap) <= BOUND_MAP_REL_L2
    assert m.train()(images.cuda())[4] is None
