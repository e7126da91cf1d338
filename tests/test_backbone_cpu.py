"""CPU: the detector backbone's frozen pass -- TowerEngine.encode_dense(taps=, final=), EVAVisionTower.forward_intermediates and
clipself_amd.fvit.EvaCLIPViT -- on the per-kernel references (tests/_backbone_ref.RefOpsBackbone) against the golden vectors of the real
reference tower driven in the order of F-ViT/models/evaclip_vit.py:61-106 (tools/gen_golden_fvit.py).

Bounds.  Taps and map come out of the bf16-operand schedule and are compared with an fp32 reference: rel-L2 2e-2, the bound this suite
already holds the dense map and the features of that schedule to against the fp32 reference (tests/test_engine_cpu.py) -- bf16 rounds at
2^-9 relative, a block has about ten rounding points, four blocks: sqrt(40) * 2^-9 = 1.2e-2 if every rounding hit the full value.  For
unit vectors 1 - cos = |difference|^2 / 2 <= (2e-2)^2 / 2 = 2e-4.  The neck (fp32 torch on both sides) adds float rounding only: 1e-5."""
import pytest
import torch
import torch.nn.functional as F

from _backbone_ref import FIXTURES, OUT_INDICES, RefOpsBackbone, backbone_cfg, build_tower, load_fixture, one_minus_cos, rel_l2
from oracle.ops_ref import RefOps

TOL_REL, TOL_COS = 2e-2, 2e-4


@pytest.fixture(scope="module")
def ops():
    return RefOpsBackbone()


@pytest.fixture(scope="module")
def towers(ops):
    return {}


def _tower(towers, ops, seed):
    if seed not in towers:
        towers[seed] = build_tower(ops, seed)
    return towers[seed]


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_intermediates_matches_the_reference_backbone_pass(towers, ops, name):
    images, taps, fmap, seed = load_fixture(name)
    tower = _tower(towers, ops, seed)
    got_taps, got_map = tower.forward_intermediates(images, OUT_INDICES)
    assert len(got_taps) == 4 and not got_map.requires_grad and not any(t.requires_grad for t in got_taps)
    for i, (got, want) in enumerate(zip(got_taps, taps)):
        assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
        r = rel_l2(got, want)
        print(f"{name} tap{i}: rel-L2 {r:.3e}")
        assert r < TOL_REL, (name, i, r)
    r, c = rel_l2(got_map, fmap), one_minus_cos(got_map, fmap)
    print(f"{name} map: rel-L2 {r:.3e}, 1-cos {c:.3e}")
    assert got_map.shape == fmap.shape and r < TOL_REL and c < TOL_COS, (name, r, c)
    # the map is the view of encode_dense's, value for value
    assert torch.equal(got_map, tower.encode_dense(images, keep_shape=True))
    # bf16 taps: one rounding of the fp32 ones
    bf_taps, _ = tower.forward_intermediates(images, OUT_INDICES, dtype=torch.bfloat16)
    assert all(torch.equal(b, t.to(torch.bfloat16)) for b, t in zip(bf_taps, got_taps))
    # a subset of the blocks, the last one alone
    sub, _ = tower.forward_intermediates(images, [1, 3])
    assert len(sub) == 2 and torch.equal(sub[0], got_taps[1]) and torch.equal(sub[1], got_taps[3])


class _Recorder:
    """Forwards every op to the wrapped backend and records its name."""

    def __init__(self, inner):
        self._inner, self.calls = inner, []
        self.name = inner.name
        self.TOKEN_TAPS = getattr(inner, "TOKEN_TAPS", False)

    def __getattr__(self, attr):
        fn = getattr(self._inner, attr)
        if not callable(fn):
            return fn

        def call(*a, **k):
            self.calls.append(attr)
            return fn(*a, **k)
        return call


def _launches(calls):
    return [c for c in calls if c not in ("empty", "zeros")]


def test_taps_add_one_launch_each_and_training_mode_skips_the_tail(ops):
    images, _, _, seed = load_fixture(FIXTURES[0])
    rec = _Recorder(ops)
    tower = build_tower(rec, seed)
    eng = tower.engine
    rec.calls.clear()
    plain, g = eng.encode_dense(images)
    base = _launches(rec.calls)
    assert "tokens_to_nchw" not in base
    rec.calls.clear()
    dense, g2, maps = eng.encode_dense(images, taps=(0, 1, 2, 3))
    tapped = _launches(rec.calls)
    # the same launches in the same order, plus one copy after each tapped block; the map is bit-identical
    assert [c for c in tapped if c != "tokens_to_nchw"] == base and tapped.count("tokens_to_nchw") == 4
    assert torch.equal(dense, plain) and g2 == g and len(maps) == 4
    # the last tap follows the last block and precedes the tail: final LayerNorm, head GEMM, normalisation
    assert tapped[-4:] == ["tokens_to_nchw", "layernorm_fwd", "gemm_nt", "l2norm_fwd"]
    rec.calls.clear()
    none, _, maps2 = eng.encode_dense(images, taps=(0, 1, 2, 3), final=False)
    train = _launches(rec.calls)
    assert none is None and train == tapped[:-3] and "l2norm_fwd" not in train
    assert all(torch.equal(a, b) for a, b in zip(maps, maps2))


def test_errors(ops):
    images, _, _, seed = load_fixture(FIXTURES[0])
    tower = build_tower(ops, seed)
    eng = tower.engine
    for bad in ((0, 4), (-1, 2), (2, 1), (1, 1)):                       # out of range (4 blocks), negative, descending, repeated
        with pytest.raises(ValueError):
            eng.encode_dense(images, taps=bad)
        with pytest.raises(ValueError):
            tower.forward_intermediates(images, list(bad))
    with pytest.raises(ValueError, match="need_grad"):
        eng.encode_dense(images, need_grad=True, taps=(0,))
    with pytest.raises(ValueError):
        eng.encode_dense(images, need_grad=True, final=False)
    plain = build_tower(RefOps(), seed)                                # the frozen oracle backend has no token taps
    with pytest.raises(NotImplementedError, match="TOKEN_TAPS"):
        plain.forward_intermediates(images, OUT_INDICES)
    dense, g = plain.engine.encode_dense(images)                       # ... and runs everything else as before
    assert torch.equal(dense, eng.encode_dense(images)[0])


@pytest.fixture()
def backbone_factory(monkeypatch, tmp_path, ops):
    """EvaCLIPViT builds its tower through create_model(model_name, pretrained='eva', cache_dir=<checkpoint>): the miniature's config under a
    name of its own, its seeded weights in a checkpoint file."""
    from clipself_amd import fvit
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import factory
    cfg = backbone_cfg()
    real = factory.get_tower_cfg
    monkeypatch.setattr(factory, "get_tower_cfg", lambda n: cfg if n == cfg.name else real(n))

    def make(seed, **kw):
        ckpt = tmp_path / f"seed{seed}.pt"
        torch.save(seeded_visual_state(cfg, seed), ckpt)
        return fvit.EvaCLIPViT(cfg.name, str(ckpt), ops=ops, **kw)
    return make


@pytest.mark.parametrize("name", FIXTURES)
def test_backbone_module_matches_the_reference(backbone_factory, name):
    images, taps, fmap, seed = load_fixture(name)
    torch.manual_seed(3)
    m = backbone_factory(seed, out_indices=OUT_INDICES, norm_cfg=dict(type="BN", requires_grad=True))
    assert m.embed_dim == 64 and m.width == 128 and m.patch_size == 8
    assert isinstance(m.interpolate1[1], torch.nn.BatchNorm2d) and isinstance(m.interpolate3, torch.nn.Identity)
    assert not any(p.requires_grad for p in m.visual.parameters()) and all(p.requires_grad for p in m.interpolate1.parameters())
    m.eval()
    outs = m(images)
    assert isinstance(outs, tuple) and len(outs) == 5
    h = images.shape[-1] // 8
    assert [o.shape[-1] for o in outs] == [4 * h, 2 * h, h, h // 2, h]
    with torch.no_grad():
        want = [m.interpolate1(taps[0]), m.interpolate2(taps[1]), taps[2], F.max_pool2d(taps[3], 2, 2)]
    for i in range(4):
        r = rel_l2(outs[i], want[i])
        print(f"{name} out{i}: rel-L2 {r:.3e}")
        assert outs[i].shape == want[i].shape and r < TOL_REL, (i, r)
    assert rel_l2(outs[4], fmap) < TOL_REL and one_minus_cos(outs[4], fmap) < TOL_COS
    assert outs[0].requires_grad and outs[1].requires_grad and not outs[4].requires_grad      # the neck trains, the tower does not
    # training mode: the tower stays in evaluation mode, the neck follows, no map
    m.train()
    assert m.training and m.interpolate1.training and not m.visual.training
    tr = m(images)
    assert tr[4] is None and len(tr) == 5
    assert rel_l2(tr[2], outs[2]) == 0 and rel_l2(tr[3], outs[3]) == 0
    tr[0].sum().backward()
    assert m.interpolate1[0].weight.grad is not None and all(p.grad is None for p in m.visual.parameters())
    # init_weights reloads the checkpoint into the tower and keeps it frozen
    with torch.no_grad():
        m.visual.engine.p["visual.norm.weight"].add_(1.0)
    m.init_weights()
    m.eval()
    again = m(images)
    assert torch.equal(again[4], outs[4]) and not any(p.requires_grad for p in m.visual.parameters())


def test_backbone_module_wants_four_taps_and_known_norms(backbone_factory):
    images, _, _, seed = load_fixture(FIXTURES[0])
    m = backbone_factory(seed, out_indices=[0, 1, 3])
    assert isinstance(m.interpolate1[1], torch.nn.Identity)
    with pytest.raises(AssertionError):
        m.eval()(images)
    from clipself_amd.fvit import build_norm
    assert isinstance(build_norm(dict(type="SyncBN", requires_grad=True), 8), torch.nn.SyncBatchNorm)
    frozen = build_norm(dict(type="BN", requires_grad=False), 8)
    assert not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(NotImplementedError):
        build_norm(dict(type="GN", num_groups=2), 8)


def test_the_kernel_reference_drops_the_cls_rows_and_respects_the_row_stride(ops):
    B, N, C, ld = 2, 10, 12, 16
    x = torch.randn(B * N, ld)
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(B, C, 3, 3, dtype=dt)
        ops.tokens_to_nchw(x[:, :C], B, N, C, out)
        assert torch.equal(out, x.view(B, N, ld)[:, 1:, :C].permute(0, 2, 1).reshape(B, C, 3, 3).to(dt))
