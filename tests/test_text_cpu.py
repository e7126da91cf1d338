"""encode_text on the CPU: the frozen text tower's schedule (clipself_amd/engine_text.py) through the model API of both families, on
tests/_text_ref.RefOpsText -- RefOps plus causal attention at the kernel's rounding points -- against vectors of the real reference
(tools/gen_golden_text.py).  The GPU twin is tests/test_gpu_text.py; the bounds are derived in profiles/text_tower_parity.md."""
import numpy as np
import pytest
import torch

from _text_ref import BOUND_ONE_MINUS_COS, BOUND_REL_L2, BOUND_SAME_ROUNDING, FIXTURES, RefOpsText, build_model, load_fixture, one_minus_cos, rel_l2
from oracle.ops_ref import RefOps

_RUNS = {}


def runs(name):
    """(cfg, ids, golden, shapes, model, trimmed features, untrimmed features) of a fixture, computed once."""
    if name not in _RUNS:
        cfg, ids, feats, shapes, seed = load_fixture(name)
        model = build_model(cfg, RefOpsText(), seed)
        _RUNS[name] = (cfg, ids, feats, shapes, model, model.encode_text(ids), model.encode_text(ids, trim=False))
    return _RUNS[name]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_encode_text_matches_the_reference(name):
    """Trimmed and trim=False runs are both within the golden bound; trimming is exact under the causal mask (their difference is
    printed: 0 on this backend, whose attention is one pass whatever the padded length)."""
    cfg, ids, gold, _, model, trimmed, full = runs(name)
    assert trimmed.shape == gold.shape == (ids.shape[0], cfg.embed_dim) and trimmed.dtype == torch.float32
    for tag, got in (("trimmed", trimmed), ("trim=False", full)):
        r, c = rel_l2(got, gold), one_minus_cos(got, gold)
        print(f"{name} {tag}: rel-L2 {r:.3e}  max(1 - cos) {c:.3e}")
        assert r <= BOUND_REL_L2 and c <= BOUND_ONE_MINUS_COS, (name, tag, r, c)
    print(f"{name}: max |trimmed - untrimmed| = {float((trimmed - full).abs().max()):.3e}")
    assert rel_l2(trimmed, full) <= BOUND_SAME_ROUNDING      # the same arithmetic on fewer rows


def test_first_maximum_is_the_end_of_text():
    """torch.argmax semantics: a row with the maximum twice pools its first occurrence, an all-equal row position 0 -- so rows that differ
    only behind that position (where a causal tower cannot look) give identical features."""
    cfg, ids, gold, _, model, trimmed, _ = runs("tiny_text_openai")
    assert ids.argmax(-1).tolist() == [1, 5, 15, 0, 3, 15]
    other = ids.clone()
    other[4, 4:] = 1                      # behind the first maximum (position 3), the second maximum included
    other[3, 1:] = 0                      # behind position 0 of the all-equal row: still the (first) maximum
    assert torch.equal(model.encode_text(other)[[3, 4]], trimmed[[3, 4]])


def test_normalize_gives_unit_rows():
    cfg, ids, _, _, model, trimmed, _ = runs("tiny_text_eva")
    n = model.encode_text(ids, normalize=True)
    assert torch.allclose(n.norm(dim=-1), torch.ones(ids.shape[0]), atol=1e-6)
    assert torch.allclose(n, torch.nn.functional.normalize(trimmed, dim=-1))


@pytest.mark.parametrize("name", ["tiny_text_openai", "tiny_text_eva"])
def test_state_dict_keys_and_shapes_are_the_reference_list(name):
    """Text keys and shapes of state_dict() equal what the reference model listed.  (`text.attn_mask`: a non-persistent buffer in the
    reference; the EVA-family tower here has always listed it, the OpenAI-family one never -- unchanged, and checked as exactly that.)"""
    cfg, _, _, shapes, model, _, _ = runs(name)
    ours = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith("visual.") and k != "logit_scale"}
    mask = {k for k in ours if k.endswith("attn_mask")}
    assert mask == ({"text.attn_mask"} if cfg.arch != "openai" else set())
    assert {k: v for k, v in ours.items() if k not in mask} == shapes
    for k in mask:
        assert ours[k] == (cfg.text_context, cfg.text_context)


def test_text_tower_stays_frozen_and_untouched():
    cfg, ids, _, _, _, _, _ = runs("tiny_text_openai")
    from clipself_amd.init import seeded_text_state
    sd = seeded_text_state(cfg, 11)
    model = build_model(cfg, RefOpsText(), 11)
    model.train()
    out = model.encode_text(ids)
    assert not out.requires_grad and out.grad_fn is None and out.device == model.visual.engine.device
    tower = model._text_tower()
    assert tower._engine is not None
    for safe, k in tower._names.items():
        p = tower._parameters[safe]
        assert not p.requires_grad and p.grad is None and torch.equal(p.detach().cpu(), sd[k]), k


def test_weight_shadows_are_lazy_and_follow_a_load():
    """No engine (no bf16 copies) until the first encode_text; a load_state_dict afterwards is seen by the next call."""
    cfg, ids, _, _, _, trimmed, _ = runs("tiny_text_openai")
    from clipself_amd.init import seeded_text_state
    model = build_model(cfg, RefOpsText(), 11)
    assert model._text_tower()._engine is None
    assert torch.equal(model.encode_text(ids), trimmed)
    model.load_state_dict(seeded_text_state(cfg, 12), strict=False)
    other = model.encode_text(ids)
    assert not torch.allclose(other, trimmed, atol=1e-2)
    model.load_state_dict(seeded_text_state(cfg, 11), strict=False)
    assert torch.equal(model.encode_text(ids), trimmed)
    # a write through .data advances no version counter: invalidate() is the documented way to announce it
    tower = model._text_tower()
    proj = tower._parameters["text_projection"]
    proj.data.copy_(proj.data * 2)
    tower.invalidate()
    assert torch.allclose(model.encode_text(ids), 2 * trimmed, rtol=2e-2, atol=1e-3)


def test_chunks_are_trimmed_separately_to_the_same_features():
    cfg, ids, _, _, model, trimmed, _ = runs("tiny_text_ctx77")
    tower = model._text_tower()
    assert rel_l2(tower(ids, chunk=2), trimmed) <= BOUND_SAME_ROUNDING       # chunks of 2: trimmed to 32, 33, 65 and 77 positions instead of 77
    assert tower(ids[:0]).shape == (0, cfg.embed_dim)


def test_error_paths():
    cfg, ids, _, _, model, _, _ = runs("tiny_text_openai")
    for bad in (ids.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(-1)),                  # id < 0
                ids.clone().index_put_((torch.tensor(2), torch.tensor(3)), torch.tensor(cfg.text_vocab)),      # id >= vocab
                ids[0], ids[None], ids.float(), ids[:, :-1], torch.cat([ids, ids[:, :1]], dim=1)):             # not 2-D / not integer / not ctx wide
        with pytest.raises(ValueError):
            model.encode_text(bad)
    from clipself_amd.open_clip import CLIP, CustomCLIP
    from clipself_amd.config import tiny_text_cfg
    for cls, c in ((CLIP, cfg), (CustomCLIP, tiny_text_cfg("eva02"))):
        with pytest.raises(RuntimeError, match="with_text"):
            cls(c, ops=RefOpsText(), trainable=False, with_text=False).encode_text(ids)
    with pytest.raises(NotImplementedError, match="ATTN_CAUSAL"):                                               # the plain frozen RefOps
        build_model(cfg, RefOps(), 11).encode_text(ids)
    with pytest.raises(NotImplementedError, match="ATTN_CAUSAL"):
        build_model(tiny_text_cfg("eva02"), RefOps(), 11).text(ids)
    # the old tiny configs keep their head-dim-16 text tower: it constructs and checkpoints as before, and refuses to run
    from clipself_amd.config import tiny_openai_cfg
    small = tiny_openai_cfg()
    with pytest.raises(NotImplementedError, match="head-dim-64"):
        CLIP(small, ops=RefOpsText(), trainable=False).encode_text(torch.zeros(2, small.text_context, dtype=torch.long))


def test_text_embeddings_tool_pools_like_the_reference_tool(tmp_path):
    """3 classes x 2 templates: normalise each template's feature, mean over the templates, normalise again -- from [N, T, ctx] and from
    [N*T, ctx] ids, and from a .npy file as the command line reads it."""
    import sys
    from pathlib import Path
    tools = Path(__file__).resolve().parent.parent / "tools"
    sys.path.insert(0, str(tools))
    try:
        import text_embeddings
    finally:
        sys.path.remove(str(tools))
    cfg, ids, _, _, model, trimmed, _ = runs("tiny_text_openai")
    f = torch.nn.functional.normalize(trimmed, dim=-1)
    want = torch.stack([torch.nn.functional.normalize((f[2 * n] + f[2 * n + 1]) / 2, dim=0) for n in range(3)])
    for arr in (ids.numpy().reshape(3, 2, -1), ids.numpy()):
        got = text_embeddings.class_embeddings(model, arr, templates=2)
        assert got.shape == (3, cfg.embed_dim) and got.dtype == torch.float32
        assert torch.allclose(got, want, atol=1e-6)
        assert torch.allclose(got.norm(dim=-1), torch.ones(3), atol=1e-6)
    got3 = text_embeddings.class_embeddings(model, ids.numpy(), templates=2, batch=4)      # batches that split the id list
    assert torch.allclose(got3, want, atol=1e-6)
    np.save(tmp_path / "ids.npy", ids.numpy().reshape(3, 2, -1))
    assert text_embeddings.class_embeddings(model, np.load(tmp_path / "ids.npy"), templates=2).equal(got)
    with pytest.raises(ValueError):
        text_embeddings.class_embeddings(model, ids.numpy()[:5], templates=2)
    with pytest.raises(ValueError):
        text_embeddings.class_embeddings(model, ids.numpy().reshape(2, 3, -1), templates=2)
