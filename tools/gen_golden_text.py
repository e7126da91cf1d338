"""TEST INFRASTRUCTURE -- golden vectors of the reference's encode_text.  Runs only where the reference checkout exists:
    python tools/gen_golden_text.py

Imports the real reference (oracle/ref_import.import_reference), registers the tiny text-capable configs of
clipself_amd.config.tiny_text_cfg with both of its factories -- the way oracle/gen_golden.py::_register_tiny / _build_openai do for the
vision fixtures --, loads clipself_amd.init.seeded_text_state into the reference model and runs model.encode_text on the CPU in fp32.
No weights are stored (the tests regenerate them from the seed); every file holds the ids, the unnormalised features and the reference's
text state-dict key -> shape list, and stays far below 1 MiB:

  tests/golden/tiny_text_openai.npz             open_clip CLIP.encode_text (model.py:269-281), context 16, nn.GELU
  tests/golden/tiny_text_openai_quickgelu.npz   ... QuickGELU
  tests/golden/tiny_text_eva.npz                eva_clip CustomCLIP.encode_text -> TextTransformer.forward (transformer.py:722-737)
  tests/golden/tiny_text_ctx77.npz              context 77: lengths 2, 31, 32, 33, 64, 65, 77 (every 32-row tile boundary of the kernel)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from clipself_amd.config import tiny_text_cfg                      # noqa: E402
from clipself_amd.init import seeded_text_state                    # noqa: E402
from oracle.ref_import import import_reference                     # noqa: E402

SEED = 11
VOCAB_EOT = 63                                                     # the largest id of the 64-entry vocabulary


def ids_ctx16(ctx=16, seed=5):
    """Six sequences: the end-of-text id (the largest of the row) at position 1, 5 and 15 (the last), zeros behind it like a
    tokenizer's padding; an all-equal row (argmax = 0); a row with the maximum twice (the first wins: torch.argmax) and ordinary ids
    between and behind; a row of full length: ordinary ids at every position, none of them padding, and the maximum at the last one."""
    g = np.random.Generator(np.random.PCG64(seed))
    ids = np.zeros((6, ctx), np.int64)
    for row, eot in ((0, 1), (1, 5), (2, ctx - 1)):
        ids[row, :eot] = g.integers(1, VOCAB_EOT, size=eot)
        ids[row, eot] = VOCAB_EOT
    ids[3, :] = 7                                                   # degenerate: every position is "the" maximum
    ids[4, :] = g.integers(1, VOCAB_EOT, size=ctx)
    ids[4, 3] = ids[4, 9] = VOCAB_EOT                               # twice: position 3 is the end of text
    ids[5, :] = g.integers(1, VOCAB_EOT - 1, size=ctx)              # full length: no padding at all, end of text (a different id) last
    ids[5, ctx - 1] = VOCAB_EOT - 1
    return ids


def ids_ctx77(ctx=77, seed=6):
    g = np.random.Generator(np.random.PCG64(seed))
    eots = (1, 30, 31, 32, 63, 64, 76)
    ids = np.zeros((len(eots), ctx), np.int64)
    for row, eot in enumerate(eots):
        ids[row, :eot] = g.integers(1, VOCAB_EOT, size=eot)
        ids[row, eot] = VOCAB_EOT
    return ids


def build(oc, cfg):
    """The reference model of cfg with the seeded text tower (its vision tower keeps the factory's own initialisation: never run here)."""
    text_cfg = {"context_length": cfg.text_context, "vocab_size": cfg.text_vocab, "width": cfg.text_width, "heads": cfg.text_heads,
                "layers": cfg.text_layers}
    if cfg.arch == "openai":
        from open_clip import factory
        factory._MODEL_CONFIGS[cfg.name] = {
            "embed_dim": cfg.embed_dim, "quick_gelu": cfg.quick_gelu,
            "vision_cfg": {"image_size": cfg.image_size, "layers": cfg.layers, "width": cfg.width, "patch_size": cfg.patch_size},
            "text_cfg": text_cfg}
        model = oc.create_model(cfg.name, "", device="cpu", precision="fp32")
        prefix = ""
    else:
        from open_clip.eva_clip import factory as eva_factory
        eva_factory._MODEL_CONFIGS[cfg.name] = {
            "embed_dim": cfg.embed_dim,
            "vision_cfg": {"image_size": cfg.image_size, "layers": cfg.layers, "width": cfg.width, "head_width": cfg.head_width,
                           "patch_size": cfg.patch_size, "mlp_ratio": cfg.mlp_ratio, "eva_model_name": "tiny", "drop_path_rate": 0.0,
                           "xattn": False, "fusedLN": False, "rope": True, "pt_hw_seq_len": cfg.pt_hw_seq_len, "intp_freq": True,
                           "naiveswiglu": True, "subln": True},
            "text_cfg": dict(text_cfg, xattn=False, fusedLN=False)}
        model = oc.create_model(cfg.name, "eva", cache_dir=None, device="cpu", precision="fp32")
        prefix = "text."
    sd = seeded_text_state(cfg, SEED)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    text_keys = {k: list(v.shape) for k, v in model.state_dict().items()
                 if (k.startswith("text.") if prefix else not k.startswith("visual.") and k != "logit_scale")}
    assert set(sd) <= set(text_keys) and not (set(text_keys) - set(sd) - {prefix + "attn_mask"}), sorted(set(text_keys) ^ set(sd))
    model.eval()
    return model, text_keys


def main():
    torch.manual_seed(0)
    oc = import_reference()
    gold = ROOT / "tests" / "golden"
    for name, arch, quick, ctx, ids in (("tiny_text_openai", "openai", False, 16, ids_ctx16()),
                                        ("tiny_text_openai_quickgelu", "openai", True, 16, ids_ctx16()),
                                        ("tiny_text_eva", "eva02", False, 16, ids_ctx16()),
                                        ("tiny_text_ctx77", "openai", False, 77, ids_ctx77())):
        cfg = tiny_text_cfg(arch, quick, ctx)
        model, text_keys = build(oc, cfg)
        with torch.no_grad():
            feats = model.encode_text(torch.from_numpy(ids), normalize=False)
        assert feats.shape == (ids.shape[0], cfg.embed_dim) and bool(torch.isfinite(feats).all())
        meta = {"seed": SEED, "cfg": cfg.name, "eot": ids.argmax(-1).tolist(), "state_shapes": text_keys}
        out = gold / f"{name}.npz"
        np.savez_compressed(out, ids=ids.astype(np.int16), features=feats.numpy().astype(np.float32), meta=np.array(json.dumps(meta)))
        assert out.stat().st_size < 2 ** 20, out
        print(name, "eot", meta["eot"], "|f| mean", float(feats.abs().mean()), out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
