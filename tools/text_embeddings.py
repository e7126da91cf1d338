"""Class text embeddings from token ids: the file the `--train-embed-path` / `dataloader.dataset.embeddings`-style arguments of the
shipped flows consume (RegionCLIP's noun bank, the zero-shot region evaluation).

    python tools/text_embeddings.py --ids ids.npy --templates T --model EVA02-CLIP-B-16 --checkpoint ckpt.pt --out classes.npy

ids.npy holds token ids [N, T, context] or [N*T, context] (class-major: the T prompt templates of a class are adjacent); tokenisation is
not part of this project.  Pooling: every template's feature is normalised, the T features of a class are averaged, and the mean is
normalised again -> fp32 [N, E].
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def class_embeddings(model, ids, templates: int, batch: int = 4096):
    """ids: integer array / tensor [N, T, ctx] or [N*T, ctx] -> fp32 tensor [N, E] on the CPU."""
    ids = torch.as_tensor(np.asarray(ids) if not isinstance(ids, torch.Tensor) else ids)
    if ids.dim() == 3:
        if ids.shape[1] != templates:
            raise ValueError(f"ids are [N, T, ctx] with T = {ids.shape[1]}, but --templates is {templates}")
        ids = ids.reshape(-1, ids.shape[-1])
    if ids.dim() != 2 or templates < 1 or ids.shape[0] % templates:
        raise ValueError(f"ids must be [N, T, ctx] or [N*T, ctx] with T = {templates}, got {tuple(ids.shape)}")
    ids = ids.long()
    feats = torch.cat([model.encode_text(ids[k:k + batch], normalize=True).float().cpu() for k in range(0, ids.shape[0], batch)])
    return F.normalize(feats.view(-1, templates, feats.shape[-1]).mean(dim=1), dim=-1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ids", required=True, help=".npy of token ids [N, T, ctx] or [N*T, ctx]")
    ap.add_argument("--templates", type=int, default=1, help="prompt templates per class (T)")
    ap.add_argument("--model", required=True)
    ap.add_argument("--checkpoint", default=None, help="EVA family: the checkpoint file; OpenAI family: an open_clip checkpoint")
    ap.add_argument("--pretrained", default=None, help="as in open_clip.create_model (default: 'eva' for EVA towers, the checkpoint otherwise)")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from clipself_amd.config import get_tower_cfg
    from clipself_amd.open_clip import create_model
    if get_tower_cfg(args.model).arch == "openai":
        model = create_model(args.model, args.pretrained or args.checkpoint, trainable=False, require_pretrained=bool(args.checkpoint))
    else:
        model = create_model(args.model, args.pretrained or "eva", cache_dir=args.checkpoint, trainable=False,
                             require_pretrained=bool(args.checkpoint))
    out = class_embeddings(model, np.load(args.ids), args.templates, args.batch)
    np.save(args.out, out.numpy().astype(np.float32))
    print(f"wrote {args.out}: {tuple(out.shape)}")


if __name__ == "__main__":
    main()
