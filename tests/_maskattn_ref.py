"""TEST INFRASTRUCTURE -- per-kernel reference of the extra query rows ("passengers") of mask-attention pooling under autograd:
RefOps plus the two grown entry points, cs_attn_query_fwd(lse) and cs_attn_bwd(extra), in torch at the kernels' rounding points
(include/clipself_hip.h).  The frozen oracle/ops_ref.RefOps deliberately lacks them: a tower on it refuses to train through
extract_type='v1'."""
import torch

from oracle.ops_ref import RefOps


def exact_passenger_grads(q, k, v, do, allow, scale, dtype=torch.float64):
    """Autograd of the masked attention o = softmax(scale q k^T | allow) v in `dtype`: q, do [B,H,Q,64]; k, v [B,H,N,64]; allow bool
    [B,Q,N].  A row that allows no key has o = 0 and contributes no gradient.  -> (dq, dk, dv)."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~allow[:, None], float("-inf"))
    none = ~allow.any(-1)[:, None, :, None]                                   # [B,1,Q,1]
    p = torch.softmax(s.masked_fill(none, 0.0), dim=-1).masked_fill(none, 0.0)
    o = p @ v
    return torch.autograd.grad(o, (q, k, v), do.to(dtype))


class RefOpsExtra(RefOps):
    name = "ref+extra"
    ATTN_EXTRA_QUERIES = True

    @staticmethod
    def _heads(t, B, rows, H):
        return t[:, :H * 64].float().reshape(B, rows, H, 64).permute(0, 2, 1, 3)

    def attn_query_fwd(self, q, kv, allow, out, B, Q, Ntok, H, scale, lse=None):
        """RefOps.attn_query_fwd with the kernel's answer for a row that allows no key (zeros, not NaN), plus the log-sum-exp."""
        C = H * 64
        s = (self._heads(q, B, Q, H) @ self._heads(kv[:, :C], B, Ntok, H).transpose(-1, -2)) * scale
        s = s.masked_fill(~allow.view(B, 1, Q, Ntok).bool(), float("-inf"))
        mx = s.max(-1, keepdim=True).values
        none = torch.isinf(mx)
        e = torch.exp(s - torch.where(none, torch.zeros_like(mx), mx))
        den = e.sum(-1, keepdim=True)
        o = (self._r(e) @ self._heads(kv[:, C:2 * C], B, Ntok, H)) / torch.where(none, torch.ones_like(den), den)
        out[:, :C] = o.permute(0, 2, 1, 3).reshape(B * Q, C).to(torch.bfloat16)
        if lse is not None:
            l = mx + torch.log(den)                                           # -inf for a row without keys ...
            lse.view(B * H, Q).copy_(torch.where(none, torch.full_like(l, float("inf")), l).reshape(B * H, Q))      # ... +inf by contract

    def attn_bwd_workspace(self, B, Ntok, H, Q=0):
        return 4

    def attn_bwd(self, qkv, o, dout, lse, cos, sin, dqkv, workspace, B, Ntok, H, scale, extra=None):
        if extra is None:
            return super().attn_bwd(qkv, o, dout, lse, cos, sin, dqkv, workspace, B, Ntok, H, scale)
        if not (bool((cos == 1).all()) and bool((sin == 0).all())):
            raise ValueError("extra query rows need identity rotary tables")
        C, Q = H * 64, extra["Q"]
        if o is not None:
            super().attn_bwd(qkv, o, dout, lse, cos, sin, dqkv, workspace, B, Ntok, H, scale)
        else:
            dqkv[:, :3 * C] = 0
        r = self._r
        k, v = self._heads(qkv[:, C:2 * C], B, Ntok, H), self._heads(qkv[:, 2 * C:3 * C], B, Ntok, H)
        q, of, do = self._heads(extra["q"], B, Q, H), self._heads(extra["o"], B, Q, H), self._heads(extra["dout"], B, Q, H)
        allow = extra["allow"].view(B, 1, Q, Ntok).bool()
        s = (q @ k.transpose(-1, -2)) * scale
        p = torch.exp(s - extra["lse"].view(B, H, Q, 1))                      # lse = +inf: exp(-inf) = 0
        p = torch.where(allow, p, torch.zeros_like(p))
        dsum = (do * of).sum(-1, keepdim=True)
        ds = r(p * (do @ v.transpose(-1, -2) - dsum) * scale)
        back = lambda t, rows: t.permute(0, 2, 1, 3).reshape(B * rows, C)
        extra["dq"][:, :C] = back(ds @ k, Q).to(torch.bfloat16)
        dk, dv = back(ds.transpose(-1, -2) @ q, Ntok), back(r(p).transpose(-1, -2) @ do, Ntok)
        # the kernel adds the passengers' fp32 sums to the rounded image-row gradient and rounds once more
        dqkv[:, C:2 * C] = (dqkv[:, C:2 * C].float() + dk).to(torch.bfloat16)
        dqkv[:, 2 * C:3 * C] = (dqkv[:, 2 * C:3 * C].float() + dv).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the training fixture and its recipes
RECIPES = ("blocks/", "stem/", "stem64/", "all/", "q/blocks/")


def load_gold(golden_dir):
    """tests/golden/tiny_openai_maskattn_grad*.npz (tools/gen_golden_maskattn_grad.py; several files, each below 1 MiB) as one dict."""
    import numpy as np
    blob = {}
    files = sorted(golden_dir.glob("tiny_openai_maskattn_grad*.npz"))
    assert len(files) == 5, files
    for f in files:
        with np.load(f) as g:
            blob.update({k: g[k] for k in g.files})
    return blob


def recipe_of(gold, tag):
    import json
    return json.loads(str(gold[tag + "recipe"]))


def batch_for(rec, step):
    from clipself_amd.init import synthetic_batch
    images, boxes, crops = synthetic_batch(2, 3, rec["image_size"], 32, seed=rec["seed_b"] + step)
    boxes[1, 2, -1] = 0                                           # 3 + 2 valid boxes: a padding passenger, the non-dense rois path
    return images, boxes, crops


def oracle_loss(student_sd, teacher_sd, cfg, batch, emulate_bf16=False):
    """CLIPSelf.__call__ with extract_type='v1' on the restatement (oracle/clip_vit_ref.py)."""
    import torch.nn.functional as F
    from oracle import clip_vit_ref, eva_ref
    images, boxes, crops = batch
    rois, crops = eva_ref.split_valid(boxes, crops)
    with torch.no_grad():
        teacher = clip_vit_ref.encode_image(teacher_sd, cfg, crops)
    student = clip_vit_ref.extract_roi_features_v1(student_sd, cfg, images, rois, emulate_bf16=emulate_bf16)
    return 1.0 - (F.normalize(student, dim=-1) * F.normalize(teacher, dim=-1)).sum(-1).mean()


def oracle_grads(cfg, rec, batch, emulate_bf16=False, dtype=torch.float32):
    from clipself_amd.init import seeded_visual_state
    from oracle import clip_vit_ref
    student = {k: v.to(dtype) for k, v in seeded_visual_state(cfg, rec["seed_w"]).items()}
    teacher = {k: v.to(dtype) for k, v in seeded_visual_state(cfg, rec["seed_t"]).items()}
    names = [n for n in clip_vit_ref.trainable_names(student, cfg, rec["unlocked"] if rec["lock"] else -1) if n in student]
    for n in names:
        student[n].requires_grad_(True)
    loss = oracle_loss(student, teacher, cfg, tuple(t.to(dtype) for t in batch), emulate_bf16)
    loss.backward()
    return float(loss.detach()), {n: student[n].grad for n in names}


def build_pair(cfg, rec, student_ops, teacher_ops):
    """(student, teacher) CLIP models of a recipe: student seed / lock of the recipe, teacher from its own seed."""
    from clipself_amd.init import seeded_visual_state
    from clipself_amd.open_clip import CLIP
    student, teacher = CLIP(cfg, ops=student_ops, trainable=True), CLIP(cfg, ops=teacher_ops, trainable=False)
    student.visual.engine.load_state(seeded_visual_state(cfg, rec["seed_w"]))
    teacher.visual.engine.load_state(seeded_visual_state(cfg, rec["seed_t"]))
    if rec["lock"]:
        student.lock_image_tower(unlocked_groups=rec["unlocked"])
    student.train()
    return student, teacher


def run_recipe(student, teacher, rec, steps, device="cpu", hook=None):
    """`steps` steps of CLIPSelf()(extract_type='v1') + the engine's AdamW.  -> (losses, first-step gradients by name (clones))."""
    from types import SimpleNamespace
    from clipself_amd.training.clipself import CLIPSelf
    from oracle import eva_ref
    eng = student.visual.engine
    args = SimpleNamespace(multiscale=False, extract_type="v1", cosine_weight=1.0)
    method, losses, first = CLIPSelf(), [], {}
    for step in range(steps):
        eng.zero_grad()
        eng.grad_ready_hook = hook
        out, bs, _ = method(batch_for(rec, step), student, teacher, None, device, None, False, args)
        assert bs == 2
        sum(out.values()).backward()
        eng.grad_ready_hook = None
        if step == 0:
            first = {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.grad is not None}
        eng.adamw_step(step + 1, eva_ref.cosine_lr_value(step, rec["lr"], rec["warmup"], rec["total"]), rec["wd"])
        losses.append(float(sum(out.values()).detach()))
    return losses, first
