"""`-m gpu`: the detector's kernel-backed modules chained through one training step and one inference pass on the MI355X
(tests/_det_chain.py): every layer and every functional module on HipOps.  The same checks as tests/test_det_chain_cpu.py
-- forward seams stage by stage, backward seams bit for bit by replay, the loss terms against the float64 torch route, a live assembly
against a fresh one after the weights change, empty and ragged rows -- at B = 3 images of 128 x 128 and C = 64, where each step takes a
fraction of a second.  Every printed figure of a run is recorded in profiles/det_chain_parity.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _det_chain as D  # noqa: E402

TAG = "MI355X"
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def batch():
    return D.make_batch(0, device=DEV)


@pytest.fixture(scope="module")
def keys():
    return D.make_keys(0, device=DEV)


def _assembly(hip, seed=0):
    return D.Assembly(True, hip, seed=seed).to(DEV)


@pytest.fixture(scope="module")
def chain(hip, batch, keys):
    """(assembly, record) of the kernel route's first step, the rows past `counts` poisoned with NaN; shared read-only."""
    asm = _assembly(hip)
    rec = D.train_step(asm, batch, keys, poison=True)
    torch.cuda.synchronize()
    return asm, rec


def test_every_stage_ran_its_kernels(chain):
    asm, rec = chain
    want = {"fpn0": "_BatchNormActFn", "rpn_cls0": "_ThinFn", "rpn_reg4": "_ThinFn", "roi_feats": "_RoIExtract", "trunk": "_LinearActFn",
            "bbox_pred": "_LinearThinFn", "mask_feats": "_RoIExtract", "mask_pred": "_MaskTailFn"}
    for name, fn in want.items():
        assert rec.fns[name].startswith(fn), (name, rec.fns[name])
    assert all(rec[k].is_cuda for k in ("proposals", "rois", "mask_targets", "total"))
    assert rec["rpn_cls0"].is_contiguous() and rec["rpn_cls0"].dtype == torch.float32 and not rec["roi_feats"].is_contiguous()
    counts = rec["counts"].tolist()
    assert min(counts) < D.TRAIN_CFG["rpn_proposal"]["max_per_img"] and rec["pos_idx"].numel() > 0, (counts, rec["pos_idx"].numel())


def test_forward_seams_stage_by_stage(chain, batch, keys):
    asm, rec = chain
    D.check_forward(rec, asm, batch, keys, TAG)


def test_backward_seams_by_replay(chain, hip):
    asm, rec = chain
    D.check_replay(rec, asm, hip, TAG)


def test_loss_terms_against_the_float64_torch_route(chain, batch, keys):
    _, rec = chain
    D.check_scalars(rec, batch, keys, TAG)


def test_ragged_rows_never_reach_a_head_or_a_loss(chain):
    asm, rec = chain
    D.check_ragged(rec, asm, TAG)


def test_the_step_is_deterministic(chain, hip, batch, keys):
    asm, rec = chain
    again = D.train_step(D.fresh_like(asm, hip, rec.state), batch, keys, poison=True)
    D.same_records(rec, again, "the same step on a second assembly")


def test_a_batch_without_any_positive(hip, keys):
    neg = D.make_batch(1, negatives_only=True, device=DEV)
    asm = _assembly(hip)
    rec = D.train_step(asm, neg, keys, poison=True)
    assert rec["pos_idx"].numel() == 0 and tuple(rec["mask_feats"].shape) == (0, D.C, 14, 14) and rec.fns["mask_feats"].startswith("_RoIExtract")
    assert float(rec["loss_mask"]) == 0.0
    D.check_ragged(rec, asm, TAG)
    for k, g in rec.param_grads.items():
        if k.startswith("mask_head."):
            assert g is None, k                                                       # as on the torch route (tests/test_det_chain_cpu.py)
    D.check_replay(rec, asm, hip, TAG + ", no positive")
    D.check_scalars(rec, neg, keys, TAG + ", no positive")


def _changed(asm, how):
    if how in ("sgd", "sgd_foreach"):
        torch.optim.SGD(asm.parameters(), lr=0.01, momentum=0.9, foreach=(how == "sgd_foreach")).step()
    elif how == "adamw_fused":
        torch.optim.AdamW(asm.parameters(), lr=1e-3, fused=True).step()
    elif how == "load_state_dict":
        asm.load_state_dict(D.Assembly(True, seed=1).state_dict(), strict=True)
    elif how == "data_clone":
        for p in asm.parameters():
            p.data = p.data.clone().mul_(1.03125)
    else:
        raise AssertionError(how)


@pytest.mark.parametrize("how", ["sgd", "sgd_foreach", "adamw_fused", "load_state_dict", "data_clone"])
def test_a_live_assembly_equals_a_fresh_one_after_the_weights_change(hip, batch, keys, how):
    asm = _assembly(hip)
    first = D.train_step(asm, batch, keys)                                           # warms every cache and workspace
    _changed(asm, how)
    live = D.train_step(asm, batch, keys)
    assert not D.bits_equal(first["fpn0"], live["fpn0"]) and not D.bits_equal(first["bbox_pred"], live["bbox_pred"])
    fresh = D.train_step(D.fresh_like(asm, hip, live.state), batch, keys)
    D.same_records(live, fresh, f"step 2 after {how}: live against fresh assembly")
    if how != "sgd":
        return
    stats = {k: v.clone() for k, v in asm.state_dict().items() if "running_" in k or "num_batches" in k}
    out = D.infer(asm, batch)
    for k, v in asm.state_dict().items():
        if k in stats:
            assert torch.equal(v, stats[k]), f"infer changed {k}"
    other = D.infer(D.fresh_like(asm, hip), batch)
    D.same_records(out, other, "infer: trained live assembly against a fresh one in eval()")
    print(f"DET CHAIN [{TAG}] (d) infer: proposals {out['counts'].tolist()}, detections {out['det_counts'].tolist()}, "
          f"pasted pixels {int(out['pasted'].sum())}")
    assert not asm.training and sum(out["det_counts"].tolist()) > 0
