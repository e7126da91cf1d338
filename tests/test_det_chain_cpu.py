"""`-m "not gpu"`: the detector's kernel-backed modules chained through one training step and one inference pass (tests/_det_chain.py,
DESIGN.md §3.26).  The layers run their kernel route on the CPU backend tests/_thin_wgrad_ref.RefOpsThinWgrad; the functional modules
(targets, losses, proposals, extractor, masks, post-processing) have no CPU kernel form and take their torch routes.  The module tests pin
every module alone; these pin the seams: what one module hands to the next, gradients that two or more consumers add into one tensor,
a module called on five levels before any backward runs, the packed-weight caches across an optimizer step, empty and ragged rows.
Every printed figure of a run is recorded in profiles/det_chain_parity.md."""
import contextlib
import io

import pytest
import torch

import _det_chain as D
from _thin_wgrad_ref import RefOpsThinWgrad

TAG = "CPU backend"
# which check must reject which planted seam error, and the stage its message must name (an assertion of another stage, a shape
# assertion among them, does not count)
REJECTED_BY = {"levels_swapped": ("a", "(a) roi_feats:"), "rpn_consumer_detached": ("b", "(b) FPN output 0:"),
               "fc_flatten_nchw": ("b", "(b) shared FCs:"), "proposals_xywh": ("a", "(a) rcnn_targets: rois differ"),
               "stale_pack": ("d", "live against fresh assembly:"), "padding_rows_used": ("e", "(e) image 1:")}


@pytest.fixture(scope="module")
def ops():
    return RefOpsThinWgrad()


@pytest.fixture(scope="module")
def batch():
    return D.make_batch(0)


@pytest.fixture(scope="module")
def keys():
    return D.make_keys(0)


@pytest.fixture(scope="module")
def chain(ops, batch, keys):
    """(assembly, record) of the kernel route's first step, the rows past `counts` poisoned with NaN; shared read-only."""
    asm = D.Assembly(True, ops)
    rec = D.train_step(asm, batch, keys, poison=True)
    return asm, rec


def _changed(asm, how):
    """Change every parameter of the live assembly in one of the ways a training script does."""
    if how == "sgd":
        torch.optim.SGD(asm.parameters(), lr=0.01, momentum=0.9).step()
    elif how == "adamw_fused":                                                       # moves no version counter and no storage
        torch.optim.AdamW(asm.parameters(), lr=1e-3, fused=True).step()
    elif how == "load_state_dict":
        asm.load_state_dict(D.Assembly(asm.fused, seed=1).state_dict(), strict=True)
    elif how == "data_clone":
        for p in asm.parameters():
            p.data = p.data.clone().mul_(1.03125)
    else:
        raise AssertionError(how)


# ------------------------------------------------------------------------------------------------ the batch, on the reference route
def test_the_batch_reaches_every_path_on_the_torch_route(batch, keys):
    rec = D.train_step(D.Assembly(False), batch, keys)
    counts = rec["counts"].tolist()
    num = D.TRAIN_CFG["rcnn"]["sampler"]["num"]
    pos = ((rec["labels"] < D.NUM_CLASSES) & (rec["lw"] > 0)).reshape(D.B, num).sum(1).tolist()
    print(f"DET CHAIN [torch route] proposals per image {counts}, sampled positives per image {pos}")
    assert min(counts) < D.TRAIN_CFG["rpn_proposal"]["max_per_img"], counts        # a short proposal list
    assert min(pos) == 0 and pos[1] == 0, pos                                         # an image without positives: the one without ground truth
    assert sum(pos) >= 1 and rec["pos_idx"].numel() == sum(pos), pos                 # at least one positive overall
    assert [len(g) for g in batch["gt_bboxes"]] == [4, 0, 1]
    sizes = [rec[f"rpn_cls{i}"].shape[-1] for i in range(5)]
    assert sizes == [32, 16, 8, 4, 2] and 3 * 32 * 32 > D.TRAIN_CFG["rpn_proposal"]["nms_pre"] >= 3 * 8 * 8       # level 0 selects, 2 - 4 do not


def test_the_kernel_route_ran_the_kernel_layers(chain):
    asm, rec = chain
    from clipself_amd.linear import LinearThin
    assert isinstance(asm.bbox_head.fc_reg, LinearThin) and asm.bbox_head.shared_fcs[0].spatial == (D.C, 49)
    want = {"fpn0": "_BatchNormActFn", "rpn_cls0": "_ThinFn", "rpn_reg4": "_ThinFn", "trunk": "_LinearActFn", "bbox_pred": "_LinearThinFn",
            "mask_pred": "_MaskTailFn"}
    for name, fn in want.items():
        assert rec.fns[name].startswith(fn), (name, rec.fns[name])
    assert not rec["roi_feats"].is_contiguous() or D.C == 1                          # the extractor hands over a permuted view


# ------------------------------------------------------------------------------------------------ (a) - (c), (e)
def test_forward_seams_stage_by_stage(chain, batch, keys):
    asm, rec = chain
    D.check_forward(rec, asm, batch, keys, TAG)


def test_backward_seams_by_replay(chain, ops):
    asm, rec = chain
    D.check_replay(rec, asm, ops, TAG)


def test_loss_terms_against_the_float64_torch_route(chain, batch, keys):
    _, rec = chain
    D.check_scalars(rec, batch, keys, TAG)


def test_ragged_rows_never_reach_a_head_or_a_loss(chain):
    asm, rec = chain
    assert min(rec["counts"].tolist()) < D.TRAIN_CFG["rpn_proposal"]["max_per_img"]  # NaN rows were there to be read
    D.check_ragged(rec, asm, TAG)


def test_a_batch_without_any_positive(ops, keys):
    neg = D.make_batch(1, negatives_only=True)
    asm = D.Assembly(True, ops)
    rec = D.train_step(asm, neg, keys, poison=True)
    assert rec["pos_idx"].numel() == 0 and tuple(rec["mask_feats"].shape) == (0, D.C, 14, 14) and tuple(rec["mask_pred"].shape) == (0, 1, D.MASK, D.MASK)
    D.check_ragged(rec, asm, TAG)
    ref = D.train_step(D.Assembly(False), neg, keys)
    assert float(ref["loss_mask"]) == 0.0 and float(rec["loss_mask"]) == 0.0
    for k, g in rec.param_grads.items():
        if k.startswith("mask_head."):
            assert (g is None) == (ref.param_grads[k] is None), k                     # exactly as on the torch route
    D.check_replay(rec, asm, ops, TAG + ", no positive")                             # the FPN levels: the remaining consumers
    D.check_scalars(rec, neg, keys, TAG + ", no positive")


# ------------------------------------------------------------------------------------------------ (d) state across steps
@pytest.mark.parametrize("how", ["sgd", "adamw_fused", "load_state_dict", "data_clone"])
def test_a_live_assembly_equals_a_fresh_one_after_the_weights_change(ops, batch, keys, how):
    asm = D.Assembly(True, ops)
    first = D.train_step(asm, batch, keys)                                           # warms every cache and workspace
    _changed(asm, how)
    live = D.train_step(asm, batch, keys)
    assert not D.bits_equal(first["fpn0"], live["fpn0"]) and not D.bits_equal(first["bbox_pred"], live["bbox_pred"])
    fresh = D.train_step(D.fresh_like(asm, ops, live.state), batch, keys)
    D.same_records(live, fresh, f"step 2 after {how}: live against fresh assembly")
    if how != "sgd":
        return
    stats = {k: v.clone() for k, v in asm.state_dict().items() if "running_" in k or "num_batches" in k}
    out = D.infer(asm, batch)
    for k, v in asm.state_dict().items():
        if k in stats:
            assert torch.equal(v, stats[k]), f"infer changed {k}"
    other = D.infer(D.fresh_like(asm, ops), batch)
    D.same_records(out, other, "infer: trained live assembly against a fresh one in eval()")
    print(f"DET CHAIN [{TAG}] (d) infer: proposals {out['counts'].tolist()}, detections {out['det_counts'].tolist()}, "
          f"pasted pixels {int(out['pasted'].sum())}")
    assert not asm.training and sum(out["det_counts"].tolist()) > 0


# ------------------------------------------------------------------------------------------------ (f) planted seam errors
def _rejects(fn):
    """-> the message of the AssertionError fn raises, None when it passes."""
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
    except AssertionError as e:
        return str(e) or "AssertionError without a message"
    return None


def _checks(ops, batch, keys, flaw):
    """-> {check letter: the message it rejects the chain with `flaw` planted with, or None}."""
    asm = D.Assembly(True, ops)
    if flaw == "stale_pack":
        D.train_step(asm, batch, keys)
        _changed(asm, "sgd")
        with D.stale_packs():
            rec = D.train_step(asm, batch, keys)
        fresh = D.train_step(D.fresh_like(asm, ops, rec.state), batch, keys)
        return {"d": _rejects(lambda: D.same_records(rec, fresh, "stale_pack: live against fresh assembly"))}
    rec = D.train_step(asm, batch, keys, flaw=flaw, poison=True)
    return {"a": _rejects(lambda: D.check_forward(rec, asm, batch, keys)), "b": _rejects(lambda: D.check_replay(rec, asm, ops)),
            "c": _rejects(lambda: D.check_scalars(rec, batch, keys)), "e": _rejects(lambda: D.check_ragged(rec, asm))}


@pytest.mark.parametrize("flaw", D.FLAWS)
def test_every_planted_seam_error_is_rejected(ops, batch, keys, flaw):
    got = _checks(ops, batch, keys, flaw)
    letter, stage = REJECTED_BY[flaw]
    for k, msg in got.items():
        print(f"DET CHAIN [{TAG}] (f) {flaw}: ({k}) {'passes' if msg is None else 'rejects: ' + msg[:110]}")
    assert got[letter] is not None, f"check ({letter}) accepts the planted seam error {flaw!r}: {got}"
    assert stage in got[letter], f"check ({letter}) rejects {flaw!r} at another stage than {stage!r}: {got[letter]}"


def test_the_clean_chain_is_not_rejected_by_the_flaw_harness(ops, batch, keys):
    got = _checks(ops, batch, keys, None)
    assert all(v is None for v in got.values()), got
