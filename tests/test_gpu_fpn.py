"""`-m gpu`: the detector's feature pyramid on the MI355X.

Kernels alone (HipOps.upsample2x_add / pool2x, forms 7 / 8 of cs_transpose_bf16): bit for bit against the np.float32 restatement of the
header's text (tests/_fpn_ref.RefOpsFPN) for all four type pairs, both accumulate settings and two row strides; form 7 with equal types
also against torch's own fine + F.interpolate(coarse); the adjoint identity on integer maps; inside the poisoned halos of
tests/_extents.py; the header's rejections.  Conv1x1 and the module (fpn.FPN on HipOps): exact operands bit for bit against float64
autograd, random operands inside the derived bounds (Conv1x1) and the recorded thresholds (the module with norm, profiles/fpn_parity.md)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from _fpn_ref import (BF, CONV1X1_SHAPES, EXACT_GEOMS, F32, LAYOUTS, PARITY_GRAD_REL_L2, PARITY_OUT_REL_L2, RefOpsFPN, check_conv1x1,  # noqa: E402
                      check_exact, parity, random_case, run_module)

# The grid cap of forms 7 / 8: 8 workgroups of 256 threads per compute unit (include/clipself_hip.h); one thread per channel group of a
# coarse pixel.  The wrap test's shape has one grid row of 1024 pixels more than that many 8-channel groups, so the grid-stride loop
# goes round again.
BLOCKS_PER_CU, THREADS = 8, 256
# (B, h, w, C): smallest | h != w both ways | a full wave of groups | several images, an odd channel-group count | vector width 4 but
# not 8 | one element per lane
SHAPES = [(1, 1, 1, 8), (2, 3, 5, 24), (3, 5, 3, 40), (1, 8, 8, 256), (2, 7, 16, 264), (1, 4, 4, 12), (2, 2, 3, 5)]
TYPE_PAIRS = [(F32, F32), (F32, BF), (BF, F32), (BF, BF)]            # (coarse, fine)
_INT = {BF: torch.int16, F32: torch.int32}
NAN_BITS = {BF: 0x7FA5, F32: 0x7FA5A5A5}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOpsFPN()


def _same_bits(got, want, what):
    it = _INT[got.dtype]
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.cpu().contiguous().view(it), want.contiguous().view(it)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


@functools.lru_cache(maxsize=None)
def _maps(B, h, w, C):
    """Seeded fp32 (coarse [B*h*w, C + 8], fine [4*B*h*w, C + 8]) whose values bf16 holds exactly; built on the device (the large shape),
    kept on the host, shared read-only."""
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + h * 100 + w * 10 + C)
    mk = lambda rows: torch.randn(rows, C + 8, generator=g, device="cuda").to(BF).to(F32).cpu()
    return mk(B * h * w), mk(4 * B * h * w)


def _place(data, C, ld, dtype, fill=None):
    """A [rows, C] view with row stride ld holding data[:, :C] as dtype (or NaN-filled); the padding columns hold NaN."""
    buf = torch.full((data.shape[0], ld), NAN_BITS[dtype], dtype=_INT[dtype]).view(dtype)
    if fill is None:
        buf[:, :C] = data[:, :C].to(dtype)
    return buf


def _check_forms(hip, ref, B, h, w, C, ct, ft):
    coarse0, fine0 = _maps(B, h, w, C)
    for ld in (C, C + 8):
        for acc in (False, True):
            # form 7: out = fine (NaN-filled on the overwrite form)
            c_host, f_host = _place(coarse0, C, ld, ct), _place(fine0, C, ld, ft, fill=None if acc else "nan")
            want = f_host.clone()
            ref.upsample2x_add(c_host[:, :C], want[:, :C], B, h, w, C, accumulate=acc)
            runs = []
            for _ in range(2):
                c_dev, f_dev = c_host.cuda(), f_host.cuda()
                hip.upsample2x_add(c_dev[:, :C], f_dev[:, :C], B, h, w, C, accumulate=acc)
                _same_bits(f_dev, want, f"form 7 {ct}->{ft} ld={ld} acc={acc}")              # the NaN padding columns included
                runs.append(f_dev)
            assert torch.equal(runs[0].view(_INT[ft]), runs[1].view(_INT[ft]))
            if acc and ct == ft:                                                            # torch's own expression, same types
                cm = c_host[:, :C].contiguous().cuda().view(B, h, w, C).permute(0, 3, 1, 2)
                fm = f_host[:, :C].contiguous().cuda().view(B, 2 * h, 2 * w, C).permute(0, 3, 1, 2)
                t = fm + F.interpolate(cm, scale_factor=2, mode="nearest")
                _same_bits(runs[0][:, :C].contiguous(), t.permute(0, 2, 3, 1).reshape(-1, C).cpu(), f"form 7 against torch {ct} ld={ld}")
            # form 8: out = coarse
            f_host, c_host = _place(fine0, C, ld, ft), _place(coarse0, C, ld, ct, fill=None if acc else "nan")
            want = c_host.clone()
            ref.pool2x(f_host[:, :C], want[:, :C], B, h, w, C, accumulate=acc)
            runs = []
            for _ in range(2):
                f_dev, c_dev = f_host.cuda(), c_host.cuda()
                hip.pool2x(f_dev[:, :C], c_dev[:, :C], B, h, w, C, accumulate=acc)
                _same_bits(c_dev, want, f"form 8 {ft}->{ct} ld={ld} acc={acc}")
                runs.append(c_dev)
            assert torch.equal(runs[0].view(_INT[ct]), runs[1].view(_INT[ct]))


# ------------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("ct,ft", TYPE_PAIRS)
@pytest.mark.parametrize("B,h,w,C", SHAPES)
def test_forms_7_and_8_are_the_headers_text_bit_for_bit(hip, ref, B, h, w, C, ct, ft):
    assert hip.FPN_TOPDOWN
    _check_forms(hip, ref, B, h, w, C, ct, ft)


@pytest.mark.parametrize("ct,ft", TYPE_PAIRS)
def test_the_grid_stride_loop_wraps_past_the_cap(hip, ref, ct, ft):
    cap_items = BLOCKS_PER_CU * hip.num_cus * THREADS
    h, w, C = cap_items // 1024 + 1, 1024, 8                             # 8 channels: one group (bf16 pair) or two per pixel
    assert h * w > cap_items
    _check_forms(hip, ref, 1, h, w, C, ct, ft)


@pytest.mark.parametrize("B,h,w,C", [(2, 3, 5, 24), (1, 4, 4, 12), (2, 2, 3, 5)])
def test_adjoint_identity_on_integer_maps(hip, B, h, w, C):
    g = torch.Generator().manual_seed(h * w + C)
    x = torch.randint(-8, 9, (B * h * w, C), generator=g).to(F32)
    y = torch.randint(-8, 9, (4 * B * h * w, C), generator=g).to(F32)
    up = torch.full_like(y, float("nan")).cuda()
    hip.upsample2x_add(x.cuda(), up, B, h, w, C, accumulate=False)
    pool = torch.full_like(x, float("nan")).cuda()
    hip.pool2x(y.cuda(), pool, B, h, w, C, accumulate=False)
    lhs, rhs = (up.cpu().double() * y.double()).sum(), (x.double() * pool.cpu().double()).sum()
    assert float(lhs) == float(rhs) and float(lhs) != 0.0                # <up(x), y> == <x, pool(y)>, exactly


def _halo_case(B, h, w, C, ct, ft, pool, acc):
    def fn(ops, a):
        coarse0, fine0 = _maps(B, h, w, C)
        if pool:
            fine = a.inp(fine0[:, :C].to(ft), a.ld(C))
            coarse = a.out((B * h * w, C), ct, ld=a.ld(C), init=coarse0[:, :C].to(ct) if acc else None)
            ops.pool2x(fine, coarse, B, h, w, C, accumulate=acc)
            return {"coarse": coarse}
        coarse = a.inp(coarse0[:, :C].to(ct), a.ld(C))
        fine = a.out((4 * B * h * w, C), ft, ld=a.ld(C), init=fine0[:, :C].to(ft) if acc else None)
        ops.upsample2x_add(coarse, fine, B, h, w, C, accumulate=acc)
        return {"fine": fine}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("B,h,w,C", SHAPES)
def test_kernels_stay_inside_their_extents(hip, B, h, w, C, pad):
    for ct, ft in TYPE_PAIRS:
        for pool in (False, True):
            for acc in (False, True):
                key = f"{'pool2x' if pool else 'upsample2x_add'}[{B},{h},{w},{C},{ct},{ft},{acc}]"
                problems = run_case(hip, _halo_case(B, h, w, C, ct, ft, pool, acc), "cuda", pad, key=key)
                assert not problems, f"{key} (row strides + {pad}):\n  " + "\n  ".join(problems)


def test_entry_point_refuses_what_the_header_lists(hip):
    B, h, w, C = 2, 2, 3, 8
    coarse = torch.ones(B * h * w, C, device="cuda")
    fine = torch.ones(4 * B * h * w, C, device="cuda")
    p = lambda t: t.data_ptr()
    good = 7 | 1 << 8 | 1 << 9 | w << 12

    def call(form=good, ldc=C, ldf=C, R=h * w, Cc=C, batch=B, pool=False):
        a, b = (fine, coarse) if pool else (coarse, fine)
        lda, ldb = (ldf, ldc) if pool else (ldc, ldf)
        return hip.lib.cs_transpose_bf16(p(a), lda, p(b), ldb, R, Cc, form, batch, None)

    def refused(**kw):
        rc = call(**kw)
        msg = hip.lib.cs_last_error()
        return rc == -1 and b"FPN top-down" in msg

    assert refused(form=7 | 1 << 8 | 1 << 9)                                        # w = 0
    assert refused(R=h * w + 1)                                                     # R is no multiple of w
    assert refused(ldc=C - 1) and refused(ldf=C - 1)                                # a row stride below C
    assert refused(form=8 | 1 << 8 | w << 12, ldc=C - 1, pool=True) and refused(form=8 | 1 << 8 | w << 12, ldf=C - 1, pool=True)
    assert refused(form=7 | 1 << 9 | w << 12) and refused(form=8 | w << 12, pool=True)      # bit 8 clear: no factor but 2
    assert refused(form=7 | 1 << 8 | 256 << 12, R=1 << 16, batch=1 << 15)           # batch * R * C past 2^31 - 1
    assert refused(Cc=0) and refused(batch=0) and refused(R=0)
    torch.cuda.synchronize()
    assert float(fine.min()) == 1.0 and float(coarse.min()) == 1.0                  # nothing was launched
    assert call() == 0                                                              # and the next valid call succeeds
    torch.cuda.synchronize()
    assert float(fine.min()) == 2.0 and float(fine.max()) == 2.0
    with pytest.raises(AssertionError):
        hip.upsample2x_add(coarse, fine[:-1], B, h, w, C)
    with pytest.raises(AssertionError):
        hip.pool2x(fine.t(), coarse, B, h, w, C)


# ------------------------------------------------------------------------------------------------ Conv1x1
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
@pytest.mark.parametrize("shape", list(CONV1X1_SHAPES))
def test_conv1x1_against_float64_autograd(hip, shape, layout, dtype, kind):
    check_conv1x1(hip, shape, layout, dtype, kind, device="cuda")


# ------------------------------------------------------------------------------------------------ the module
def _fpn(hip, **extra):
    from clipself_amd.fpn import FPN
    return lambda *a, **k: FPN(*a, ops=hip, fused=True, **k, **extra)


@pytest.mark.parametrize("name", list(EXACT_GEOMS))
def test_module_exact_operands_bit_for_bit(hip, name):
    check_exact(_fpn(hip), name, device="cuda")


def test_module_random_operands_within_the_recorded_thresholds(hip):
    """Measured on the MI355X: outputs and input gradients 2.6371e-3, parameter gradients 2.8333e-3 (profiles/fpn_parity.md)."""
    worst_out, worst_grad = parity(_fpn(hip), device="cuda", tag="MI355X")
    assert worst_out <= PARITY_OUT_REL_L2, (worst_out, PARITY_OUT_REL_L2)
    assert worst_grad <= PARITY_GRAD_REL_L2, (worst_grad, PARITY_GRAD_REL_L2)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_module_repeats_its_bits_and_keeps_layout_and_dtype(hip, dtype):
    state, xs, gs, *_ = random_case()
    m = _fpn(hip)([64] * 4, 64, 5, norm_cfg=dict(type="BN")).train()
    m.load_state_dict(state, strict=True)
    m = m.cuda()
    first = run_module(m, xs, gs, dtype=dtype, device="cuda", channels_last=dtype == BF)
    m.load_state_dict(state, strict=True)                                # the running statistics back to where they were
    again = run_module(m, xs, gs, dtype=dtype, device="cuda", channels_last=dtype == BF)
    for o in first[0]:
        assert o.dtype == dtype and o.is_cuda and o.permute(0, 2, 3, 1).is_contiguous()
    assert [tuple(o.shape[2:]) for o in first[0]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert all(d.dtype == dtype for d in first[1])
    for a, b in zip(first[0] + first[1] + list(first[2].values()), again[0] + again[1] + list(again[2].values())):
        assert torch.equal(a, b)                                         # the same inputs, the same bits


def test_backbone_shaped_input_flows_through(hip):
    """What EvaCLIPViT returns: four NCHW fp32 maps and a trailing entry (None in training) that the detector slices off with [:-1]."""
    from clipself_amd.fpn import FPN
    torch.manual_seed(11)
    m = FPN([128] * 4, 64, 5, norm_cfg=dict(type="SyncBN", requires_grad=True), ops=hip).cuda().train()
    feats = tuple(torch.randn(2, 128, s, s, device="cuda", requires_grad=s >= 12) for s in (24, 12, 6, 3)) + (None,)
    outs = m(feats[:-1])
    assert [tuple(o.shape) for o in outs] == [(2, 64, 24, 24), (2, 64, 12, 12), (2, 64, 6, 6), (2, 64, 3, 3), (2, 64, 2, 2)]
    assert all(o.dtype == F32 and o.is_cuda for o in outs)
    sum(o.square().mean() for o in outs).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0 for p in m.parameters())
    assert feats[0].grad is not None and feats[1].grad is not None and feats[2].grad is None
