"""`-m gpu`: Linear (+ ReLU) as split-K GEMMs (the cs_gemm_nt block of include/clipself_hip.h, clipself_amd/linear.py,
clipself_amd/bbox_head.py) on the MI355X.

The kernels alone (HipOps.gemm_nt with epilogues 0 and 9, splits in {1, 2, 3, 5, automatic}): outputs and workspaces are handed in as
NaN, every call runs twice with equal bits.  Exact operands: bit for bit against float64 at every slice count.  Random operands: inside
the derived per-element bounds of tests/_fc_ref.py, the worst error / bound printed (profiles/fc_parity.md).  A slice count above K / 64
is a rejection, so the small shapes check that instead.  ReLU edge values, the header's rejections, a padded ldc and an exactly sized
workspace inside the poisoned halos of tests/_extents.py, the layer under autograd and the head beside its torch-FC twin."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from _fc_ref import BF, F32, bound, bounds, case, check_bound, layer, reference, rne_bf16, run_layer, same_bits  # noqa: E402
from clipself_amd.bbox_head import ConvFCBBoxHead  # noqa: E402
from clipself_amd.linear import LinearAct  # noqa: E402

# (M, N, K): one row, one K tile | two K tiles | two M tiles of 128, five K tiles | past one 256-row tile, N no multiple of 64, seven K
# tiles | the flatten form with C = 64, P = 49: several tiles in M and N, 49 K tiles
SHAPES = [(1, 8, 64), (3, 8, 128), (130, 16, 320), (257, 72, 448), (300, 512, 3136)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
SPLITS = [1, 2, 3, 5, 0]                                    # 0 = chosen by the library
ACT = {0: None, 9: "relu"}


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(it), b.view(it)), "two runs on equal inputs differ"
    return a


def _gemm(hip, X, W, bias, epi, splits, M, N):
    """One call into a NaN-filled C with a NaN-filled workspace of exactly splits * M * N floats (none where one slice runs)."""
    n = splits if splits > 0 else hip.gemm_nt_splits(M, N, X.shape[1])
    C = _nan((M, N), BF)
    hip.gemm_nt(X, W, C, bias, extra=_nan((n * M * N,), F32) if n > 1 else None, epi=epi, splits=splits)
    return C


@pytest.mark.parametrize("epi", [0, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_kernels_exact_bit_for_bit_and_random_within_the_bounds(hip, shape, epi):
    assert hip.LINEAR_ACT
    M, N, K = shape
    for kind in ("exact", "random"):
        x, w, b, dy, ref = case((M, K, N), kind, ACT[epi])
        X, W, bias = x.to(BF).cuda(), w.to(BF).cuda(), b.cuda()
        for splits in SPLITS:
            n = splits if splits > 0 else hip.gemm_nt_splits(M, N, K)
            if n > K // 64:                                  # the header: splits > K / 64 is an error, nothing is written
                C = _nan((M, N), BF)
                with pytest.raises(RuntimeError, match="exceeds"):
                    hip.gemm_nt(X, W, C, bias, extra=_nan((n * M * N,), F32), epi=epi, splits=splits)
                torch.cuda.synchronize()
                assert bool(C.isnan().all())
                continue
            C = _twice(lambda: _gemm(hip, X, W, bias, epi, splits, M, N))
            if kind == "exact":
                same_bits(C, rne_bf16(ref["y"]), f"epi {epi} splits {splits}")
            else:
                check_bound(f"FC PARITY gemm {SHAPE_IDS[SHAPES.index(shape)]} epi{epi} splits={splits or 'auto'}({n}) y", C, ref["y"],
                            bound(ref["ay"], K, n, ref["y"], True))


def test_automatic_splits_are_the_headers_rule(hip):
    from _fc_ref import auto_splits
    for M, N, K in SHAPES + [(4096, 512, 12544), (8000, 512, 12544), (4096, 512, 512), (4096, 768, 12544)]:
        assert hip.gemm_nt_splits(M, N, K) == auto_splits(M, N, K, hip.num_cus)


@pytest.mark.parametrize("splits", [1, 2])
def test_relu_edge_values(hip, splits):
    """Pre-activations of exactly +0 (3 - 3), -0 (a bias of -0 on a zero sum: +0 + -0 = +0 in fp32 as in float64), negative integers and
    NaN, placed through an integer bias: bit for bit what F.relu gives on the float64 pre-activation."""
    A = torch.zeros(5, 128, dtype=BF)
    A[:4, 0] = 1.0                                           # row 4 stays zero: its sums are +0
    W = torch.zeros(8, 128, dtype=BF)
    W[:, 0] = 3.0
    bias = torch.tensor([-3.0, -0.0, -5.0, float("nan"), 2.0, 0.0, -4.0, -3.0])
    pre = A.double() @ W.double().T + bias.double()
    want = torch.relu(pre).to(BF)
    C = _nan((5, 8), BF)
    hip.gemm_nt(A.cuda(), W.cuda(), C, bias.cuda(), extra=_nan((splits * 5 * 8,), F32) if splits > 1 else None, epi=9, splits=splits)
    got = C.cpu()
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert torch.equal(got[:, keep].contiguous().view(torch.int16), want[:, keep].contiguous().view(torch.int16))
    assert bool(got[:, 3].isnan().all())                     # a NaN passes, as through torch's ReLU


def test_rejections(hip):
    M, N, K = 3, 8, 128
    X, W = torch.ones(M, K, dtype=BF, device="cuda"), torch.ones(N, K, dtype=BF, device="cuda")
    ws = _nan((3 * M * N + 4,), F32)
    for kw, msg in ((dict(epi=9, splits=3, extra=ws), "exceeds"),                       # K / 64 = 2
                    (dict(epi=0, splits=3, extra=ws), "exceeds"),
                    (dict(epi=9, splits=2, extra=None), "workspace"),
                    (dict(epi=0, splits=2, extra=ws[1:]), "workspace"),                  # 4 bytes off a 16-byte boundary
                    (dict(epi=7, splits=2, extra=ws), "split-K")):
        C = _nan((M, N), BF)
        with pytest.raises(RuntimeError, match=msg):
            hip.gemm_nt(X, W, C, None, **kw)
        torch.cuda.synchronize()
        assert bool(C.isnan().all()), kw
    C1 = _nan((M, N), F32)
    with pytest.raises(RuntimeError, match="split-K"):
        hip.gemm_nt(X, W, C1, None, extra=ws, epi=1, splits=2)
    torch.cuda.synchronize()
    assert bool(C1.isnan().all())
    with pytest.raises(ValueError, match="workspace"):                                   # the wrapper's own check of the size
        hip.gemm_nt(X, W, _nan((M, N), BF), None, extra=ws[:2 * M * N - 4], epi=9, splits=2)


# ------------------------------------------------------------------------------------------------ extents
def _extent_case(M, N, K, epi):
    def fn(ops, a):
        g = torch.Generator().manual_seed(M + N + K)
        A = a.inp((torch.randn(M, K, generator=g)).to(BF), a.ld(K, 8))
        B = a.inp((torch.randn(N, K, generator=g) * K ** -0.5).to(BF), a.ld(K, 8))
        bias = a.inp(torch.randn(N, generator=g))
        outs = {}
        for splits in SPLITS:
            n = splits if splits > 0 else ops.gemm_nt_splits(M, N, K)
            if n > K // 64:
                continue
            C = a.out((M, N), BF, a.ld(N, 4))                # a padded ldc in the halo run; the padding is sentinel and must stay
            ws = a.ws(n * M * N * 4).view(F32) if n > 1 else None         # exactly splits * M * N floats
            ops.gemm_nt(A, B, C, bias, extra=ws, epi=epi, splits=splits)
            outs[f"C[splits={splits}]"] = C
        return outs
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("epi", [0, 9])
@pytest.mark.parametrize("shape", SHAPES[2:], ids=SHAPE_IDS[2:])
def test_padded_ldc_and_exact_workspace_inside_poisoned_halos(hip, shape, epi, pad):
    problems = run_case(hip, _extent_case(*shape, epi), "cuda", pad, key=f"fc.gemm_nt.epi{epi}{list(shape)}")
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------ the layer under autograd
LAYER_CASES = [((130, 320, 16), None), ((300, 3136, 512), (64, 7, 7))]
LAYER_IDS = ["130x320x16", "300x(64x7x7)x512"]


@pytest.mark.parametrize("shape,geom", LAYER_CASES, ids=LAYER_IDS)
def test_layer_under_autograd(hip, shape, geom):
    spatial = None if geom is None else (geom[0], geom[1] * geom[2])
    for kind in ("exact", "random"):
        x, w, b, dy, ref0 = case(shape, kind)
        m = layer(hip, w, b, device="cuda", fused=True, act="relu", spatial=spatial)
        for dtype in (F32, BF):
            y, dx, dw, db = (t.cpu() for t in run_layer(m, x, dy, dtype, geom))
            y2, dx2, dw2, db2 = (t.cpu() for t in run_layer(m, x, dy, dtype, geom))
            for u, v, k in ((y, y2, "y"), (dx, dx2, "dx"), (dw, dw2, "dw"), (db, db2, "db")):
                same_bits(u, v, f"{k}: two runs on equal inputs")
            if kind == "exact":
                same_bits(y, rne_bf16(ref0["y"]).to(dtype), "y")
                same_bits(dx, ref0["dx"].to(F32) if dtype == F32 else rne_bf16(ref0["dx"]), "dx")
                same_bits(dw, ref0["dw"].to(F32), "dw")
                same_bits(db, ref0["db"].to(F32), "db")
            else:
                ref = reference(x, w, b, dy, mask=y > 0)         # the device's own saved Y: the mask is unambiguous
                tol = bounds(ref, shape, splits=8, bf16_dx=dtype == BF)
                for k, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
                    check_bound(f"FC PARITY layer {LAYER_IDS[LAYER_CASES.index((shape, geom))]} {str(dtype)[6:]} {k}", got, ref[k], tol[k])


def test_layer_outside_the_coverage_and_forced_splits(hip):
    x, w, b, dy, ref = case((300, 3136, 512), "exact")
    for splits in (1, 3):
        m = layer(hip, w, b, device="cuda", fused=True, act="relu", spatial=(64, 49), splits=splits)
        y = run_layer(m, x, dy, BF, (64, 7, 7))[0].cpu()
        same_bits(y, rne_bf16(ref["y"]), f"splits={splits}")
    reg = LinearAct(512, 4, ops=hip).cuda()                               # fc_reg's shape: torch
    assert reg.kernel_backend(torch.zeros(3, 512, device="cuda")) is None
    with pytest.raises(NotImplementedError):
        LinearAct(512, 4, ops=hip, fused=True).cuda()(torch.zeros(3, 512, device="cuda"))


# ------------------------------------------------------------------------------------------------ the head
def test_head_beside_its_torch_fc_twin(hip):
    """ConvFCBBoxHead(num_shared_convs=1, in_channels=64, fc_out_channels=64) on 6 RoIs beside the same head whose FCs run on torch
    (fused=False): equal bits out of the convolution, and every FC of the kernel head inside its bounds on the input and the gradient
    that reached it.  The reference reads what the kernels read: the input, the weights and the incoming gradient rounded to bf16."""
    cfg = dict(num_shared_convs=1, in_channels=64, fc_out_channels=64, num_shared_fcs=2, num_cls_fcs=1, num_reg_fcs=1, num_classes=5,
               reg_class_agnostic=True, norm_cfg=dict(type="SyncBN"))
    torch.manual_seed(7)
    head = ConvFCBBoxHead(ops=hip, fused=True, **cfg).cuda()
    twin = ConvFCBBoxHead(ops=hip, fused=True, **cfg).cuda()
    twin.load_state_dict(head.state_dict(), strict=True)
    fcs = lambda h: list(h.shared_fcs) + list(h.cls_fcs) + list(h.reg_fcs)
    for m in fcs(twin):
        m.fused = False
    x = torch.randn(6, 64, 7, 7, generator=torch.Generator().manual_seed(8)).cuda()
    seen = {}

    def watch(h, tag):
        h.shared_convs[-1].register_forward_hook(lambda m, i, o: seen.__setitem__((tag, "conv"), o.detach().clone()))
        for j, m in enumerate(fcs(h)):
            m.register_forward_hook(lambda m, i, o, j=j: seen.__setitem__((tag, j, "io"), (i[0].detach().clone(), o.detach().clone())))
            m.register_full_backward_hook(lambda m, gi, go, j=j: seen.__setitem__((tag, j, "g"), (gi[0].detach().clone(), go[0].detach().clone())))
    watch(head, "k")
    watch(twin, "t")
    outs = {}
    for h, tag in ((head, "k"), (twin, "t")):
        xi = x.clone().requires_grad_(True)
        x_cls, bbox_pred = h(xi)
        (x_cls.square().sum() + bbox_pred.sum() * 100).backward()
        outs[tag] = (x_cls.detach(), bbox_pred.detach())
    torch.cuda.synchronize()
    same_bits(seen["k", "conv"], seen["t", "conv"].cpu(), "the convolution's output")
    assert outs["k"][0].shape == (6, 64) and outs["k"][1].shape == (6, 4)
    for j, m in enumerate(fcs(head)):
        assert type(m).__name__ == "LinearAct" and m.act == "relu"
        xin, y = (t.cpu() for t in seen["k", j, "io"])
        dx, dy = (t.cpu() for t in seen["k", j, "g"])
        rows = xin.shape[0]
        x2 = xin.flatten(1).to(BF).to(F32)                   # flatten(1) of the map: nn.Linear's (c, p) order
        w2, dy2 = m.weight.detach().cpu().to(BF).to(F32), dy.to(BF).to(F32)
        ref = reference(x2, w2, m.bias.detach().cpu(), dy2, mask=y > 0)
        shape = (rows, m.in_features, m.out_features)
        tol = bounds(ref, shape, splits=8)
        got = dict(y=y, dx=dx.reshape(rows, -1), dw=m.weight.grad.cpu(), db=m.bias.grad.cpu())
        for k in ("y", "dx", "dw", "db"):
            check_bound(f"FC PARITY head fc{j} {shape[1]}->{shape[2]} {k}", got[k], ref[k], tol[k])
    # the two heads agree to the bf16 pipeline's rounding: four FC layers of 2^-8 each on activations and weights
    for a, b in zip(outs["k"], outs["t"]):
        assert float((a - b).abs().max()) <= 8 * 2.0 ** -8 * float(b.abs().max())
