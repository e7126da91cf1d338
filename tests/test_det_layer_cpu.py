"""CPU: clipself_amd/det_layer.py, what the kernel-backed detector layers state once -- the dispatch rule over its whole
truth table on a stub host backend, the packed-operand cache and its key, and the rows helpers (padding, chunking, channel-last views)."""
import itertools
import sys
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from clipself_amd import det_layer as D
from clipself_amd.det_layer import BF16, CHUNK_BYTES, F32, KernelLayer

DEFAULT = True                                 # the stand-in for a module's FUSED_*_DEFAULT: read when kernel_backend runs


class Host:
    """A host backend as the dispatch sees it: `empty`, `zeros` and (when built with one) the flag."""
    name = "host"

    def __init__(self, flag=True):
        self.n_empty = 0
        if flag:
            self.STUB = True

    def empty(self, shape, dtype):
        self.n_empty += 1
        return torch.empty(shape, dtype=dtype)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)


class Layer(KernelLayer):
    FLAG, COVERAGE = "STUB", "an even width"

    def __init__(self, ops, fused):
        self.ops, self.fused = ops, fused

    def fused_default(self):
        return DEFAULT

    def covered(self, x):
        return x.shape[-1] % 2 == 0

    def describe(self):
        return "Layer(stub)"


# ------------------------------------------------------------------------------------------------ dispatch
def expected(fused, default, backend, covered):
    """The route on a CPU tensor: "ops", None (torch) or the exception; the refusals in the order fused=False, device, flag, coverage."""
    if fused is False:
        return None
    if backend != "flag":                      # no backend, or one without the flag: a CPU tensor has no kernels
        return NotImplementedError if fused else None
    if not (fused or default):
        return None
    if not covered:
        return NotImplementedError if fused else None
    return "ops"


@pytest.mark.parametrize("fused,default,backend,covered", list(itertools.product((False, None, True), (False, True), ("none", "flag", "noflag"),
                                                                                 (True, False))))
def test_dispatch_truth_table(monkeypatch, fused, default, backend, covered):
    monkeypatch.setattr(sys.modules[__name__], "DEFAULT", default)
    ops = None if backend == "none" else Host(flag=backend == "flag")
    layer, x = Layer(ops, fused), torch.zeros(3, 4 if covered else 5)
    # the mixin, then the function form: the same rule without the coverage clause
    for route, want in ((lambda: layer.kernel_backend(x), expected(fused, default, backend, covered)),
                        (lambda: D.layer_ops(x, "STUB", ops, fused, default), expected(fused, default, backend, True))):
        if want is NotImplementedError:
            with pytest.raises(NotImplementedError):
                route()
        else:
            assert route() is (ops if want == "ops" else None)


def test_refusals_name_their_reason_in_order():
    x = torch.zeros(3, 5)                                                        # a CPU tensor outside the coverage
    with pytest.raises(NotImplementedError, match="needs CUDA tensors"):
        Layer(None, True).kernel_backend(x)
    with pytest.raises(NotImplementedError, match="needs CUDA tensors"):         # the device is refused before the missing flag
        Layer(Host(flag=False), True).kernel_backend(x)
    with pytest.raises(NotImplementedError, match=r"fused=True: Layer\(stub\) on torch.float32 \(3, 5\) is outside the kernels' coverage "
                                                  r"\(an even width\)"):
        Layer(Host(), True).kernel_backend(x)
    on_gpu = SimpleNamespace(is_cuda=True, device=torch.device("cuda"), shape=(3, 5))          # what the rule reads of a device tensor
    with pytest.raises(NotImplementedError, match="backend 'host' has no STUB kernels"):      # the flag is refused before the coverage
        Layer(Host(flag=False), True).kernel_backend(on_gpu)
    assert Layer(Host(flag=False), None).kernel_backend(on_gpu) is None
    assert Layer(Host(), False).kernel_backend(on_gpu) is None


def test_the_device_probe_allocates_once_per_backend():
    a, b, bare = Host(), Host(), Host(flag=False)
    x = torch.zeros(2, 4)
    for _ in range(3):
        for ops in (a, b, bare):
            Layer(ops, None).kernel_backend(x)
            Layer(ops, False).kernel_backend(x)
        assert D.backend_device(a) == torch.device("cpu")
    assert (a.n_empty, b.n_empty, bare.n_empty) == (1, 1, 0)                      # a backend without the flag is never asked


def test_conv_coverage_takes_the_output_multiple():
    conv, x = nn.Conv2d(64, 4, 1), torch.zeros(1, 64, 2, 2)
    assert D.conv_covered(conv, x) and not D.conv_covered(conv, x, 8) and D.conv_covered(nn.Conv2d(64, 16, 1), x, 8)
    assert not D.conv_covered(nn.Conv2d(32, 8, 1), torch.zeros(1, 32, 2, 2)) and not D.conv_covered(conv, x.double())
    assert not D.conv_covered(conv, x[0]) and not D.conv_covered(conv, x[:0]) and not D.conv_covered(conv.double(), x)


# ------------------------------------------------------------------------------------------------ the cache
def _packer(mod):
    calls = []

    def build():
        calls.append(1)
        assert not torch.is_grad_enabled()
        return mod.weight.detach().to(BF16), None if mod.bias is None else mod.bias.detach().clone()
    return calls, build


def test_packed_returns_the_cached_tuple_until_a_parameter_moves():
    mod = nn.Linear(4, 3)
    calls, build = _packer(mod)
    first = D.packed(mod, build)
    assert D.packed(mod, build) is first and len(calls) == 1
    assert "_wcache" in mod.__dict__ and not any("_wcache" in k for k in list(mod.state_dict()) + [n for n, _ in mod.named_parameters()])
    with torch.no_grad():
        mod.weight.mul_(2.0)
    second = D.packed(mod, build)
    assert second is not first and len(calls) == 2 and torch.equal(second[0], mod.weight.detach().to(BF16))
    with torch.no_grad():
        mod.bias.add_(1.0)
    third = D.packed(mod, build)
    assert third is not second and len(calls) == 3 and torch.equal(third[1], mod.bias.detach())
    mod.to(torch.float64).to(torch.float32)                                      # the storage is replaced, the version starts again
    assert D.packed(mod, build) is not third and len(calls) == 4
    mod.weight.data = mod.weight.data.clone()
    assert len(calls) == 4 and D.packed(mod, build) is D.packed(mod, build) and len(calls) == 5


@pytest.mark.parametrize("opt", ["adamw", "adam", "sgd"])
def test_packed_is_rebuilt_after_a_fused_optimizer_step(opt):
    """torch's fused optimizers write the parameters through one multi-tensor kernel: the values change, the version counters and the
    storages do not, so params_key cannot see the step (found by the chain test, tests/test_gpu_det_chain.py (d), where a live assembly
    went on computing with the operands packed before AdamW(fused=True).step()).  packed keys on the steps of the optimizers that own
    the module's parameters as well; a module no optimizer owns keeps its operands."""
    mod, frozen = nn.Linear(4, 3), nn.Linear(4, 3)
    calls, build = _packer(mod)
    fcalls, fbuild = _packer(frozen)
    first, ffirst = D.packed(mod, build), D.packed(frozen, fbuild)
    for p in mod.parameters():
        p.grad = torch.ones_like(p)
    make = {"adamw": torch.optim.AdamW, "adam": torch.optim.Adam, "sgd": torch.optim.SGD}[opt]
    before, key = mod.weight.detach().clone(), D.params_key(mod.weight, mod.bias)
    make(mod.parameters(), lr=0.25, fused=True).step()
    assert not torch.equal(before, mod.weight.detach()) and D.param_steps(mod.weight) == 1 and D.param_steps(mod.bias) == 1
    assert D.param_steps(frozen.weight) == 0 and D.param_steps(None) == 0
    second = D.packed(mod, build)
    assert second is not first and len(calls) == 2
    assert torch.equal(second[0], mod.weight.detach().to(BF16)) and torch.equal(second[1], mod.bias.detach())
    assert D.packed(mod, build) is second and len(calls) == 2                     # no step since: the cached tuple
    assert D.packed(frozen, fbuild) is ffirst and len(fcalls) == 1                # another module's optimizer repacks nothing here
    other = D.packed(mod, build, key=("pair", *D.params_key(mod.weight, mod.bias)), slot="_pair")
    make(mod.parameters(), lr=0.25, fused=True).step()
    assert D.packed(mod, build, key=("pair", *D.params_key(mod.weight, mod.bias)), slot="_pair") is not other      # a caller's own key too


def test_thin_heads_repack_after_a_fused_optimizer_step_of_either_module():
    """conv._thin_packed keys one cache on two modules: a fused step of the second module alone must rebuild it."""
    from clipself_amd import conv
    a, b = conv.Conv1x1Thin(64, 3), conv.Conv1x1Thin(64, 12)
    first = conv._thin_packed((a, b))
    assert conv._thin_packed((a, b)) is first
    for p in b.parameters():
        p.grad = torch.ones_like(p)
    torch.optim.AdamW(b.parameters(), lr=0.25, fused=True).step()
    second = conv._thin_packed((a, b))
    assert second is not first and torch.equal(second[0][3:].float(), b.weight.detach().view(12, 64).to(BF16).float())


def test_packed_without_a_bias_and_with_its_own_key_and_slot():
    mod = nn.Linear(4, 3, bias=False)
    calls, build = _packer(mod)
    assert D.packed(mod, build)[1] is None and D.packed(mod, build)[1] is None and len(calls) == 1
    assert D.params_key(mod.weight, None)[3] is None
    other = D.packed(mod, build, key=("pair", *D.params_key(mod.weight, None)), slot="_pair")
    assert len(calls) == 2 and D.packed(mod, build, key=("pair", *D.params_key(mod.weight, None)), slot="_pair") is other
    assert D.packed(mod, build) is not other and len(calls) == 2                  # two slots, two caches


def test_inference_tensors_are_keyed_by_minus_one():
    with torch.inference_mode():
        w, b = torch.randn(3, 4), torch.randn(3)
    assert D.version(w) == -1 and D.version(torch.zeros(1)) == 0
    key = D.params_key(w, b)
    assert key == (w.data_ptr(), -1, w.device, (b.data_ptr(), -1))
    mod = SimpleNamespace(weight=w, bias=b)
    calls, build = _packer(mod)
    assert D.packed(mod, build) is D.packed(mod, build) and len(calls) == 1


# ------------------------------------------------------------------------------------------------ the helpers
def test_pad_cols_pads_to_the_tile_or_returns_its_argument():
    ops = Host()
    g = torch.Generator().manual_seed(3)
    for width, padded in ((8, 64), (64, 64), (72, 128)):
        t = torch.randn(5, width, generator=g).to(BF16)
        out = D.pad_cols(ops, t)
        if width == padded:
            assert out is t
            continue
        assert out is not t and out.dtype == BF16 and tuple(out.shape) == (5, padded)
        assert torch.equal(out[:, :width], t) and bool((out[:, width:] == 0).all())
    t = torch.randn(5, 3, generator=g)
    assert tuple(D.pad_cols(ops, t, 16).shape) == (5, 16) and D.pad_cols(ops, torch.zeros(5, 16), 16).shape[1] == 16
    assert ops.n_empty == 0                                                      # zeros, never empty: the padding is read
    beside = D.pad_cols(None, t.double())                                        # no backend: allocated like its argument
    assert beside.dtype == torch.float64 and tuple(beside.shape) == (5, 64) and torch.equal(beside[:, :3], t.double()) and bool((beside[:, 3:] == 0).all())


def test_row_chunks_reproduces_both_former_chunkers():
    # the literals are what neck._chunks(B, rows_per_image, row_bytes) and conv._row_chunks(M, row_bytes) returned before they became one
    assert D.row_chunks(3, 5 * (CHUNK_BYTES // 10)) == [(0, 2), (2, 1)]          # neck._chunks(3, 5, CHUNK_BYTES // 10): whole images
    assert D.row_chunks(7, CHUNK_BYTES // 3) == [(0, 3), (3, 3), (6, 1)]
    assert D.row_chunks(1, CHUNK_BYTES * 2) == [(0, 1)]                          # a row past the bound still goes, alone
    assert D.row_chunks(4, 0) == [(0, 4)] and D.row_chunks(3, 5 * 0) == [(0, 3)]
    assert D.row_chunks(4, 2 * CHUNK_BYTES) == [(0, 1), (1, 1), (2, 1), (3, 1)]  # neck._chunks(4, 2, CHUNK_BYTES)
    assert D.row_chunks(7, CHUNK_BYTES // 3 + 1) == [(0, 2), (2, 2), (4, 2), (6, 1)]


def test_rows_to_map_is_the_channel_last_view():
    N, H, W, C = 2, 3, 5, 8
    rows = torch.arange(N * H * W * C, dtype=F32).view(N * H * W, C)
    m, old = D.rows_to_map(rows, N, H, W), rows.view(N, H, W, C).permute(0, 3, 1, 2)
    assert tuple(m.shape) == (N, C, H, W) and m.stride() == old.stride() and m.data_ptr() == rows.data_ptr() and torch.equal(m, old)
    assert D.is_channel_last(m) and D.channel_last_rows(m).data_ptr() == rows.data_ptr()


def test_epilogue_and_gradient_types():
    from clipself_amd import hip
    assert (D.EPI_BF16, D.EPI_F32, D.EPI_RELU_BF16) == (hip.EPI_BF16, hip.EPI_F32, hip.EPI_RELU_BF16) == (0, 1, 9)
    assert D.epi_for(F32) == D.EPI_F32 and D.epi_for(BF16) == D.EPI_BF16
    for dtype in (F32, BF16):
        g = torch.zeros(2, dtype=dtype)
        assert D.kernel_grad(g) is g
    assert D.kernel_grad(torch.zeros(2, dtype=torch.float64)).dtype == F32 and D.kernel_grad(torch.zeros(2, dtype=torch.float16)).dtype == F32


@pytest.mark.parametrize("shape", [(2, 1, 3, 4), (2, 5, 1, 1), (2, 6, 3, 4)], ids=["C1", "H1W1", "plain"])
def test_channel_last_predicate_and_rows_on_ambiguous_strides(shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(5)
    dense = torch.randn(shape, generator=g)
    big = torch.randn(N, C + 2, H + 1, W + 1, generator=g)
    cut = big[:, 1:C + 1, :H, :W]                                                # same shape, strides of the larger tensor
    ambiguous = C == 1 or H == W == 1
    assert D.is_channel_last(dense) == ambiguous                                 # NCHW and channel-last coincide where a size is 1
    assert D.is_channel_last(dense.contiguous(memory_format=torch.channels_last)) and not D.is_channel_last(cut)
    for t in (dense, cut, dense.contiguous(memory_format=torch.channels_last)):
        rows = D.channel_last_rows(t)
        assert tuple(rows.shape) == (N * H * W, C) and rows.is_contiguous() and torch.equal(rows, t.permute(0, 2, 3, 1).reshape(N * H * W, C))
        if D.is_channel_last(t):
            assert rows.data_ptr() == t.data_ptr()                               # a view, no copy
