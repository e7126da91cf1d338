"""CPU self-checks of the poisoned-halo harness (tests/_extents.py) that the GPU suite relies on (tests/test_gpu_extents.py).

1. The whole case table through oracle.ops_ref.RefOps in place of HipOps: every case passes, i.e. the table respects each op's contract
   (shapes, strides, what the wrapper asserts) and the reference alone is bit-identical between compact and haloed tensors and leaves
   every halo alone.
2. A deliberately wrong Python stand-in op -- writes one element into an output halo / reads one halo element / ignores a row stride --
   is flagged each time, and the correct stand-in is not.  No GPU code is involved.
"""
import pytest
import torch

from _extents import BF, CASES, rnd, run_case
from oracle.ops_ref import RefOps


@pytest.fixture(scope="module")
def ref():
    return RefOps()


@pytest.mark.parametrize("name", list(CASES))
def test_case_table_holds_on_the_reference_ops(ref, name):
    for pad in (8, 64):
        problems = run_case(ref, CASES[name], "cpu", pad, key=name)
        assert not problems, f"{name} (row strides + {pad}):\n  " + "\n  ".join(problems)


class _Scale2:
    """y[M, N] (bf16) = 2 * x[M, N], with one of three bugs."""
    name = "standin"

    def __init__(self, bug=None):
        self.bug = bug

    def scale2(self, x, y):
        M, N = x.shape
        if self.bug == "ignores_ld":                   # walks x as if its rows were N apart
            x = torch.as_strided(x, (M, N), (N, 1), x.storage_offset())
        if self.bug == "writes_halo":                  # one element past the end of the first row (on compact rows: the next row's first
            torch.as_strided(y, (1, N + 1), y.stride(), y.storage_offset())[0, N] = 1.0      # element, overwritten below)
        y.copy_((2 * x.float()).to(BF))
        if self.bug == "reads_halo":                   # the first row takes one element from beyond the row's end
            wide = torch.as_strided(x, (1, N + 1), x.stride(), x.storage_offset())
            y[0, N - 1] = (2 * wide[0, N].float()).to(BF)


def _standin_case(ops, a):
    M, N = 5, 24
    x = a.inp(rnd((M, N), BF, seed=1), a.ld(N, 8))
    y = a.out((M, N), BF, a.ld(N, 8))
    ops.scale2(x, y)
    return {"y": y}


@pytest.mark.parametrize("pad", [8, 64])
def test_harness_flags_each_kind_of_extent_bug(pad):
    assert run_case(_Scale2(), _standin_case, "cpu", pad) == []
    got = run_case(_Scale2("writes_halo"), _standin_case, "cpu", pad)
    assert len(got) == 1 and "halo elements changed" in got[0], got
    got = run_case(_Scale2("reads_halo"), _standin_case, "cpu", pad)
    assert len(got) == 1 and "1 of 120 elements differ from the compact run" in got[0], got
    got = run_case(_Scale2("ignores_ld"), _standin_case, "cpu", pad)
    assert len(got) == 1 and "elements differ from the compact run" in got[0], got


def test_harness_flags_a_documented_zero_pad_that_is_not_zero():
    class Op:
        name = "standin"

        def f(self, y, leave):
            y.zero_()
            torch.as_strided(y, (y.shape[0], y.shape[1] + 2), y.stride(), y.storage_offset())[:, y.shape[1]:] = 0 if not leave else 3

    def mk(leave):
        def fn(ops, a):
            y = a.out((3, 6), BF, a.ld(8, 4), zero_pad=2)
            ops.f(y, leave)
            return {"y": y}
        return fn
    assert run_case(Op(), mk(False), "cpu", 8) == []
    got = run_case(Op(), mk(True), "cpu", 8)
    assert len(got) == 1 and "documented zero padding" in got[0], got
