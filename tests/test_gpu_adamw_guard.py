"""`-m gpu`: the guarded form of cs_adamw_step -- gradient norm over the active granules, clip coefficient, non-finite-step skip -- against
the fp64 restatement of tests/_adamw_guard_ref.py, bit for bit against the unguarded call where the guard must not change anything, inside
poisoned halos, and end to end through train_step / FlatAdamW on the tiny tower.

Sizes (S = CS_ADAMW_GUARD_SPAN, T = threads of the finalising workgroup): one chunk, three chunks, exactly one partial, one partial + one
chunk, a short last partial, and S * (T + 3) where every finalising thread takes more than one partial or none at all."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from _adamw_guard_ref import clip_coef, grad_norm, guarded_step  # noqa: E402
from _extents import bits, run_case  # noqa: E402
from clipself_amd.hip import ADAMW_GUARD_HEAD as HEAD, ADAMW_GUARD_SPAN as S  # noqa: E402
from test_gpu_ops import BF, F32, rel, rnd  # noqa: E402

T = 256                                                   # adamw.hip: GUARD_FINAL_THREADS
SIZES = [256, 768, S, S + 256, 3 * S - 256, S * (T + 3)]
PATTERNS = ["all", "ends_off", "alternating", "partial_off", "none"]
# lr, beta1, beta2, eps, weight decay as the C ABI receives them: `float` arguments.  The reference is handed the same rounded numbers --
# 1 - float(0.999) is 1.3e-5 away from 0.001, which is the kernel's input, not its error (v would carry it in full).
HYPER = tuple(float(torch.tensor(x, dtype=torch.float32)) for x in (1e-3, 0.9, 0.999, 1e-8, 0.1))
NORM_TOL = 1e-5                                           # relative; 10 x the bound the header states for the summation scheme (< 1e-6)


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def make_flags(n, pattern):
    """bit0 by pattern, bit1 (weight decay) on two granules of three."""
    gr = n // 64
    i = torch.arange(gr)
    act = torch.ones(gr, dtype=torch.bool)
    if pattern == "ends_off":
        act[0] = act[-1] = False
    elif pattern == "alternating":
        act = i % 2 == 0
    elif pattern == "partial_off":                        # a whole partial (the middle one); a single-partial buffer loses its first half
        per, parts = S // 64, (n + S - 1) // S
        k = parts // 2
        if parts > 1:
            act[k * per:(k + 1) * per] = False
        else:
            act[:max(gr // 2, 1)] = False
    elif pattern == "none":
        act[:] = False
    return (act.to(torch.uint8) | ((i % 3 != 0).to(torch.uint8) << 1)).contiguous()


_STATE = {}


def state(n):
    """Seeded p / g / m / v of n elements on the CPU, made once per size and never written.  m and v are what one AdamW step from zero
    moments leaves behind a gradient g0: a state a run can be in.  (Independent random m and v are not -- AdamW keeps |m| / sqrt(v) below
    (1 - beta1) / sqrt((1 - beta2) (1 - beta1^2 / beta2)) = 7.3, while a v drawn near zero beside an unrelated m makes single elements
    move by hundreds of lr, and the fp32 rounding of those few updates, not the kernel under test, then decides a relative L2 error.)"""
    if n not in _STATE:
        g0 = rnd((n,), F32, 1e-3, seed=71)
        _STATE[n] = dict(p=rnd((n,), F32, 0.02, seed=70), g=rnd((n,), F32, 1e-3, seed=74), m=(1 - HYPER[1]) * g0, v=(1 - HYPER[2]) * g0 * g0)
    return _STATE[n]


def run(hip, st, flags, g=None, step=2, grad_scale=1.0, guard=None, dev=None, **kw):
    """One adamw_step from the state `st` (CPU, left alone) or from the device tensors `dev` of an earlier call (updated in place)."""
    if dev is None:
        dev = {k: st[k].cuda() for k in ("p", "m", "v")}
        dev["shadow"] = st["p"].to(BF).cuda()
    g = (st["g"] if g is None else g).cuda()
    hip.adamw_step(dev["p"], g, dev["m"], dev["v"], dev["shadow"], flags.cuda(), *HYPER, step, grad_scale, guard=guard, **kw)
    torch.cuda.synchronize()
    return dev


def new_guard(hip, n):
    return torch.zeros(hip.adamw_guard_numel(n), dtype=F32, device="cuda")


def same_bits(a, b, what=("p", "m", "v", "shadow")):
    return [k for k in what if not torch.equal(bits(a[k]), bits(b[k]))]


def first_active(flags, last=False):
    idx = torch.nonzero(flags & 1)[:, 0]
    return int(idx[-1 if last else 0]) * 64 + 5


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coefficient(hip, n, pattern):
    """head[0] / head[1] against fp64 within 1e-5 relative (grad_scale 0.5, threshold = half the norm), reserved words untouched, partials
    beyond doubt (each within 2e-5 of its fp64 sum of squares); no active granule: norm 0, coefficient 1, an applied step that writes nothing."""
    st, flags = state(n), make_flags(n, pattern)
    want = grad_norm(st["g"], flags, 0.5)
    max_norm = 0.5 * want if want > 0 else 1.0
    guard = new_guard(hip, n)
    guard[4:8] = 7.0
    out = run(hip, st, flags, grad_scale=0.5, max_norm=max_norm, guard=guard)
    head = guard[:HEAD].tolist()
    print(f"n={n} {pattern}: norm {head[0]:.9g} want {want:.9g} rel {abs(head[0] - want) / max(want, 1e-30):.2e} coef {head[1]:.9g}")
    assert head[4:8] == [7.0] * 4 and head[2] == 1.0 and head[3] == 0.0
    if pattern == "none":
        assert head[0] == 0.0 and head[1] == 1.0
        before = dict(p=st["p"], m=st["m"], v=st["v"], shadow=st["p"].to(BF))
        assert same_bits({k: t.cpu() for k, t in out.items()}, before) == []
        return
    assert abs(head[0] - want) <= NORM_TOL * want
    coef = clip_coef(want, max_norm)
    assert abs(head[1] - coef) <= NORM_TOL * coef and head[1] < 0.6
    act = (flags & 1).bool().repeat_interleave(64)
    sq = torch.where(act, st["g"].double() * 0.5, torch.zeros(n, dtype=torch.float64)).square()
    sq = torch.cat([sq, torch.zeros(-n % S, dtype=torch.float64)]).view(-1, S).sum(1)
    got = guard[HEAD:].double().cpu()
    assert got.numel() == sq.numel() and bool(((got - sq).abs() <= 2 * NORM_TOL * sq).all())


@pytest.mark.parametrize("pattern", ["all", "alternating", "partial_off"])
@pytest.mark.parametrize("n", SIZES)
def test_idle_guard_changes_no_bit(hip, n, pattern):
    """Clipping off (max_norm = 0) and a threshold far above the norm: p, m, v and the shadow carry the bits of the guard=None call."""
    st, flags = state(n), make_flags(n, pattern)
    plain = run(hip, st, flags, grad_scale=0.5)
    assert not torch.equal(plain["p"].cpu(), st["p"])
    for max_norm in (0.0, 1e6):
        guard = new_guard(hip, n)
        out = run(hip, st, flags, grad_scale=0.5, max_norm=max_norm, skip_nonfinite=True, guard=guard)
        assert same_bits(out, plain) == [], max_norm
        assert guard[1].item() == 1.0 and guard[2].item() == 1.0 and guard[3].item() == 0.0


@pytest.mark.parametrize("n,pattern", list(zip(SIZES, ["all", "ends_off", "alternating", "ends_off", "partial_off", "alternating"])))
def test_clipping_active_three_steps(hip, n, pattern):
    """Gradient norm = 10 x max_norm on each of 3 steps from zero moments (the start of test_adamw_matches_torch, whose bound this is): p, m, v
    follow the fp64 reference within 1e-6."""
    flags = make_flags(n, pattern)
    st = dict(state(n), m=torch.zeros(n), v=torch.zeros(n))
    guard, dev = new_guard(hip, n), None
    ref = {k: st[k] for k in ("p", "m", "v")}
    for step in (1, 2, 3):
        g = rnd((n,), F32, 1e-3 * step, seed=90 + step)
        max_norm = grad_norm(g, flags) / 10
        dev = run(hip, st, flags, g=g, step=step, max_norm=max_norm, guard=guard, dev=dev)
        ref = guarded_step(ref["p"], g, ref["m"], ref["v"], flags, *HYPER, step, max_norm=max_norm)
        head = guard[:4].tolist()
        assert abs(head[1] - ref["coef"]) <= NORM_TOL * ref["coef"] and 0.09 < head[1] < 0.11 and head[2] == 1.0
        for k in ("p", "m", "v"):
            r = rel(dev[k], ref[k])
            print(f"n={n} step {step} {k}: rel {r:.3e}")
            assert r < 1e-6, (step, k, r)
    assert rel(dev["shadow"].float(), ref["p"]) < 4e-3               # one bf16 rounding of p
    assert guard[3].item() == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n,pattern,last", [(256, "all", False), (S + 256, "ends_off", True), (S * (T + 3), "alternating", True),
                                            (S * (T + 3), "all", False)])
def test_nonfinite_step_is_skipped(hip, n, pattern, last, bad):
    """An Inf / NaN in an active granule with skip_nonfinite: nothing is written, head[2] = 0, head[3] grows by exactly 1; the clean call
    that follows applies and leaves the count alone."""
    st, flags = state(n), make_flags(n, pattern)
    g = st["g"].clone()
    g[first_active(flags, last)] = bad
    guard = new_guard(hip, n)
    guard[3] = 2.0                                                    # two skips so far
    out = run(hip, st, flags, g=g, max_norm=1.0, skip_nonfinite=True, guard=guard)
    before = dict(p=st["p"], m=st["m"], v=st["v"], shadow=st["p"].to(BF))
    assert same_bits({k: t.cpu() for k, t in out.items()}, before) == []
    head = guard[:4].tolist()
    assert head[2] == 0.0 and head[3] == 3.0 and not torch.isfinite(guard[0]).item()
    out = run(hip, st, flags, max_norm=1.0, skip_nonfinite=True, guard=guard, dev=out)
    head = guard[:4].tolist()
    assert head[2] == 1.0 and head[3] == 3.0 and abs(head[0] - grad_norm(st["g"], flags)) <= NORM_TOL * head[0]
    assert same_bits({k: t.cpu() for k, t in out.items()}, before) == ["p", "m", "v", "shadow"]
    assert all(bool(torch.isfinite(out[k].float()).all()) for k in out)


def test_nonfinite_step_proceeds_without_the_skip(hip):
    """skip_nonfinite = 0: the arithmetic proceeds as clip_grad_norm_(error_if_nonfinite=False) + AdamW would -- applied, nothing counted."""
    n = 768
    st, flags = state(n), make_flags(n, "all")
    g = st["g"].clone()
    g[5] = float("inf")
    guard = new_guard(hip, n)
    out = run(hip, st, flags, g=g, max_norm=1.0, skip_nonfinite=False, guard=guard)
    assert guard[:4].tolist()[2:] == [1.0, 0.0] and not bool(torch.isfinite(out["p"]).all())


@pytest.mark.parametrize("n,pattern", [(768, "ends_off"), (S + 256, "alternating"), (3 * S - 256, "partial_off"), (S * (T + 3), "partial_off")])
def test_nan_in_inactive_granules_is_ignored(hip, n, pattern):
    st, flags = state(n), make_flags(n, pattern)
    act = (flags & 1).bool().repeat_interleave(64)
    g_zero = torch.where(act, st["g"], torch.zeros(n))
    g_nan = torch.where(act, st["g"], torch.full((n,), float("nan")))
    outs = []
    for g in (g_zero, g_nan):
        guard = new_guard(hip, n)
        out = run(hip, st, flags, g=g, max_norm=0.01, skip_nonfinite=True, guard=guard)
        out["guard"] = guard
        outs.append(out)
    assert same_bits(outs[0], outs[1], ("p", "m", "v", "shadow", "guard")) == []
    assert outs[1]["guard"][2].item() == 1.0 and outs[1]["guard"][1].item() < 1.0


@pytest.mark.parametrize("n", [S + 256, S * (T + 3)])
def test_same_call_same_bits(hip, n):
    st, flags = state(n), make_flags(n, "ends_off")
    outs = []
    for _ in range(2):
        guard = new_guard(hip, n)
        out = run(hip, st, flags, max_norm=0.01, skip_nonfinite=True, guard=guard)
        out["guard"] = guard
        outs.append(out)
    assert same_bits(outs[0], outs[1], ("p", "m", "v", "shadow", "guard")) == []


def _guarded_extents_case(n):
    def fn(ops, a):                                        # _adamw_case of tests/_extents.py + the guard, at exactly adamw_guard_numel(n) floats
        flags = torch.tensor([3, 1, 0, 2, 1, 0, 3, 3] * (n // 512 + 1), dtype=torch.uint8)[:n // 64]
        p, m, v = (a.out((n,), F32, init=rnd((n,), F32, s, seed=70 + i)) for i, s in enumerate((0.02, 1e-3, 1e-3)))
        v.abs_()
        sh = a.out((n,), BF, init=torch.zeros(n, dtype=BF))
        numel = ops.adamw_guard_numel(n)
        guard = a.out((numel,), F32, init=torch.zeros(numel), name="guard")
        ops.adamw_step(p, a.inp(rnd((n,), F32, 1e-3, seed=74)), m, v, sh, a.inp(flags), *HYPER, 2, max_norm=0.01, skip_nonfinite=True,
                       guard=guard)
        return {"p": p, "m": m, "v": v, "shadow": sh, "guard": guard}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("n", [512, 1536, S + 256])
def test_guarded_extents(hip, n, pad):
    """g, flags and guard inside poisoned halos: same bits as the compact run, no halo element touched."""
    problems = run_case(hip, _guarded_extents_case(n), "cuda", pad, key=f"adamw_step_guarded[{n}]")
    assert not problems, problems


def _args(**kw):
    base = dict(device="cuda", precision="amp", distributed=False, skip_scheduler=True, grad_clip_norm=None, multiscale=False,
                extract_type="v2", cosine_weight=1.0)
    base.update(kw)
    return SimpleNamespace(**base)


def test_train_step_clips_and_skips_on_the_device():
    """Two identical tiny students, one batch, --grad-clip-norm at a tenth of the gradient norm: the torch passage (ADAMW_GUARD masked) and
    the guarded step give the same masters within 1e-6, the guarded one leaves p.grad unscaled; then an Inf in the gradient buffer with
    skip_nonfinite leaves master, shadow and both moments bitwise alone, and the next ordinary step trains again."""
    from clipself_amd.config import tiny_cfg
    from clipself_amd.init import synthetic_batch
    from clipself_amd.training.clipself import CLIPSelf
    from clipself_amd.training.optim import FlatAdamW
    from clipself_amd.training.precision import get_autocast
    from clipself_amd.training.train import train_step
    from test_gpu_step import _pair
    cfg = tiny_cfg()
    batch = synthetic_batch(2, 3, cfg.image_size, cfg.image_size, seed=40)

    def fwd_bwd(model, teacher, opt):
        opt.zero_grad()
        args = _args()
        with get_autocast(args.precision)():
            losses, _, _ = CLIPSelf()(batch, model, teacher, None, torch.device("cuda"), torch.bfloat16 if args.precision == "bf16" else None,
                                      False, args)
        sum(losses.values()).backward()

    a, teacher = _pair(cfg, 1)
    b, _ = _pair(cfg, 1)
    ea, eb = a.visual.engine, b.visual.engine
    opt_a, opt_b = FlatAdamW(a, lr=1e-3, weight_decay=0.1), FlatAdamW(b, lr=1e-3, weight_decay=0.1)
    fwd_bwd(a, teacher, opt_a)
    norm = float(ea.grad.double().norm())
    clip = norm / 10
    ea.ops.ADAMW_GUARD = False                                        # an instance attribute: today's torch passage for model a only
    assert not opt_a.guard_available() and opt_b.guard_available()
    start = eb.master.clone()
    train_step(a, CLIPSelf(), batch, opt_a, None, 0, teacher, _args(grad_clip_norm=clip))
    train_step(b, CLIPSelf(), batch, opt_b, None, 0, teacher, _args(grad_clip_norm=clip))
    assert ea.guard is None and opt_a.grad_stats() is None
    stats = opt_b.grad_stats()
    print(f"gradient norm {norm:.6g}, guarded step: {stats}; masters rel {rel(eb.master, ea.master):.3e}")
    assert abs(float(ea.grad.double().norm()) - clip) < 1e-3 * clip          # a's gradient was rescaled in place ...
    assert abs(float(eb.grad.double().norm()) - norm) < 1e-6 * norm          # ... b's was not
    assert abs(stats["norm"] - norm) <= NORM_TOL * norm and abs(stats["clip_coef"] - 0.1) < 1e-5 and stats["applied"] and stats["skipped_total"] == 0
    assert rel(eb.master, ea.master) < 1e-6 and not torch.equal(eb.master, start)
    assert rel(eb.exp_avg, ea.exp_avg) < 1e-6 and rel(eb.exp_avg_sq, ea.exp_avg_sq) < 1e-6

    fwd_bwd(b, teacher, opt_b)
    eb.grad[int(torch.nonzero(eb.flags & 1)[0]) * 64 + 3] = float("inf")
    snap = {k: getattr(eb, k).clone() for k in ("master", "shadow", "exp_avg", "exp_avg_sq")}
    opt_b.step(skip_nonfinite=True)
    for k, t in snap.items():
        assert torch.equal(bits(getattr(eb, k)), bits(t)), k
    stats = opt_b.grad_stats()
    assert stats["skipped_total"] == 1 and not stats["applied"] and opt_b.step_count == 2
    train_step(b, CLIPSelf(), batch, opt_b, None, 2, teacher, _args())
    assert not torch.equal(eb.master, snap["master"]) and bool(torch.isfinite(eb.master).all())
    assert opt_b.grad_stats()["skipped_total"] == 1                           # an unguarded step leaves the guard alone
