"""`-m gpu`: the text tower on the MI355X.

Op level    cs_attn_query_fwd(allow == NULL), causal self-attention (attn_causal_kernel), against tests/_text_ref.RefOpsText, against the
            masked kernel fed an explicit lower-triangular `allow` table (the only way the ABI could express it before), bit-exact
            first rows, bit-exact causality, bit-reproducibility, argument errors.
Extents     the causal form inside poisoned halos (tests/_extents.py's harness; its case table is not touched).
Tower level encode_text of both model families on HipOps against the vectors of the real reference (tools/gen_golden_text.py), against
            the CPU run of the same model on RefOpsText, and at the two real text widths.
Bounds: profiles/text_tower_parity.md.
"""
import ctypes
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from _extents import run_case  # noqa: E402
from _text_ref import BOUND_ONE_MINUS_COS, BOUND_REL_L2, BOUND_SAME_ROUNDING, FIXTURES, RefOpsText, build_model, load_fixture, one_minus_cos, rel_l2  # noqa: E402
from test_gpu_ops import BF, F32, check, rnd  # noqa: E402

SCALE = 0.125
# the smallest shapes that cross every 32-row tile boundary (1 / 2 / 3 / 4 waves per unit) and every packing remainder (B * H not a
# multiple of the 4 resp. 2 units of a workgroup), with both real head counts
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 31, 2), (3, 32, 8), (2, 33, 12), (5, 64, 8), (2, 65, 2), (3, 77, 8), (2, 77, 12), (1, 96, 2), (1, 97, 2),
          (2, 128, 2)]


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


_DATA = {}


def data(B, L, H):
    """(q|k|v bf16 [B*L, 3C] on the CPU, reference output): inputs scaled like test_attention_extra_query_tokens_with_key_masks (q and k
    x 2: scores of a few units, a softmax far from uniform); the reference is computed once per shape."""
    key = (B, L, H)
    if key not in _DATA:
        C = H * 64
        qkv = rnd((B * L, 3 * C), F32, 1.0, seed=90 + L)
        qkv[:, :2 * C] *= 2.0
        qkv = qkv.to(BF)
        o_r = torch.empty(B * L, C, dtype=BF)
        RefOpsText().attn_query_fwd(qkv[:, :C], qkv[:, C:], None, o_r, B, L, L, H, SCALE)
        _DATA[key] = (qkv, o_r)
    return _DATA[key]


def causal(hip, qkv_d, B, L, H):
    C = H * 64
    out = torch.full((B * L, C), float("nan"), dtype=BF, device="cuda")
    hip.attn_query_fwd(qkv_d[:, :C], qkv_d[:, C:], None, out, B, L, L, H, SCALE)
    return out


@pytest.mark.parametrize("B,L,H", SHAPES)
def test_causal_attention_op(hip, B, L, H):
    C = H * 64
    qkv, o_r = data(B, L, H)
    qkv_d = qkv.cuda()
    o_d = causal(hip, qkv_d, B, L, H)
    tag = f"attn_causal[{B},{L},{H}]"
    check(tag + ".o", o_d, o_r, 6e-3)                                        # 1. the reference op at the kernel's rounding points
    if L > 1:                                                                # 2. the masked kernel with a lower-triangular table (its Ntok > 1)
        allow = torch.ones(L, L, dtype=torch.uint8).tril_().repeat(B, 1).cuda()
        o_m = torch.full((B * L, C), float("nan"), dtype=BF, device="cuda")
        hip.attn_query_fwd(qkv_d[:, :C], qkv_d[:, C:], allow, o_m, B, L, L, H, SCALE)
        check(tag + ".vs_masked", o_d, o_m, 6e-3)
    v = qkv_d[:, 2 * C:].reshape(B, L, C)                                    # 3. a softmax over one key: row 0 is v row 0, bit for bit
    assert torch.equal(o_d.view(B, L, C)[:, 0], v[:, 0])
    assert torch.equal(causal(hip, qkv_d, B, L, H), o_d)                     # 5. two launches, equal bits
    # an output whose rows are only 2-byte aligned (the entry point sets no alignment rule for `out`): the same bits, nothing else written
    big = torch.full((B * L, C + 8), 5.0, dtype=BF, device="cuda")
    hip.attn_query_fwd(qkv_d[:, :C], qkv_d[:, C:], None, big[:, 1:C + 1], B, L, L, H, SCALE)
    assert torch.equal(big[:, 1:C + 1], o_d) and bool((big[:, :1] == 5.0).all()) and bool((big[:, C + 1:] == 5.0).all())


@pytest.mark.parametrize("B,L,H", [s for s in SHAPES if s[1] > 1])
def test_causal_attention_never_looks_ahead(hip, B, L, H):
    """4. k and v rows > j of ONE sequence replaced by other finite values (not NaN: 0 * NaN is NaN in any implementation): output rows
    <= j of that sequence and every row of every other sequence keep their bits."""
    C = H * 64
    qkv, _ = data(B, L, H)
    qkv_d = qkv.cuda()
    base = causal(hip, qkv_d, B, L, H).view(B, L, C)
    b = B // 2
    for j in sorted({j for j in (0, 30, 31, 32, L - 2) if 0 <= j <= L - 2}):
        other = qkv_d.clone().view(B, L, 3 * C)
        other[b, j + 1:, C:] = (rnd((L - 1 - j, 2 * C), F32, 3.0, seed=200 + j) + 0.5).to(BF).cuda()
        got = causal(hip, other.view(B * L, 3 * C), B, L, H).view(B, L, C)
        assert torch.equal(got[b, :j + 1], base[b, :j + 1]), f"[{B},{L},{H}] j={j}: rows <= j changed"
        keep = [i for i in range(B) if i != b]
        assert torch.equal(got[keep], base[keep]), f"[{B},{L},{H}] j={j}: another sequence changed"
        assert not torch.equal(got[b, j + 1:], base[b, j + 1:]), "the perturbation must reach the rows that may see it"


def test_causal_attention_argument_errors(hip):
    """6. Ntok = 129, Q != Ntok and an lse pointer with allow == NULL: -1 and a cs_last_error text, nothing launched (the output keeps its fill)."""
    B, L, H = 1, 8, 1
    C = H * 64
    qkv = torch.zeros(B * 129, 3 * C, dtype=BF, device="cuda")
    out = torch.full((B * 129, C), 7.0, dtype=BF, device="cuda")
    lse = torch.full((B * H * L,), 7.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(Q, Ntok, lse_t):
        return hip.lib.cs_attn_query_fwd(qkv.data_ptr(), qkv[:, C:].data_ptr(), None, out.data_ptr(), lse_t.data_ptr() if lse_t is not None else None,
                                         B, Q, Ntok, H, 3 * C, 3 * C, C, ctypes.c_float(SCALE), stream)

    assert call(L, L, None) == 0                                             # the same call with legal arguments runs
    torch.cuda.synchronize()
    out.fill_(7.0)
    for what, (Q, Ntok, lse_t) in {"Ntok": (129, 129, None), "Q": (L - 1, L, None), "lse": (L, L, lse)}.items():
        assert call(Q, Ntok, lse_t) == -1, what
        msg = hip.lib.cs_last_error().decode()
        assert "cs_attn_query_fwd" in msg and what in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())
    with pytest.raises(AssertionError):                                      # the tensor-level wrapper refuses before the library does
        hip.attn_query_fwd(qkv[:, :C], qkv[:, C:], None, out, B, 129, 129, H, SCALE)


# ------------------------------------------------------------------------------------------------ extents
def _causal_case(B, L, H):
    def fn(ops, a):
        C = H * 64
        qkv = a.inp(data(B, L, H)[0], a.ld(3 * C, 8))
        out = a.out((B * L, C), BF, a.ld(C, 8))
        ops.attn_query_fwd(qkv[:, :C], qkv[:, C:], None, out, B, L, L, H, SCALE)
        return {"out": out}
    return fn


@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("B,L,H", [(2, 77, 2), (3, 33, 2), (1, 1, 1)])
def test_causal_attention_extents(hip, B, L, H, pad):
    """q|k|v and the output as views inside NaN / sentinel halos with padded row strides: bit-identical to the compact run, no halo
    element changed, no element excluded (rows past a sequence's end are re-reads of its last row, never the halo's NaN)."""
    name = f"attn_causal[{B},{L},{H}]"
    problems = run_case(hip, _causal_case(B, L, H), "cuda", pad, key=name)
    assert not problems, f"{name} (row strides + {pad}):\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ tower level
_CPU = {}


def cpu_run(key, cfg, ids, seed):
    """encode_text of the same model on the CPU (RefOpsText: the kernels' rounding points in torch), once per model."""
    if key not in _CPU:
        _CPU[key] = build_model(cfg, RefOpsText(), seed).encode_text(ids)
    return _CPU[key]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_encode_text_matches_the_reference(hip, name):
    cfg, ids, gold, _, seed = load_fixture(name)
    model = build_model(cfg, hip, seed)
    trimmed, full = model.encode_text(ids), model.encode_text(ids, trim=False)
    assert trimmed.is_cuda and trimmed.dtype == F32 and not trimmed.requires_grad and trimmed.shape == gold.shape
    cpu = cpu_run(name, cfg, ids, seed)
    r0, c0 = rel_l2(cpu, gold), one_minus_cos(cpu, gold)
    print(f"\n{name} cpu(RefOpsText) vs golden: rel-L2 {r0:.3e}  max(1 - cos) {c0:.3e}")
    for tag, got in (("trimmed", trimmed), ("trim=False", full)):
        r, c, same = rel_l2(got, gold), one_minus_cos(got, gold), rel_l2(got, cpu)
        print(f"{name} hip {tag} vs golden: rel-L2 {r:.3e}  max(1 - cos) {c:.3e}   vs cpu: rel-L2 {same:.3e}")
        assert r <= BOUND_REL_L2 and c <= BOUND_ONE_MINUS_COS, (name, tag, r, c)
        # the kernels against the emulation of their own rounding points: more than twice its error is a kernel defect, not a tolerance
        assert r <= 2 * r0 and c <= 2 * c0, (name, tag, r, r0, c, c0)
        assert same <= BOUND_SAME_ROUNDING, (name, tag, same)
    print(f"{name}: trimmed vs untrimmed rel-L2 {rel_l2(trimmed, full):.3e}, max abs {float((trimmed - full).abs().max()):.3e}")
    assert rel_l2(trimmed, full) <= BOUND_SAME_ROUNDING
    n = model.encode_text(ids, normalize=True)
    assert torch.allclose(n.norm(dim=-1), torch.ones(ids.shape[0], device="cuda"), atol=1e-5)


@pytest.mark.parametrize("width,heads", [(512, 8), (768, 12)])
def test_encode_text_at_real_text_widths(hip, width, heads):
    """The two shipped text shapes (512 / 8 heads, 768 / 12 heads; vocab 49408, context 77) with 2 layers on a tiny vision tower: 16
    prompts whose end-of-text ids sit at positions 3 .. 40 -- HIP against the CPU run of the same schedule."""
    from clipself_amd.config import tiny_text_cfg
    cfg = dataclasses.replace(tiny_text_cfg("openai"), name=f"ViT-tiny-text{width}-test", embed_dim=width, text_width=width, text_heads=heads,
                              text_vocab=49408, text_context=77)
    g = torch.Generator().manual_seed(width)
    ids = torch.zeros(16, 77, dtype=torch.long)
    for row, eot in enumerate(torch.linspace(3, 40, 16).round().long().tolist()):
        ids[row, :eot] = torch.randint(1, 49406, (eot,), generator=g)
        ids[row, eot] = 49407
    got = build_model(cfg, hip, 13).encode_text(ids)
    want = cpu_run(("real", width), cfg, ids, 13)
    r, c = rel_l2(got, want), one_minus_cos(got, want)
    print(f"\ntext {width}/{heads}: hip vs cpu(RefOpsText) rel-L2 {r:.3e}  max(1 - cos) {c:.3e}")
    assert got.shape == (16, width) and bool(torch.isfinite(got).all())
    assert r <= BOUND_SAME_ROUNDING and c <= BOUND_ONE_MINUS_COS
