"""`-m gpu`: the attention kernels on operands with known answers (tests/_attn_exact.py): every element of o, every lse and every gradient
element on its own -- bit for bit where the construction is exact (needle, tied pair), inside bounds derived from the kernels' rounding
points elsewhere (uniform o and dQ, lse in fp32 ulps).  The relative-L2 checks of test_gpu_ops.py / test_gpu_attn_norope.py / test_gpu_text.py
/ test_gpu_maskattn_train.py pass a dropped key, a wrong table row or two swapped V rows of one query row; these do not
(tests/test_attn_exact_cpu.py shows both on a float64 model).  Outputs are pre-filled with NaN.  Figures go to the per-kernel metrics file
(test_gpu_ops._metric) and are printed before they are asserted (pytest -s); measured values: profiles/attn_exact.md.

Measured on an MI355X (profiles/attn_exact.md): every exact check holds bit for bit; lse within 1.27 ulps (image kernels, bound 3) and
0.27 ulps (query kernel, bound 5); the uniform case uses up to 0.998 of its o bound (a rounding to bf16 reaches half a spacing) and 0.58 of
its dQ bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_exact as X  # noqa: E402
from test_gpu_ops import _metric  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SCALE = X.SCALE


@pytest.fixture(scope="module")
def hip():
    from clipself_amd.hip import HipOps
    return HipOps()


def _nan(shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _dev(t):
    return None if t is None else t.cuda()


def _same(name, a, b, problems):
    if not torch.equal(a, b):
        problems.append(f"{name}: {int((a != b).sum())} of {a.numel()} elements differ")


def _report(tag, metrics, problems):
    line = f"attn_exact {tag}: " + " ".join(f"{k} {v:.4g}" for k, v in sorted(metrics.items())) + (f" PROBLEMS {len(problems)}" if problems else "")
    print(line)
    _metric(line)
    assert not problems, f"{tag}:\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ image kernels
def _run_image(hip, c, tables, problems, metrics):
    B, N, H = c.B, c.N, c.H
    C = H * 64
    inp = X.image_inputs(c, tables)
    tag = f"{c.kind}[{B},{N},{H},{tables}]"
    qkv, dout, o_in, lse_in, cos, sin = (_dev(t) for t in (inp.qkv, inp.dout, inp.o_in, inp.lse_in, inp.cos, inp.sin))
    out, lse, out2 = _nan((B * N, C)), _nan((B * H, N), F32), _nan((B * N, C))
    hip.attn_fwd(qkv, cos, sin, out, lse, B, N, H, SCALE)
    hip.attn_fwd(qkv, cos, sin, out2, None, B, N, H, SCALE)
    out3, lse3, part = _nan((B * N, C)), _nan((B * H, N), F32), _nan((H, B * N, 2), F32)
    hip.attn_fwd_stats(qkv, cos, sin, out3, lse3, part, B, N, H, SCALE)
    ws = torch.empty(hip.attn_bwd_workspace(B, N, H), dtype=torch.uint8, device="cuda")
    dqkv = _nan((B * N, 3 * C))
    hip.attn_bwd(qkv, o_in, dout, lse_in, cos, sin, dqkv, ws, B, N, H, SCALE)      # fed the expected o and lse
    torch.cuda.synchronize()
    m = X.check_image_forward(tag, inp, out, lse, problems, stats_part=part)
    _same(tag + ".o without lse", out2, out, problems)
    _same(tag + ".o of attn_fwd_stats", out3, out, problems)
    _same(tag + ".lse of attn_fwd_stats", lse3, lse, problems)
    m.update(X.check_image_backward(tag, inp, dqkv, problems))
    for k, v in m.items():
        metrics[k] = max(metrics.get(k, 0.0), v)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("shape", X.IMAGE_SQUARE, ids=lambda s: "x".join(map(str, s)))
def test_image_kernels_on_known_answers(hip, shape, kind):
    """cs_attn_fwd, cs_attn_fwd_stats and cs_attn_bwd with quarter-turn tables, identity tables and NULL tables."""
    c = X.image_case(kind, *shape)
    problems, metrics = [], {}
    for tables in X.TABLES:
        _run_image(hip, c, tables, problems, metrics)
    _report(f"{kind}{list(shape)}", metrics, problems)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("Ntok", X.IMAGE_NON_SQUARE)
def test_image_kernels_on_known_answers_at_any_token_count(hip, Ntok, kind):
    """Token counts without a grid (and the smallest sequence): NULL tables only."""
    c = X.image_case(kind, 2, Ntok, 2)
    problems, metrics = [], {}
    _run_image(hip, c, "null", problems, metrics)
    _report(f"{kind}[2,{Ntok},2]", metrics, problems)


# ------------------------------------------------------------------------------------------------ the CLS query
@pytest.mark.parametrize("kind", ["needle", "tied_lo", "tied_hi"])
@pytest.mark.parametrize("Ntok,H", X.CLS_SHAPES)
def test_cls_query_on_known_answers(hip, Ntok, H, kind):
    """cs_attn_cls_fwd: one image per probe (the hit lands in every 32-key pass and on the last key), every head-group instantiation,
    a padded row stride; the same rows through cs_attn_query_fwd with every key allowed, whose lse is checked too."""
    c = X.cls_case(kind, Ntok, H)
    B, C = c.B, H * 64
    problems, metrics = [], {}
    for tables in X.TABLES:
        cos, sin = X.make_tables(tables, Ntok)
        ld = 3 * C + 8
        qkv = torch.full((B * Ntok, ld), float("nan"), dtype=BF)
        qkv[:, C:2 * C] = X.to_bf16_exact(X.rows_of(X.unrotate(c.base.k, cos, sin)), "k")
        qkv[:, 2 * C:3 * C] = X.to_bf16_exact(X.rows_of(c.base.v), "v")
        qkv.view(B, Ntok, ld)[:, 0, :C] = X.to_bf16_exact(X.rows_of(c.q), "q")       # the CLS query is never rotated
        qkv = qkv.cuda()
        out = _nan((B, C + 8))
        hip.attn_cls_fwd(qkv.view(B, Ntok, ld)[:, 0, :C], qkv[:, C:3 * C], _dev(cos), _dev(sin), out[:, :C], B, Ntok, H, SCALE)
        torch.cuda.synchronize()
        X.check_exact(f"cls.{kind}[{Ntok},{H},{tables}].o", out[:, :C], X.rows_of(c.o), problems)
        if not bool(torch.isnan(out[:, C:]).all()):
            problems.append(f"cls.{kind}[{Ntok},{H},{tables}]: the padding of the output rows was written")
        if tables == "null":
            ones = torch.ones(B, Ntok, dtype=torch.uint8, device="cuda")
            out2, lse = _nan((B, C)), _nan((B * H, 1), F32)
            hip.attn_query_fwd(qkv.view(B, Ntok, ld)[:, 0, :C], qkv[:, C:3 * C], ones, out2, B, 1, Ntok, H, SCALE, lse=lse)
            torch.cuda.synchronize()
            X.check_exact(f"query(all allowed).{kind}[{Ntok},{H}].o", out2, X.rows_of(c.o), problems)
            metrics["lse_ulps"] = X.check_lse(f"query(all allowed).{kind}[{Ntok},{H}].lse", lse, c.lse, X.LSE_ULPS_QUERY, problems)
    _report(f"cls.{kind}[{Ntok},{H}]", metrics, problems)


# ------------------------------------------------------------------------------------------------ allow masks
@pytest.mark.parametrize("kind", ["needle", "tied_lo", "tied_hi"])
@pytest.mark.parametrize("shape", X.QUERY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_query_rows_with_allow_masks_on_known_answers(hip, shape, kind):
    """cs_attn_query_fwd: the needle key disallowed (the runner-up wins exactly), one partner of a tied pair disallowed, and rows that allow no
    key at all (o = 0, lse = +inf)."""
    B, Q, Ntok, H = shape
    C = H * 64
    c = X.query_case(kind, *shape)
    qkv = torch.full((B * Ntok, 3 * C), float("nan"), dtype=BF)
    qkv[:, C:2 * C] = X.to_bf16_exact(X.rows_of(c.k), "k")
    qkv[:, 2 * C:] = X.to_bf16_exact(X.rows_of(c.v), "v")
    qkv, q, allow = qkv.cuda(), X.to_bf16_exact(X.rows_of(c.q), "q").cuda(), c.allow.cuda()
    out, lse, out2 = _nan((B * Q, C)), _nan((B * H, Q), F32), _nan((B * Q, C))
    hip.attn_query_fwd(q, qkv[:, C:], allow, out, B, Q, Ntok, H, SCALE, lse=lse)
    hip.attn_query_fwd(q, qkv[:, C:], allow, out2, B, Q, Ntok, H, SCALE)
    torch.cuda.synchronize()
    problems, tag = [], f"query.{kind}{list(shape)}"
    X.check_exact(tag + ".o", out, X.rows_of(c.o), problems)
    _same(tag + ".o without lse", out2, out, problems)
    ulps = X.check_lse(tag + ".lse", lse, c.lse.reshape(B * H, Q), X.LSE_ULPS_QUERY, problems)
    _report(tag, {"lse_ulps": ulps}, problems)


# ------------------------------------------------------------------------------------------------ causal self-attention
@pytest.mark.parametrize("B,L,H", X.CAUSAL_SHAPES)
def test_causal_attention_on_known_answers(hip, B, L, H):
    """cs_attn_query_fwd(allow = NULL): a needle in the past wins; when a row's best key lies in the future, its best past key wins."""
    C = H * 64
    c = X.causal_case(B, L, H)
    qkv = X.to_bf16_exact(torch.cat([X.rows_of(c.q), X.rows_of(c.k), X.rows_of(c.v)], 1), "qkv").cuda()
    out = _nan((B * L, C))
    hip.attn_query_fwd(qkv[:, :C], qkv[:, C:], None, out, B, L, L, H, SCALE)
    torch.cuda.synchronize()
    problems, tag = [], f"causal[{B},{L},{H}]"
    X.check_exact(tag + ".o", out, X.rows_of(c.o), problems)
    _report(tag, {"rows_with_the_best_key_in_the_future": float(c.future.sum())}, problems)


# ------------------------------------------------------------------------------------------------ passenger backward
@pytest.mark.parametrize("kind", ["tied_lo", "tied_hi"])
@pytest.mark.parametrize("shape", X.PASSENGER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_passenger_backward_on_known_answers(hip, shape, kind):
    """cs_attn_bwd(extra=) without image rows: tied pairs under allow masks; the passengers' dq and the dK | dV written to dqkv are exact."""
    B, Q, Ntok, H = shape
    C = H * 64
    c = X.passenger_case(kind, *shape)
    qkv = torch.zeros(B * Ntok, 3 * C, dtype=BF)
    qkv[:, C:2 * C] = X.to_bf16_exact(X.rows_of(c.k), "k")
    qkv[:, 2 * C:] = X.to_bf16_exact(X.rows_of(c.v), "v")
    qkv = qkv.cuda()
    q, o, dout = (X.to_bf16_exact(X.rows_of(t), n).cuda() for t, n in ((c.q, "q"), (c.o, "o"), (c.dout, "dout")))
    lse, allow = c.lse.reshape(B * H, Q).to(F32).cuda(), c.allow.cuda()
    ws = torch.empty(hip.attn_bwd_workspace(B, Ntok, H, Q), dtype=torch.uint8, device="cuda")
    want = torch.cat([torch.zeros(B * Ntok, C, dtype=torch.float64), X.rows_of(c.dk), X.rows_of(c.dv)], 1)
    problems = []
    for tables in ("null", "ident"):
        cos, sin = X.make_tables(tables, Ntok)
        dq, dqkv = _nan((B * Q, C)), _nan((B * Ntok, 3 * C))
        hip.attn_bwd(qkv, None, None, None, _dev(cos), _dev(sin), dqkv, ws, B, Ntok, H, SCALE,
                     extra=dict(q=q, o=o, dout=dout, lse=lse, allow=allow, dq=dq, Q=Q))
        torch.cuda.synchronize()
        tag = f"passengers.{kind}{list(shape)}.{tables}"
        X.check_exact(tag + ".extra.dq", dq, X.rows_of(c.dq), problems)
        for name, sl in (("dq(image rows)", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
            X.check_exact(f"{tag}.{name}", dqkv[:, sl], want[:, sl], problems)
    _report(f"passengers.{kind}{list(shape)}", {"non_zero_dq": float((c.dq != 0).sum())}, problems)
