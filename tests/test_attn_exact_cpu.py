"""CPU: the attention cases with known answers (tests/_attn_exact.py) are what they claim to be, and their checks reject what the
relative-L2 checks of the GPU suite accept.

(1) the helper's expected values (index arithmetic) equal dense float64 attention rounded once to bf16, and RefOps.attn_fwd / attn_bwd bit
    for bit (uniform case: inside its bounds); every case of the GPU lists builds, i.e. its preconditions and representability asserts hold;
(2) mutations of a float64 model of the operation, each touching one row or one token of one head, are rejected by the new checks -- and
    accepted by check(..., 4e-3) on the random operands of the GPU suite (the gap that tests/test_gpu_attn_exact.py closes).
Figures are printed before they are asserted (pytest -s)."""
import pytest
import torch

import _attn_exact as X
from oracle.ops_ref import RefOps, _rope_rows

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _dense64(inp):
    """float64 attention forward and backward on the kernel-side inputs of a case (the backward at the o the case feeds it)."""
    c = inp.case
    B, N, H = c.B, c.N, c.H
    C = H * 64
    rot = (lambda t: t) if inp.cos is None else (lambda t: _rope_rows(t, inp.cos.double(), inp.sin.double()))
    q, k, v = (X.heads_of(inp.qkv[:, j * C:(j + 1) * C], B, N, H) for j in range(3))
    q, k = rot(q), rot(k)
    do, og = X.heads_of(inp.dout, B, N, H), X.heads_of(inp.o_in, B, N, H)
    s = (q @ k.transpose(-1, -2)) * X.SCALE
    p = torch.softmax(s, -1)
    o, lse = p @ v, torch.logsumexp(s, -1)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * og).sum(-1, keepdim=True)) * X.SCALE
    dq, dk = X.unrotate(ds @ k, inp.cos, inp.sin), X.unrotate(ds.transpose(-1, -2) @ q, inp.cos, inp.sin)
    return X.rows_of(o), lse.reshape(B * H, N), torch.cat([X.rows_of(dq), X.rows_of(dk), X.rows_of(dv)], 1)


@pytest.mark.parametrize("tables", ["quarter", "ident"])
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("N", [17, 65, 197, 226])
def test_expected_values_equal_float64_and_refops(N, kind, tables):
    B, H = 2, 2
    C = H * 64
    c = X.image_case(kind, B, N, H)
    inp = X.image_inputs(c, tables)
    o64, lse64, g64 = _dense64(inp)
    bf = lambda t: t.to(F32).to(BF).double()
    assert float((lse64 - c.lse.reshape(B * H, N)).abs().max()) <= 1e-12 * float(lse64.abs().max())
    if c.exact:
        assert torch.equal(bf(o64), bf(X.rows_of(c.o))) and torch.equal(bf(X.rows_of(c.o)), X.rows_of(c.o))
        assert torch.equal(bf(g64), bf(inp.want_dqkv)), int((bf(g64) != bf(inp.want_dqkv)).sum())
        if kind == "needle":
            assert float(inp.want_dqkv[:, :2 * C].abs().max()) == 0.0 and float(inp.want_dqkv[:, 2 * C:].abs().max()) > 0
        else:
            nz = [float((inp.want_dqkv[:, j * C:(j + 1) * C] != 0).double().mean()) for j in range(3)]
            print(f"{kind}[{N}] non-zero share of dq / dk / dv: {nz}")
            assert min(nz) > 0.005                                   # the backward is not trivial
    else:
        assert float((o64 - X.rows_of(c.o)).abs().max()) <= 1e-12
        assert float((g64[:, :C] - inp.want_dqkv[:, :C]).abs().max()) <= 1e-12        # dQ at p = 1 / N
        assert float(g64[:, C:2 * C].abs().max()) <= 1e-12                            # dK = 0
        assert float((g64[:, 2 * C:] - inp.want_dqkv[:, 2 * C:]).abs().max()) <= 2.0 ** -6 * float(g64[:, 2 * C:].abs().max())
    # RefOps at the kernels' rounding points: the GPU checks themselves must pass on it (bit for bit in the exact cases)
    ref = RefOps()
    o, lse = torch.empty(B * N, C, dtype=BF), torch.empty(B * H, N)
    ref.attn_fwd(inp.qkv, inp.cos, inp.sin, o, lse, B, N, H, X.SCALE)
    part = torch.empty(H, B * N, 2)
    ref.attn_fwd_stats(inp.qkv, inp.cos, inp.sin, o, lse, part, B, N, H, X.SCALE)
    dqkv = torch.zeros(B * N, 3 * C, dtype=BF)
    ref.attn_bwd(inp.qkv, inp.o_in, inp.dout, inp.lse_in, inp.cos, inp.sin, dqkv, None, B, N, H, X.SCALE)
    problems = []
    m = X.check_image_forward(f"ref.{kind}[{N},{tables}]", inp, o, lse, problems, stats_part=part)
    m.update(X.check_image_backward(f"ref.{kind}[{N},{tables}]", inp, dqkv, problems))
    print(f"RefOps {kind}[{N},{tables}]: {m}")
    assert not problems, "\n".join(problems)


def test_every_gpu_case_builds():
    """The preconditions (score gaps, representability, exact sums, no bf16 tie of 1 / N) and the table layout for every shape of the GPU lists."""
    from clipself_amd.hip import HipOps
    for B, N, H in X.IMAGE_SQUARE + [(2, n, 2) for n in X.IMAGE_NON_SQUARE]:
        for kind in X.KINDS:
            c = X.image_case(kind, B, N, H)
            assert c.gap >= X.GAP
            for tables in (X.TABLES if X.is_square(N) and N > 2 else ("null",)):
                inp = X.image_inputs(c, tables)
                if tables == "quarter":
                    HipOps._check_rope_tables(HipOps.__new__(HipOps), inp.cos, inp.sin, N)     # raises on a layout the kernels cannot read
                    assert set(torch.unique(torch.cat([inp.cos, inp.sin])).tolist()) == {-1.0, 0.0, 1.0}
                    assert not torch.equal(inp.cos[0], inp.cos[1])                         # neighbouring tokens rotate differently
    for N, H in X.CLS_SHAPES:
        assert H in (1, 2, 3, 4, 5, 6) and X.is_square(N)
        for kind in X.KINDS[:3]:
            c = X.cls_case(kind, N, H)
            assert {t // 32 for t in c.tgt.flatten().tolist()} == set(range((N + 31) // 32)) and N - 1 in c.tgt
    assert {6 if H % 6 == 0 else 4 if H % 4 == 0 else 3 if H % 3 == 0 else 2 if H % 2 == 0 else 1 for _, H in X.CLS_SHAPES} == {1, 2, 3, 4, 6}
    for shape in X.QUERY_SHAPES:
        for kind in X.KINDS[:3]:
            c = X.query_case(kind, *shape)
            assert {"one_off", "none"} <= set(c.kinds) and int((c.cnt == 0).sum()) > 0
    for shape in X.CAUSAL_SHAPES:
        X.causal_case(*shape)
    for shape in X.PASSENGER_SHAPES:
        for kind in ("tied_lo", "tied_hi"):
            c = X.passenger_case(kind, *shape)
            assert float(c.dq.abs().max()) > 0 and float(c.dk.abs().max()) > 0 and int((c.cnt == 2).sum()) > 0


# ------------------------------------------------------------------------------------------------ (2) mutations
B_, N_, H_ = 2, 197, 2
CHUNK = 96                                                           # the key chunk of the short-sequence forward


def _old_operands(B=B_, H=H_):
    """The random operands of tests/test_gpu_ops.py::test_attention_forward_short_sequences_against_the_oracle at [2,197,2] or [40,197,12]
    (seed 38, rotary tables of the 14 x 14 grid), which holds o to check(..., 4e-3) against RefOps.
    -> rotated q, k and v [B,H,N,64] float64, the un-rotated k, the tables, RefOps' o."""
    from oracle.eva_ref import rope_tables
    from test_gpu_ops import rnd
    C = H * 64
    qkv = rnd((B * N_, 3 * C), BF, 1.0, seed=38)
    cos, sin = rope_tables(14, 64)
    o = torch.empty(B * N_, C, dtype=BF)
    RefOps().attn_fwd(qkv, cos, sin, o, None, B, N_, H, X.SCALE)
    q, k, v = (X.heads_of(qkv[:, j * C:(j + 1) * C], B, N_, H) for j in range(3))
    rot = lambda t: _rope_rows(t, cos.double(), sin.double()).to(F32).to(BF).double()      # the kernels round the rotated rows to bf16
    return rot(q), rot(k), v, k, (cos, sin), o


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _row_whose_winner_is(c, b, h, key):
    if c.kind == "needle":
        return int(torch.nonzero(c.pi[b, h] == key)[0, 0])
    if c.kind.startswith("tied"):
        return int(torch.nonzero(c.t[b, h] == c.gid[key])[0, 0])
    return 5


def _rot_row(x, cos_row, sin_row):
    """one token rotated by the given table row"""
    p = x.reshape(-1, 2)
    c, s = cos_row.double().reshape(-1, 2), sin_row.double().reshape(-1, 2)
    return torch.stack((p[:, 0] * c[:, 0] - p[:, 1] * s[:, 0], p[:, 1] * c[:, 1] + p[:, 0] * s[:, 1]), -1).flatten()


def _mutated(q, k, v, mutation, row_for, k_raw, tables, b=1, h=1):
    """(o, lse) of the float64 model with one mutation on rotated rows q, k, v [B,H,N,64]; each mutation touches one query row or one key
    token of head (b, h).  row_for(key): the query row to mutate when the mutation concerns `key`; k_raw / tables: the un-rotated keys and
    the tables they are rotated with (table_row_plus_one)."""
    N = q.shape[-2]
    vis = torch.ones(q.shape[0], q.shape[1], N, N, dtype=torch.bool)
    k, v = k.clone(), v.clone()
    kw = dict(chunk=CHUNK)
    if mutation == "drop_last_key":
        vis[b, h, row_for(N - 1), N - 1] = False
    elif mutation == "drop_ragged_key":
        key = (N // 32) * 32 + 1                                    # inside the ragged last 32-key tile
        assert key < N - 1
        vis[b, h, row_for(key), key] = False
    elif mutation == "swap_v_rows":
        v[b, h, [40, 41]] = v[b, h, [41, 40]]                       # two rows of one 32-key tile
    elif mutation == "table_row_plus_one":
        t = 56                                                      # token t's own table row is t - 1 = (3, 13); row t = (4, 0) is its neighbour's
        k[b, h, t] = _rot_row(k_raw[b, h, t], tables[0][t], tables[1][t])
    elif mutation == "skip_rescale":
        kw["skip_rescale"] = (b, h, row_for(N - 2))                 # the winner sits in the last chunk: the maximum rises there
    else:
        raise ValueError(mutation)
    return X.model64(q, k, v, vis, **kw)


IMAGE_MUTATIONS = ["drop_last_key", "drop_ragged_key", "swap_v_rows", "table_row_plus_one", "skip_rescale"]
# The old norm at [2,197,2] accepts the dropped keys (asserted below).  It does reject the other three at this small shape -- a skipped rescale
# moves its row by ~16 %, 5e-3 of a tensor of 788 rows; the swapped V rows and the wrong table row move every row of the head -- and that is
# recorded, not asserted: the same defects in a launch of 40 x 12 heads, the other shape of that test, weigh 11 times less
# (test_at_the_large_shape_the_old_norm_accepts_every_single_row_mutation).
ACCEPTED_BY_OLD_NORM = {"drop_last_key", "drop_ragged_key"}


def _forward_problems(c, o, lse):
    inp = X.image_inputs(c, "null")                                 # the model works in the rotated frame: the frame of NULL tables
    problems = []
    X.check_image_forward(c.kind, inp, X.rows_of(o).to(F32).to(BF), lse.reshape(c.B * c.H, c.N).to(F32), problems)
    return problems


def test_the_unmutated_model_passes_the_new_checks():
    for kind in X.KINDS:
        c = X.image_case(kind, B_, N_, H_)
        o, lse = X.model64(c.q, c.k, c.v, chunk=CHUNK)
        assert not _forward_problems(c, o, lse), kind


@pytest.mark.parametrize("mutation", IMAGE_MUTATIONS)
def test_image_mutations_are_rejected_by_the_new_checks_and_accepted_by_the_old_norm(mutation):
    caught = {}
    quarter = X.quarter_tables(14)
    for kind in X.KINDS:
        c = X.image_case(kind, B_, N_, H_)
        o, lse = _mutated(c.q, c.k, c.v, mutation, lambda key: _row_whose_winner_is(c, 1, 1, key), X.unrotate(c.k, *quarter), quarter)
        caught[kind] = _forward_problems(c, o, lse)
    print(f"{mutation}: " + "; ".join(f"{k}: {v[0] if v else 'passes'}" for k, v in caught.items()))
    must = {"drop_last_key": X.KINDS, "drop_ragged_key": X.KINDS, "swap_v_rows": X.KINDS[:3], "table_row_plus_one": X.KINDS[:3],
            "skip_rescale": X.KINDS[:3]}[mutation]              # (q = 0 and a column sum see neither a rotation nor an order of rows)
    for kind in must:
        assert caught[kind], f"{mutation} passes the {kind} checks"
    # the old check on the old operands: relative L2 over the whole tensor against RefOps, bound 4e-3
    q, k, v, k_raw, tables, o_ref = _old_operands()
    base, _ = X.model64(q, k, v, chunk=CHUNK)
    s = (q[1, 1] @ k[1, 1].T) * X.SCALE
    if mutation == "skip_rescale":                                  # of the rows whose maximum rises in the last chunk, the one with the median rise
        rise = s[:, 2 * CHUNK:].max(-1).values - s[:, :2 * CHUNK].max(-1).values
        rows = torch.nonzero(rise > 0)[:, 0]
        row_for = lambda key: int(rows[rise[rows].sort().indices[len(rows) // 2]])
    else:                                                           # the row that gives the dropped key the median probability of all rows
        row_for = lambda key: int(torch.softmax(s, -1)[:, key].sort().indices[N_ // 2])
    mut, _ = _mutated(q, k, v, mutation, row_for, k_raw, tables)
    r0, r1 = _rel(X.rows_of(base).to(F32).to(BF), o_ref), _rel(X.rows_of(mut).to(F32).to(BF), o_ref)
    moved = (mut - base).norm(dim=-1) / base.norm(dim=-1)
    print(f"{mutation} on random operands [2,197,2]: rel-L2 against RefOps {r0:.3e} -> {r1:.3e} (bound 4e-3); {int((moved > 1e-9).sum())} rows moved, "
          f"worst row by {float(moved.max()):.1%}")
    assert float(moved.max()) > 1e-3, "the mutation did not reach the random operands"
    if mutation in ACCEPTED_BY_OLD_NORM:
        assert int((moved > 1e-9).sum()) == 1
        assert r1 <= 4e-3, f"{mutation}: the old norm rejects it ({r1:.3e}); this test records that it does not"


def test_at_the_large_shape_the_old_norm_accepts_every_single_row_mutation():
    """[40,197,12], the large shape of test_attention_forward_short_sequences_against_the_oracle: a mutation of one query row of one head out
    of 480, and a wrong table row for one token of one head, leave the relative L2 of o against RefOps under 4e-3."""
    q, k, v, k_raw, tables, o_ref = _old_operands(40, 12)
    base, _ = X.model64(q, k, v, chunk=CHUNK)
    r0 = _rel(X.rows_of(base).to(F32).to(BF), o_ref)
    s = (q[1, 1] @ k[1, 1].T) * X.SCALE
    rise = s[:, 2 * CHUNK:].max(-1).values - s[:, :2 * CHUNK].max(-1).values
    rows = torch.nonzero(rise > 0)[:, 0]
    for mutation in IMAGE_MUTATIONS:
        if mutation == "skip_rescale":
            row_for = lambda key: int(rows[rise[rows].sort().indices[len(rows) // 2]])
        else:
            row_for = lambda key: int(torch.softmax(s, -1)[:, key].sort().indices[N_ // 2])
        mut, _ = _mutated(q, k, v, mutation, row_for, k_raw, tables)
        r1 = _rel(X.rows_of(mut).to(F32).to(BF), o_ref)
        moved = (mut - base).norm(dim=-1) / base.norm(dim=-1)
        print(f"{mutation} on random operands [40,197,12]: rel-L2 against RefOps {r0:.3e} -> {r1:.3e} (bound 4e-3); {int((moved > 1e-9).sum())} rows "
              f"moved, worst row by {float(moved.max()):.1%}")
        assert float(moved.max()) > 1e-2, mutation
        if mutation in ("drop_last_key", "drop_ragged_key", "skip_rescale"):
            assert int((moved > 1e-9).sum()) == 1
        if mutation != "swap_v_rows":                               # two V rows swapped for EVERY row of a head still show: 6.0e-3
            assert r1 <= 4e-3, mutation


def test_an_ignored_allow_bit_is_rejected():
    for kind in ("needle", "tied_lo"):
        c = X.query_case(kind, 4, 3, 65, 4)
        g = c.kinds.index("one_off")
        b, r = divmod(g, c.Q)
        hidden = torch.nonzero(~c.vis[b, 0, r] & (c.P[b, 0, r] == 0))[:, 0]
        # the hidden key that matters for head 0: the needle itself / the hidden partner
        S = (c.q[b, 0, r] @ c.k[b, 0].T)
        key = int(hidden[torch.argmax(S[hidden])])
        vis = c.vis.clone()
        vis[b, 0, r, key] = True
        for mutate in (False, True):
            o, lse = X.model64(c.q, c.k, c.v, vis if mutate else c.vis)
            problems = []
            X.check_exact("o", X.rows_of(o).to(F32).to(BF), X.rows_of(c.o), problems)
            X.check_lse("lse", lse.to(F32), c.lse, X.LSE_ULPS_QUERY, problems)
            print(f"allow bit of row {g}, key {key} ignored={mutate} ({kind}): {problems or 'passes'}")
            assert bool(problems) == mutate


def test_a_causal_row_that_sees_a_future_key_is_rejected():
    c = X.causal_case(2, 77, 2)
    b, h = 1, 1
    i = int(torch.nonzero(c.future[b, h])[3, 0])
    S = c.q[b, h, i] @ c.k[b, h].T
    a = int(torch.argmax(S))
    assert a > i                                                    # the row's best key lies in the future
    for mutate in (False, True):
        vis = c.vis.expand(c.B, c.H, c.L, c.L).clone()
        if mutate:
            vis[b, h, i, a] = True
        o, _ = X.model64(c.q, c.k, c.v, vis)
        problems = []
        X.check_exact("o", X.rows_of(o).to(F32).to(BF), X.rows_of(c.o), problems)
        print(f"causal row {i} sees key {a}: {mutate}: {problems or 'passes'}")
        assert bool(problems) == mutate
