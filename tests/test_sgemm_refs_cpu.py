"""CPU proofs behind tests/test_gpu_stream_gemm.py (tests/sgemm_refs.py): each fp64 restatement is a
direct torch fp64 evaluation written the reference project's way (F.linear, F.gelu, F.layer_norm,
torch.cat) — to fp64 accuracy where no polynomial GELU is involved, within the polynomial's pinned
distance from F.gelu carried to the output where one is; gelu_poly64 is within common.h's 2.6e-5 of
the exact-erf GELU; the dispatch restatement names 25 + 5 instantiations and the shape tables reach
every one of them at the row, pair and rotation edges they are there for; the bounds have teeth
(thirteen single-fault mutations of the reference each leave their bound); and on the MLP / AFG
inputs the flagged-rounding allowance stays below the output's half ulp."""
import math

import pytest
import torch
import torch.nn.functional as F

import sgemm_refs as R

F64, BF16 = R.F64, R.BF16
TOL = dict(rtol=1e-11, atol=1e-12)
FIT = R.C["gelu_fit"]


def _rank(M, period, c):
    r1, r2 = R.rank_scalars(M, period)
    return (r1, r2, period, c.c1, c.c2)


def _rank_term(rank, M):
    if rank is None:
        return 0.0
    r1, r2, period, c1, c2 = rank
    ri = torch.arange(M) % period
    return r1.double()[ri, None] * c1.double() + r2.double()[ri, None] * c2.double()


# ------------------------------------------------- a. references == torch fp64 --
@pytest.mark.parametrize("rank", [False, True])
@pytest.mark.parametrize("D,N", [(128, 192), (384, 64)])
def test_act_matches_torch(D, N, rank):
    M = 45
    c = R.base(D, N, 64)
    rk = _rank(M, 33, c) if rank else None
    z = F.linear(c.x[:M].double(), c.w.double(), c.b.double()) + _rank_term(rk, M)
    torch.testing.assert_close(R.act(c.x[:M], c.w, c.b, "none", rk).out, z, **TOL)
    got = R.act(c.x[:M], c.w, c.b, "gelu", rk).out
    assert float((got - F.gelu(z)).abs().max()) <= FIT


@pytest.mark.parametrize("rank", [False, True])
def test_ln_matches_torch(rank):
    D, M = 128, 45
    c = R.base(D, D, 64)
    g, be = R.ln_vecs(D)
    rk = _rank(M, 7, c) if rank else None
    x = c.x[:M].double()
    z = F.linear(x, c.w.double(), c.b.double()) + _rank_term(rk, M)
    ref = F.layer_norm(F.leaky_relu(z, R.SLOPE) + x, (D,), g.double(), be.double(), R.f32(R.EPS))
    torch.testing.assert_close(R.ln(c.x[:M], c.w, c.b, rk, g, be, R.SLOPE, R.f32(R.EPS)).out, ref, **TOL)


def test_head2_matches_torch():
    D, M = 128, 45
    c = R.base(D, 4 * D, 64)
    w_out, b_out = R.head_vecs(D)
    h = F.gelu(F.linear(c.x[:M].double(), c.w.double(), c.b.double()))
    logits = F.linear(h, w_out.double(), b_out.double())
    r = R.head2(c.x[:M], c.w, c.b, w_out, b_out)
    carried = FIT * float(w_out.abs().sum(-1).max())
    assert float((r.logits - logits).abs().max()) <= carried
    assert float((r.probs - torch.softmax(logits, -1)).abs().max()) <= carried / 2     # |dp| <= p (1 - p) 2 dl


def test_cat_matches_torch():
    M, N, period = 45, 64, 33
    c = R.base(768, N, 64)
    g = R._gen(11)
    x2 = R._bf(torch.randn(M, 384, generator=g))
    g2 = R._bf(torch.rand(period, 384, generator=g))
    q = c.x[:M, :384]
    prod = (x2.float() * g2[torch.arange(M) % period].float()).to(BF16)
    ref = F.gelu(F.linear(torch.cat([q.double(), prod.double()], -1), c.w.double(), c.b.double()))
    assert float((R.cat(q, x2, g2, period, c.w, c.b).out - ref).abs().max()) <= FIT


@pytest.mark.parametrize("epi2", [0, 1])
def test_mlp_matches_torch(epi2):
    """The hidden's bf16 rounding taken from the restatement (a polynomial GELU and an exact one
    round differently): what is compared is the second projection and EPI2, and the hidden itself."""
    M = 45
    c = R.mlp_base()
    rk = (*R.rank_scalars(M, 33), 33, c.c1, c.c2)
    parts = R.mlp_parts(c, epi2)
    z = F.linear(c.x[:M].double(), c.w1.double(), c.b1.double()) + _rank_term(rk, M)
    h64 = R.gelu_poly64(z)
    assert float((h64 - F.gelu(z)).abs().max()) <= FIT
    y2 = F.linear(R.rne_bf16(h64), c.w2.double(), c.b2.double())
    ref = torch.sigmoid(y2) if epi2 == 0 else F.layer_norm(y2, (c.D,), c.g.double(), c.be.double(), R.f32(R.EPS))
    torch.testing.assert_close(R.mlp(c.x[:M], c.w1, c.w2, parts, epi2, rk).out, ref, **TOL)


def test_afgate_input_matches_torch():
    """The gate (exact-erf GELUs, F.layer_norm) to fp64 accuracy, then the MLP above on its rounding."""
    M = 40
    ag = R.afgate_weights()
    af, afp = R.afgate_inputs(M)
    cc = torch.stack([af, afp], -1).double()
    w = [t.double() for t in ag]
    gate = torch.sigmoid(F.linear(F.gelu(F.linear(cc, w[0], w[1])), w[2], w[3]))
    enc = F.gelu(F.layer_norm(F.linear(cc, w[4], w[5]), (384,), w[6], w[7], 1e-5))
    v = af.double()[:, None] + R.RES_SCALE * gate * enc
    torch.testing.assert_close(R.FR.af_gate(af, afp, ag, R.RES_SCALE), v, **TOL)
    c = R.mlp_base()
    o = R.afgate_mlp(af, afp, ag, R.RES_SCALE, c.w1, c.w2, c.b1, c.b2)
    h = R.rne_bf16(R.gelu_poly64(F.linear(R.rne_bf16(v), c.w1.double(), c.b1.double())))
    torch.testing.assert_close(o.out, torch.sigmoid(F.linear(h, c.w2.double(), c.b2.double())), **TOL)


# ----------------------------------------------------------- b. GELU distance --
def test_gelu_poly_distance_from_exact_erf():
    """Dense grid over [-12, 12] plus every bf16 value there: common.h's 2.6e-5."""
    grid = torch.linspace(-12, 12, 2_400_001, dtype=F64)
    bits = torch.arange(0, 0x10000, dtype=torch.int32).to(torch.int16).view(BF16).double()
    bfv = bits[torch.isfinite(bits) & (bits.abs() <= 12)]
    x = torch.cat([grid, bfv])
    d = (R.gelu_poly64(x) - R.gelu_erf64(x)).abs()
    i = int(d.argmax())
    print(f"max |gelu_poly64 - gelu_erf64| = {float(d[i]):.4e} at x = {float(x[i]):.4f}")
    assert float(d[i]) <= FIT


def test_gelu_err_covers_an_f32_evaluation():
    """gelu_bf16's own sequence in torch f32 (exact exp2 / reciprocal rounded once) stays inside
    gelu_err with dz = 0: the evaluation terms are not under-counted."""
    z = torch.cat([torch.linspace(-10, 10, 400001, dtype=F64), R.gelu_domain_input().double().reshape(-1)])
    z = z.float()
    L2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
    xc = z.clamp(-8, 8)
    x2 = xc * xc
    c2, c1, c0 = [torch.tensor(v, dtype=torch.float32) * L2E for v in (7.03033577e-4, -7.40112920e-2, -1.59501577)]
    e = xc * (x2 * (x2 * c2 + c1) + c0)
    y32 = z * (1.0 / (1.0 + torch.exp2(e)))
    zz = z.double()
    err = (y32.double() - R.gelu_poly64(zz)).abs()
    bound = R.gelu_err(zz, torch.zeros_like(zz))
    assert bool((err <= bound + 2.0 ** -149).all()), float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------ c. teeth --
def _exceeds(mut, true):
    return R.ratio(mut.out, true.out, true.bound) > 1.0


def _act_teeth_inputs(D, N, M, a):
    c = R.base(D, N, 1024)
    return c, (lambda w=c.w, b=c.b, rk=None, x=c.x[:M]: R.act(x, w, b, a, rk))


def _drop_kstep(w, tile=1, step=2):
    w = w.clone()
    w[32 * tile:32 * tile + 32, 16 * step:16 * step + 16] = 0
    return w


def _rank_teeth(f, M, c, rows=R.ROWS4):
    """The three rank faults of a form f(rk=...) at the periods 33, M and M + 7 of the tables: the
    scalars read at (m + 1) % period, r1 and r2 exchanged and, where the period is above the
    workgroup height (M > rows), the period taken as that height."""
    assert M > rows
    for period in (33, M, M + 7):
        r1, r2 = R.rank_scalars(M, period)
        rk = lambda a1=r1, a2=r2, p=period: (a1, a2, p, c.c1, c.c2)
        true = f(rk=rk())
        assert _exceeds(f(rk=rk(torch.roll(r1, -1), torch.roll(r2, -1))), true), period
        assert _exceeds(f(rk=rk(r2, r1)), true), period
        if period > rows:
            assert _exceeds(f(rk=rk(p=rows)), true), period


@pytest.mark.parametrize("D,a", [(D, a) for D in R.DS for a in ("none", "gelu")] + [(768, "gelu")])
def test_teeth_act(D, a):
    """ACT (and the K = 768 form): a k-step left out of one tile, the bias of the next quad and of
    the next pair; with rank terms: the scalars at (m + 1) % period, r1 and r2 exchanged, the period
    taken as the workgroup height."""
    rows = 128
    M, N = rows + 33, 192
    c, f = _act_teeth_inputs(D, N, M, a)
    true = f()
    assert _exceeds(f(w=_drop_kstep(c.w)), true)
    assert _exceeds(f(b=torch.roll(c.b, -4)), true)
    assert _exceeds(f(b=torch.roll(c.b, -64)), true)
    if D == 768:
        return
    _rank_teeth(f, M, c)


@pytest.mark.parametrize("rank", [False, True])
@pytest.mark.parametrize("D", R.DS)
def test_teeth_ln(D, rank):
    """LN: a dropped k-step, the bias, g and be of the next quad / pair, the residual left out and
    added late, eps x 10 on the low-variance case; with rank terms the three rank faults at periods
    33, M and M + 7 (the period taken as the workgroup height at the two above it)."""
    M = 129
    c = R.base(D, D, 1024)
    g, be = R.ln_vecs(D)
    eps = R.f32(R.EPS)
    r1, r2 = R.rank_scalars(M, 33)
    rk = (r1, r2, 33, c.c1, c.c2) if rank else None
    f = lambda w=c.w, b=c.b, rk=rk, g=g, be=be, eps=eps, mut=None: R.ln(c.x[:M], w, b, rk, g, be, R.SLOPE, eps, None, mut)
    true = f()
    assert _exceeds(f(w=_drop_kstep(c.w)), true)
    assert _exceeds(f(b=torch.roll(c.b, -4)), true)
    assert _exceeds(f(b=torch.roll(c.b, -64)), true)
    assert _exceeds(f(mut="no_resid"), true)
    assert _exceeds(f(mut="round_first"), true)
    assert _exceeds(f(g=torch.roll(g, -64), be=torch.roll(be, -64)), true)
    if rank:
        _rank_teeth(f, M, c)
    lv = R.low_variance_case(D, M)
    fl = lambda e: R.ln(lv.x, lv.w, lv.b, None, lv.g, lv.be, R.SLOPE, e)
    assert _exceeds(fl(R.f32(10 * R.EPS)), fl(eps))


@pytest.mark.parametrize("D", R.DS)
def test_teeth_head2(D):
    M = 129
    c = R.base(D, 4 * D, 4096)
    w_out, b_out = R.head_vecs(D)
    f = lambda w=c.w, b=c.b, wo=w_out: R.head2(c.x[:M], w, b, wo, b_out)
    true = f()
    for mut in (f(w=_drop_kstep(c.w)), f(b=torch.roll(c.b, -4)), f(b=torch.roll(c.b, -64)),
                f(wo=torch.roll(w_out, -64, 1))):
        assert R.ratio(mut.logits, true.logits, true.bound_logits) > 1.0
        assert R.ratio(mut.probs, true.probs, true.bound_probs) > 1.0


def test_teeth_cat():
    M, N = 129, 192
    c = R.base(768, N, 1024)
    g = R._gen(12)
    x2 = R._bf(torch.randn(M, 384, generator=g))
    for period in (33, M, M + 5):
        g2 = R._bf(torch.rand(period, 384, generator=g))
        q = c.x[:M, :384]
        true = R.cat(q, x2, g2, period, c.w, c.b)
        assert _exceeds(R.cat(q, x2, torch.roll(g2, -1, 0), period, c.w, c.b), true)
        assert _exceeds(R.act(R.cat_input(q, x2, g2, period, swap=True), c.w, c.b, "gelu"), true)
        assert _exceeds(R.cat(q, x2, g2, period, _drop_kstep(c.w, 1, 30), c.b), true)
        # the un-rounded product is NOT what the kernel multiplies: the rounding is part of the operation
        ri = torch.arange(M) % period
        raw = torch.cat([q.double(), x2.double() * g2.double()[ri]], -1)
        assert _exceeds(R.act(raw, c.w, c.b, "gelu"), true)


@pytest.mark.parametrize("epi2", [0, 1])
@pytest.mark.parametrize("rank", [False, True])
def test_teeth_mlp(rank, epi2):
    """MLP: one k-step (16 input columns) left out of one 32-unit tile of W1, b1 of the next quad /
    pair, the hidden pair P against W2's columns of pair P + 1, g and be of the next pair; with rank
    terms the three rank faults at periods 33, M and M + 7."""
    M = 129
    c = R.mlp_base()
    parts = R.mlp_parts(c, epi2)
    r1, r2 = R.rank_scalars(M, 33)
    rk = (r1, r2, 33, c.c1, c.c2) if rank else None
    f = lambda w1=c.w1, w2=c.w2, parts=parts, rk=rk: R.mlp(c.x[:M], w1, w2, parts, epi2, rk)
    true = f()
    assert _exceeds(f(w1=_drop_kstep(c.w1)), true)
    assert _exceeds(f(parts=dict(parts, b1=torch.roll(c.b1, -4))), true)
    assert _exceeds(f(parts=dict(parts, b1=torch.roll(c.b1, -64))), true)
    assert _exceeds(f(w2=torch.roll(c.w2, -64, 1)), true)
    if rank:
        _rank_teeth(f, M, c)
    if epi2 == 1:
        assert _exceeds(f(parts=dict(parts, g=torch.roll(c.g, -64), be=torch.roll(c.be, -64))), true)


def test_near_midpoint_and_exact_cases():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-6, 1.0 + 2.0 ** -7, 0.0, 1.0 + 1e-7], dtype=F64)
    d = torch.full_like(v, 2e-6)
    assert R.near_midpoint(v, d).tolist() == [True, True, False, False, False]
    c = R.exact_case(128, 130, 192, 33)
    ref = R.act(c.x, c.w, c.b, "none", c.rank).out
    assert torch.equal(ref, c.out.double())
    x = R.gelu_domain_input()
    assert x.shape[1] == 128 and int((x != 0).sum()) == 2 * (130 * 128 + 1)
    assert bool((x.float().abs()[x != 0] >= 2.0 ** -126).all())


# ------------------------------------------------------- d. table properties --
def test_dispatch_names():
    assert len(R.SG_INSTANCES) == 25 and len(R.MLP_INSTANCES) == 5 and len(set(R.ALL_INSTANCES)) == 30
    assert R.dispatch(384, "act", "none", False) == (R.sg_name(384, "act", "none", False, 8), 256)
    assert R.dispatch(384, "act", "gelu", False, waves4=True) == (R.sg_name(384, "act", "gelu", False, 4), 128)
    assert R.dispatch(384, "act", "gelu", True)[1] == 128 and R.dispatch(256, "act", "none", False)[1] == 128
    for bad in ((768, "act", "none", False), (768, "ln", "lrelu", False), (128, "head2", "none", False),
                (128, "ln", "gelu", False), (128, "act", "lrelu", False), (64, "act", "none", False)):
        with pytest.raises(ValueError):
            R.dispatch(*bad)


def test_tables_reach_every_instantiation_and_edge():
    got = R.all_table_instances()
    assert set(got) == set(R.ALL_INSTANCES), set(R.ALL_INSTANCES) ^ set(got)
    assert all(n >= 1 for n in got.values())

    def edges(rows_set, rows, nps):
        s = set(rows_set)
        return {rows - 1, rows, rows + 1} <= s and any(np_ * rows + 1 in s for np_ in nps)
    for D, a, r, w4 in R.act_forms():
        rows = R.dispatch(D, "act", a, r, w4)[1]
        nps = [n // 64 for n in R.act_n(D)]
        assert {1, 2, 3} <= set(nps) and any(p > 3 and p % 2 for p in nps)
        assert edges(R.act_rows(rows), rows, nps), (D, a, r, w4)
        if r:
            for M in R.act_rows(rows):
                assert {1, 33, rows, M, M + 7} == set(R.periods(M, rows))
    nps = [n // 64 for n in R.K768_N]
    assert {1, 3} <= set(nps) and edges(R.K768_M, 128, nps)
    assert {127, 128, 129} <= set(R.LN_M)                   # LN does not rotate: no block-NP case
    for D in R.DS:
        assert edges(R.head_rows(D), 128, [4 * D // 64])
    assert edges(R.MLP_M, 128, [1536 // 64])


# ----------------------------------------------------------- e. flagged share --
def test_flagged_allowance_stays_below_the_half_ulp():
    """On the table's MLP and AFG inputs the flagged term of the bound is below the output's half
    ulp for at least 95 % of the output elements (so the allowance cannot swallow the teeth)."""
    c = R.mlp_base()
    outs = []
    for rank in (False, True):
        for epi2 in (0, 1):
            for M, p in ((129, 33 if rank else None), (R.MLP_M[-1], R.MLP_M[-1] + 7 if rank else None)):
                if M > 129 and (rank, epi2) != (True, 1):
                    continue                                # one full-height case; the rows are the same inputs
                rk = (*R.rank_scalars(M, p), p, c.c1, c.c2) if rank else None
                outs.append((f"mlp rank={rank} epi2={epi2} M={M}", R.mlp(c.x[:M], c.w1, c.w2, R.mlp_parts(c, epi2), epi2, rk)))
    for kind, M, cond in (("rand", 129, False), ("pairs", len(R.AF_PAIRS), False), ("cond", 130, True)):
        af, afp = R.afgate_inputs(M, kind)
        outs.append((f"afg {kind}", R.afgate_mlp(af, afp, R.afgate_weights(conditioning=cond), R.RES_SCALE, c.w1, c.w2, c.b1, c.b2)))
    for name, o in outs:
        ok = (o.flag_term < o.half_ulp).to(F64)
        if name == "afg cond":
            # the af = 0.3 rows (even) are the point of the case: the prologue's closed-form variance
            # cancels there (terms of 0.05 against a variance of 1e-6 under eps = 1e-5), its derived
            # error is 1e-4 of x and a tenth of those inputs are flagged; the allowance then exceeds
            # the half ulp by construction, and the GPU case measures that the kernel loses no more
            # than the form implies.  The condition holds on the ordinary rows.
            wide = (o.bound / o.half_ulp)[::2]
            print(f"{name}, af = 0.3 rows: flag term < half ulp on {float(ok[::2].mean()):.4f} of the outputs; "
                  f"bound / half ulp median {float(wide.median()):.2f}, max {float(wide.max()):.2f}; "
                  f"ordinary rows median {float((o.bound / o.half_ulp)[1::2].median()):.2f}")
            ok = ok[1::2]
        share = float(ok.mean())
        worst = float((o.flag_term / o.half_ulp).max())
        print(f"{name}: flagged hidden {o.flag_share:.4f}, flag term < half ulp on {share:.4f} of the outputs (worst {worst:.3f})"
              + (f", flagged inputs {o.x_flag_share:.4f}" if hasattr(o, "x_flag_share") else ""))
        assert share >= 0.95, name
