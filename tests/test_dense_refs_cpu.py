"""CPU proofs behind tests/test_gpu_dense_gemm.py (tests/dense_refs.py): the fp64 restatement of
snvrag_linear_ex agrees with torch.nn.functional in fp64 (linear, gelu, leaky_relu, sigmoid,
layer_norm; fold_layernorm + the row-norm form == LN-then-linear); an f32 evaluation in the kernels'
order (K-tile after K-tile, the epilogue's operations one by one, one-pass row-norm statistics) stays
inside the derived bounds for both input families and every epilogue; fourteen single-fault mutations
each leave their bound (or change bits of the exact family); the shape tables reach all 36
instantiations and every edge they are there for; the restated XCD remap is a permutation and the
restated rows_pick_nw agrees with kernels.stat_tiles."""
import math

import pytest
import torch
import torch.nn.functional as F

import dense_refs as D
import sgemm_refs as S

F64, F32, BF16 = D.F64, D.F32, D.BF16
TOL = dict(rtol=1e-11, atol=1e-12)
FIT = S.C["gelu_fit"]


def _rank_term(e, M):
    if e.row1 is None:
        return 0.0
    ri = D.row_index(M, e.period)
    return (e.row1.double()[ri * e.s1, None] * e.col1.double() + e.row2.double()[ri * e.s2, None] * e.col2.double())


def _torch_act(code, z, slope):
    return (z, F.gelu(z), F.leaky_relu(z, slope), torch.sigmoid(z))[code]


# ------------------------------------------------- a. references == torch fp64 --
@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("tin,tout", D.PAIRS)
def test_linear_matches_torch(tin, tout, i):
    M, N, K = 70, 128, D.ROWS_K[tin][1]
    c = D.base(tin, K, N)
    form, _ = D.form_of(i, M)
    e = D.make_spec(tout, N, M, form, 37 if form["rank"] else 0)
    z = F.linear(c.x[:M].double(), c.w.double(), None if e.bias is None else e.bias.double()) + _rank_term(e, M)
    want = _torch_act(e.act, z, e.slope) + (0.0 if e.resid is None else e.resid.double())
    got = D.linear(c.x[:M], c.w, e, tin, tout).out
    poly = e.act == D.ACT_GELU and tout == BF16
    assert float((got - want).abs().max()) <= (FIT if poly else 1e-11)
    tile = D.linear(c.x[:M], c.w, e, tin, tout, kernel="tile").out            # exact-erf for both output types
    torch.testing.assert_close(tile, want, **TOL)


@pytest.mark.parametrize("lf", range(len(D.LN_FORMS)))
def test_ln_tail_matches_torch(lf):
    M, N, K, tout = 70, 128, 64, BF16
    c = D.base(BF16, K, N)
    e = D.make_spec(tout, N, M, D.FORMS[2], 37, D.LN_FORMS[lf])
    v = F.leaky_relu(F.linear(c.x[:M].double(), c.w.double()) + _rank_term(e, M), D.SLOPE)
    y = F.layer_norm(v, (N,), e.ln_g.double(), e.ln_b.double(), e.ln_eps)
    y = (y, F.gelu(y), F.relu(y), torch.sigmoid(y))[e.ln_act]
    if e.post_base is not None:
        w = 1.0
        if e.post_maf:
            af = e.post_af.double()[D.row_index(M, e.post_af_period)]
            w = torch.clamp(torch.log1p(1.0 / (torch.minimum(af, 1 - af) + D.MAF_EPS)), max=3.0)[:, None]
        y = e.post_base.double() + e.post_scale * y * w
    torch.testing.assert_close(D.linear(c.x[:M], c.w, e, BF16, tout).out, y, **TOL)


@pytest.mark.parametrize("parts", D.RN_PARTS)
def test_fold_layernorm_rownorm_is_ln_then_linear(parts):
    from src import kernels
    M, N, K = 33, 64, 96
    g = S._gen(parts, 41)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.3
    w, b = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    gam, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    wg, bg, c1 = kernels.fold_layernorm(w, b, gam, beta, F32)
    rn = D.SimpleNamespace(stats=D.row_partials(x, parts), n_parts=parts, dim=K, eps=S.f32(D.EPS), c1=c1)
    ref = D.linear(x, wg, D.spec(bias=bg, rownorm=rn), F32, F32)
    want = F.linear(F.layer_norm(x.double(), (K,), gam.double(), beta.double(), S.f32(D.EPS)), w.double(), b.double())
    assert D.ratio(ref.out, want, ref.bound + 1e-5) <= 1.0      # wg, bg, c1 and the partials are f32 roundings
    assert float(ref.bound.max()) < 1e-3


def test_stats_are_tile_sums():
    M, N, K = 5, 1152, 64
    c = D.base(BF16, K, N)
    r = D.linear(c.x[:M], c.w, D.spec(stats=True), BF16, BF16, bn=384)
    v = F.linear(c.x[:M].double(), c.w.double())
    for t in range(3):
        torch.testing.assert_close(r.stats[t, :, 0], v[:, 384 * t:384 * (t + 1)].sum(-1), **TOL)
        torch.testing.assert_close(r.stats[t, :, 1], (v[:, 384 * t:384 * (t + 1)] ** 2).sum(-1), **TOL)


# ------------------------------------- b. an f32 evaluation stays in the bounds --
def _f(v):
    return torch.tensor(v, dtype=F32)


def _gelu32(z, kind):
    if kind == "poly":
        L2E = _f(1.4426950408889634)
        xc = z.clamp(-8, 8)
        x2 = xc * xc
        c2, c1, c0 = [_f(v) * L2E for v in (7.03033577e-4, -7.40112920e-2, -1.59501577)]
        return z * (1.0 / (1.0 + torch.exp2(xc * (x2 * (x2 * c2 + c1) + c0))))
    ax = z.abs() * _f(0.70710678118654752)
    t = 1.0 / (_f(0.3275911) * ax + 1.0)
    q = t * _f(1.061405429) + _f(-1.453152027)
    for cf in (1.421413741, -0.284496736, 0.254829592):
        q = t * q + _f(cf)
    q = t * q * torch.exp2(ax * ax * _f(-1.4426950408889634))
    return z * torch.where(z >= 0, 1.0 - 0.5 * q, 0.5 * q)


def _act32(code, z, slope, kind):
    if code == D.ACT_GELU:
        return _gelu32(z, kind)
    if code == D.ACT_LRELU:
        return torch.where(z >= 0, z, z * _f(slope))
    if code == D.ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-z))
    return z


def eval32(x, w, e, tin, tout, kernel="rows", bn=None):
    """The kernels' order of operations in torch f32: (out rounded to tout, stats or None)."""
    M, K = x.shape
    t = D.ept(tin)
    acc = torch.zeros(M, w.shape[0], dtype=F32)
    for k0 in range(0, K, t):
        acc = acc + x[:, k0:k0 + t].float() @ w[:, k0:k0 + t].float().T
    if e.rownorm is not None:
        rn = e.rownorm
        s, ss = torch.zeros(M), torch.zeros(M)
        for p in range(rn.n_parts):
            s, ss = s + rn.stats[p, :M, 0], ss + rn.stats[p, :M, 1]
        mean = s / _f(float(rn.dim))
        var = (ss / _f(float(rn.dim)) - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + _f(rn.eps))
        acc = rstd[:, None] * acc + (-rstd * mean)[:, None] * rn.c1
    if e.bias is not None:
        acc = acc + e.bias
    ri = D.row_index(M, e.period)
    for row, s, col in ((e.row1, e.s1, e.col1), (e.row2, e.s2, e.col2)):
        if row is not None:
            acc = acc + row[ri * s, None] * col
    v = _act32(e.act, acc, e.slope, D.gelu_kind(kernel, tout))
    if e.resid is not None:
        v = v + e.resid.float()
    out = v
    if e.ln_g is not None:
        N = v.shape[1]
        mean = v.sum(-1, keepdim=True) / N
        d = v - mean
        rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / N + _f(e.ln_eps))
        out = _act32(e.ln_act, d * rstd * e.ln_g + e.ln_b, 0.0, "erf")
        if e.post_base is not None:
            wgt = torch.ones(M, 1)
            if e.post_maf:
                af = e.post_af[D.row_index(M, e.post_af_period)]
                wgt = torch.log1p(1.0 / (torch.minimum(af, 1.0 - af) + _f(1e-6))).clamp_max(3.0)[:, None]
            out = e.post_base.float() + _f(e.post_scale) * (out * wgt)
    st = None
    if e.stats:
        vt = v.view(M, -1, bn)
        st = torch.stack([vt.sum(-1).T, (vt * vt).sum(-1).T], -1)
    return out.to(tout), st


def _assert_inside(o32, st32, ref, what):
    r = D.ratio(o32, ref.out, ref.bound)
    print(f"{what}: f32 evaluation max err/bound {r:.3f}")
    assert r <= 1.0, what
    if st32 is not None:
        rs = D.ratio(st32, ref.stats, ref.stats_bound)
        print(f"{what}: stats {rs:.3f}")
        assert rs <= 1.0, what


@pytest.mark.parametrize("tin,tout", D.PAIRS)
def test_bounds_admit_f32_evaluation_plain(tin, tout):
    """Every form x period of the sweeps, the row-panel and the 128-tile GELU choice, stats."""
    for nw, M in ((6, 129), (1, 65)):
        N, K = D.ROWS_N[nw][1], D.ROWS_K[tin][2]
        c = D.base(tin, K, N)
        for i in range(30):
            form, period = D.form_of(i, M)
            for kernel in ("rows", "tile"):
                e = D.make_spec(tout, N, M, form, period, stats=kernel == "rows")
                ref = D.linear(c.x[:M], c.w, e, tin, tout, kernel, 64 * nw, D.base_gemm(tin, K, N))
                _assert_inside(*eval32(c.x[:M], c.w, e, tin, tout, kernel, 64 * nw), ref, f"{kernel} nw={nw} form {i}")
    K = D.TILE_K[tin][1]                                     # a K tail
    c = D.base(tin, K, 72)
    e = D.make_spec(tout, 72, 129, D.FORMS[1], 37)
    _assert_inside(*eval32(c.x[:129], c.w, e, tin, tout, "tile"), D.linear(c.x[:129], c.w, e, tin, tout, "tile"), "tile tail")


@pytest.mark.parametrize("tin,tout", D.PAIRS)
def test_bounds_admit_f32_evaluation_ln_and_rownorm(tin, tout):
    M = 129
    for nw in (6, 2):
        N, K = 64 * nw, D.ROWS_K[tin][1]
        c = D.base(tin, K, N)
        for i in range(30):
            form, period = D.form_of(i, M)
            e = D.make_spec(tout, N, M, form, period, D.LN_FORMS[i % 5])
            _assert_inside(*eval32(c.x[:M], c.w, e, tin, tout), D.linear(c.x[:M], c.w, e, tin, tout), f"LN nw={nw} case {i}")
    N, K = 320, D.ROWS_K[tin][2]
    c = D.base(tin, K, N)
    for i, parts in enumerate(D.RN_PARTS * 2):
        form, period = D.form_of(i, M)
        e = D.make_spec(tout, N, M, form, period)
        e.rownorm = D.make_rownorm(tin, tout, K, N, M, parts)
        _assert_inside(*eval32(c.x[:M], c.w, e, tin, tout), D.linear(c.x[:M], c.w, e, tin, tout), f"row-norm parts={parts} form {i}")


@pytest.mark.parametrize("tin,tout", D.PAIRS)
def test_exact_family_is_exact(tin, tout):
    """linear() gives the exact answers, its dense bound aside, and an f32 evaluation gives their bits."""
    M, N, K = 130, 128, D.ROWS_K[tin][2]
    for kw in (dict(period=37, strides=(2, 1), resid=True, stats_bn=128), dict(strides=None, rownorm=5), dict(strides=None, rownorm=2),
               dict(period=M + 7, strides=(1, 2))):
        c = D.exact_case(tin, tout, K, M, N, **kw)
        ref = D.linear(c.x, c.w, c.e, tin, tout, bn=128)
        assert torch.equal(ref.out, c.out.double())
        o32, st32 = eval32(c.x, c.w, c.e, tin, tout, bn=128)
        assert torch.equal(o32.double(), c.out.double())
        if st32 is not None:
            assert torch.equal(st32, c.stats) and torch.equal(ref.stats, c.stats.double())


# ------------------------------------------------------------------ c. teeth --
def _case(tin=BF16, tout=BF16, M=129, N=384, K=192, form=1, period=37, **kw):
    c = D.base(tin, K, N)
    e = D.make_spec(tout, N, M, D.FORMS[form], period, **kw)
    return c.x[:M], c.w, e


def _leaves(mut, ref, what):
    r = D.ratio(mut, ref.out, ref.bound)
    print(f"{what}: mutated reference at {r:.3g} of the bound")
    assert r > 1.0, what


def test_teeth_dropped_k_step():
    x, w, e = _case()
    x2 = x.clone()
    x2[:, 96:128] = 0                                       # the second MFMA K-step of K-tile 1
    _leaves(D.linear(x2, w, e).out, D.linear(x, w, e), "dropped K-step")
    c = D.exact_case(BF16, BF16, 192, 129, 384, period=37)
    x2 = c.x.clone()
    x2[:, 96:128] = 0
    assert not torch.equal(D.linear(x2, c.w, c.e).out, c.out.double())


@pytest.mark.parametrize("tin", [BF16, F32])
def test_teeth_k_tail_read_as_zero(tin):
    K = D.TILE_K[tin][1]
    x, w, e = _case(tin, F32, N=72, K=K)
    x2 = x.clone()
    x2[:, D.ept(tin):] = 0
    _leaves(D.linear(x2, w, e, tin, F32, "tile").out, D.linear(x, w, e, tin, F32, "tile"), "K tail as zero")


def test_teeth_bias_shifted_one_column():
    x, w, e = _case()
    ref = D.linear(x, w, e)
    e.bias = e.bias.roll(1)
    _leaves(D.linear(x, w, e).out, ref, "bias shifted")
    c = D.exact_case(BF16, BF16, 64, 65, 128)
    c.e.bias = c.e.bias.roll(1)
    assert not torch.equal(D.linear(c.x, c.w, c.e).out, c.out.double())


def test_teeth_rows_swapped():
    x, w, e = _case(form=4)
    ref = D.linear(x, w, e)
    e.row1, e.row2 = e.row2, e.row1
    _leaves(D.linear(x, w, e).out, ref, "row1 / row2 swapped")
    c = D.exact_case(BF16, BF16, 64, 65, 128, period=37)
    c.e.row1, c.e.row2 = c.e.row2, c.e.row1
    assert not torch.equal(D.linear(c.x, c.w, c.e).out, c.out.double())


def test_teeth_period_wrap_off_by_one_on_last_tile():
    M, period = 257, 37
    x, w, e = _case(M=M, form=4, period=period)
    ref = D.linear(x, w, e)
    m = torch.arange(M)
    idx = torch.where(m < 256, m % period, (m - 1) % period)
    e.row1, e.row2, e.period = e.row1[idx], e.row2[idx], 0
    mut = D.linear(x, w, e).out
    _leaves(mut, ref, "period wrap on the last tile")
    assert D.ratio(mut[:256], ref.out[:256], ref.bound[:256]) == 0.0


def test_teeth_stride_one_for_two():
    x, w, e = _case(form=2)
    ref = D.linear(x, w, e, tout=F32)
    e.s1 = 1
    _leaves(D.linear(x, w, e, tout=F32).out, ref, "stride 1 for 2")


def test_teeth_residual_with_ldc():
    M, N = 129, 384
    x, w, e = _case()
    ref = D.linear(x, w, e)
    store = torch.zeros(M, N + D.PADS["ld_resid"], dtype=e.resid.dtype)
    store[:, :N] = e.resid
    e.resid = store.reshape(-1)[:M * (N + D.PADS["ldc"])].view(M, N + D.PADS["ldc"])[:, :N]
    mut = D.linear(x, w, e).out
    _leaves(mut, ref, "resid with ldc")
    assert D.ratio(mut[:1], ref.out[:1], ref.bound[:1]) == 0.0


@pytest.mark.parametrize("off", [-8, 8])
def test_teeth_ln_over_other_columns(off):
    x, w, e = _case(N=128, K=64, ln_form=D.LN_FORMS[0])
    ref = D.linear(x, w, e)
    n = 128 + off
    v = F.pad(ref.v, (0, 8))[:, :n]
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + e.ln_eps)
    _leaves((ref.v - mean) * rstd * e.ln_g.double() + e.ln_b.double(), ref, f"LN over N{off:+d}")


def test_teeth_post_af_without_period():
    M = 129
    x, w, e = _case(N=128, K=64, ln_form=D.LN_FORMS[3])
    assert e.post_af_period == D.AF_PERIOD and e.post_af.numel() == D.AF_PERIOD
    ref = D.linear(x, w, e)
    e.post_af, e.post_af_period = D.vecs(BF16, 128).post_af[:M], 0
    mut = D.linear(x, w, e).out
    _leaves(mut, ref, "post_af without its period")
    assert D.ratio(mut[:D.AF_PERIOD], ref.out[:D.AF_PERIOD], ref.bound[:D.AF_PERIOD]) == 0.0


def test_teeth_stats_of_neighbouring_tile():
    x, w, e = _case(N=1152, stats=True)
    ref = D.linear(x, w, e, bn=384)
    r = D.ratio(ref.stats.roll(1, 0), ref.stats, ref.stats_bound)
    assert r > 1.0
    c = D.exact_case(BF16, BF16, 64, 65, 256, stats_bn=128)
    assert not torch.equal(c.stats.roll(1, 0), c.stats)


def test_teeth_rownorm_faults():
    tin, tout, M, N, K = BF16, BF16, 129, 320, 192
    x, w, e = _case(tin, tout, M, N, K, form=0, period=0)
    e.rownorm = D.make_rownorm(tin, tout, K, N, M, 5)
    ref = D.linear(x, w, e)
    st = e.rownorm.stats
    e.rownorm.stats = st.roll(-1, 1)
    _leaves(D.linear(x, w, e).out, ref, "row-norm stats of row m + 1")
    e.rownorm.stats, e.rownorm.n_parts = st, 4
    _leaves(D.linear(x, w, e).out, ref, "n_parts - 1 partials")
    c = D.exact_case(tin, tout, 192, 65, 128, strides=None, rownorm=5)
    c.e.rownorm.stats = c.e.rownorm.stats.roll(-1, 1)
    assert not torch.equal(D.linear(c.x, c.w, c.e).out, c.out.double())


@pytest.mark.parametrize("tout,kernel,wrong", [(F32, "rows", "poly"), (BF16, "tile", "poly"), (BF16, "rows", "erf")])
def test_teeth_wrong_gelu(tout, kernel, wrong):
    """f32 outputs pin the exact-erf GELU anywhere; a bf16 output pins its GELU where the output is
    small against the fit's 2.6e-5 (the half ulp of |y| < 2^-7 is below 1.6e-5).  On the selection
    matrix (one product per output): the dense dz at K = 192 is itself above 2.6e-5."""
    x, _, e = _case(tout=tout, form=4, period=0)
    w = D.selection_w(BF16, 192, 384)
    e.row1 = e.row2 = None
    ref = D.linear(x, w, e, BF16, tout, kernel)
    _leaves(D.linear(x, w, e, BF16, tout, kernel, gelu=wrong).out, ref, f"{wrong} GELU in {kernel} -> {tout}")


def test_teeth_wrong_row_across_the_half():
    x, w, e = _case()
    ref = D.linear(x, w, e)
    mut = ref.out.clone()
    mut[64:128] = ref.out[65:129]
    _leaves(mut, ref, "rows 64.. one off")
    assert D.ratio(mut[:64], ref.out[:64], ref.bound[:64]) == 0.0


# ----------------------------------------------------------------- d. tables --
def test_tables_reach_every_instantiation_and_edge():
    got = D.all_table_instances()
    assert set(got) == set(D.ALL_INSTANCES) and len(D.ALL_INSTANCES) == 36, sorted(set(D.ALL_INSTANCES) - set(got))
    assert min(got.values()) >= len(D.ROWS_M)
    for tin in (BF16, F32):
        for nw in D.NWS:
            cases = D.rows_cases(tin, nw)
            assert {D.rows_pick_nw(N) for _, N, _, _ in cases} == {nw}
            assert {N // (64 * nw) for _, N, _, _ in cases} >= {1} and max(N // (64 * nw) for _, N, _, _ in cases) > 1
            assert {K // D.ept(tin) for _, _, K, _ in cases} == {1, 2, 3}           # both exits of the stage ring
            assert {M for M, _, _, _ in cases} >= {1, 63, 64, 65, 127, 128, 129, 257}
            grids = {D.dispatch(tin, BF16, M, N, K).grid for M, N, K, _ in cases}
            assert any(g > 8 and g % 8 for g in grids), (nw, grids)
            combos = {(i % 6, D.form_of(i, M)[1] != 0 and D.periods(M).index(D.form_of(i, M)[1])) for M, _, _, i in cases}
            assert len({c[0] for c in combos}) == 6 and {c[1] for c in combos} >= {1, 2, 3, 4}
            assert all(D.rows_pick_nw(N, True) == nw for _, N, _, _ in D.ln_cases(tin, nw))
            assert {i % 5 for *_, i in D.ln_cases(tin, nw)} == set(range(5))
        tc = D.tile_cases(tin)
        assert {N for _, N, _, t, _ in tc if not t} == {8, 72, 136, 200}
        assert all(K % D.ept(tin) for _, _, K, t, _ in tc if not t)                 # every K has a tail
        assert {cdiv for cdiv in (D.cdiv(K, D.ept(tin)) for _, _, K, t, _ in tc if not t)} == {1, 2, 3}
        assert {M for M, *_ in tc} >= {1, 3, 127, 128, 129, 641}
        assert max(D.dispatch(tin, BF16, M, N, K, tile128=t).grid for M, N, K, t, _ in tc) == 12
        assert all(D.dispatch(tin, BF16, M, N, K, tile128=t).kernel == "tile" for M, N, K, t, _ in tc)
        assert all(D.dispatch(tin, BF16, M, N, K).kernel == "rows" for M, N, K, t, _ in tc if t)
    assert {f["rank"] for f in D.FORMS} >= {None, (1, 2), (2, 1), (1, 1), (2, 2)}
    assert {f["pad"] for f in D.FORMS} == {False, True} and {f["act"] for f in D.FORMS} == {0, 1, 2, 3}
    p = D.periods(257)
    assert p[0] == 0 and p[1] == 1 and 1 < p[2] < 64 and p[3] == 128 and p[4] > 257
    assert {f["afp"] for f in D.LN_FORMS} == {0, 1} and {f["post"] for f in D.LN_FORMS} == {0, 1, 2}
    assert D.RN_PARTS == (1, 2, 5) and D.PADS == dict(lda=8, ldw=16, ldc=8, ld_resid=16, ld_post=24)


def test_dispatch_refusals_and_forced_width():
    assert D.dispatch(BF16, BF16, 5, 384, 64, nw=2).name == D.rows_name(BF16, BF16, 2, False)
    assert D.dispatch(BF16, BF16, 5, 384, 64, ln=True, nw=2).nw == 6                # a full row ignores gemm_nw
    assert D.dispatch(BF16, F32, 5, 8, 8).name == D.tile_name(BF16, F32)
    assert D.dispatch(F32, F32, 5, 64, 40).kernel == "tile" and D.dispatch(F32, F32, 5, 64, 32).kernel == "rows"
    for bad in (dict(N=72, K=64, stats=True), dict(N=512, K=64, ln=True), dict(N=64, K=72, rownorm=True), dict(N=68, K=64)):
        with pytest.raises(ValueError):
            D.dispatch(BF16, BF16, 5, **bad)


def test_remap_is_a_permutation():
    for n in range(1, 65):
        assert sorted(D.xcd_remap(n, i) for i in range(n)) == list(range(n))
    assert [D.xcd_remap(12, i) for i in range(12)] == [0, 2, 4, 6, 8, 9, 10, 11, 1, 3, 5, 7]


def test_pick_nw_matches_stat_tiles():
    from src import kernels
    for N in range(64, 4097, 64):
        assert N // (64 * D.rows_pick_nw(N)) == kernels.stat_tiles(N)
    assert D.rows_pick_nw(100) == 0 and D.rows_pick_nw(512, True) == 0
    assert [D.stats_depth(64 * nw) for nw in D.NWS] == [28, 20, 12, 11]
