"""CPU proofs behind tests/test_gpu_block_tail.py (tests/tail_refs.py): with the roundings and flags
off, tail_ref and proj_ref are the plain fp64 torch formula of test_tail32_kernel /
test_proj_kernel_vs_fp64 to 1e-12; an f32 emulation of the same function (torch's CPU summation
order, the two bf16 roundings, one-pass statistics) stays inside the bound on every family; each of
the listed single faults, applied to that emulation, leaves the bound; the flagged-rounding caps hold
on the reference alone; the families are what their names say (every weight fragment holds a
non-zero, low_var's three variances are within a factor 4 of eps, ln_rows' rows are the rows
described) and the shape tables reach the edges they are there for."""
import functools

import pytest
import torch
import torch.nn.functional as F

import tail_refs as T

F64, F32, BF16 = T.F64, T.F32, T.BF16
M = 129
TOL = dict(rtol=1e-12, atol=1e-12)


@functools.lru_cache(maxsize=None)
def _ref(family, D, eps=1e-5, pre=True):
    return T.ref_of(T.case(family, D, M, eps), eps, pre)


def _families():
    return [(f, 1e-5) for f in T.FAMILIES] + [("low_var", 1e-3)]


# ------------------------------------------------- a. references == torch fp64 --
@pytest.mark.parametrize("D", [128, 384])
def test_tail_ref_matches_torch(D):
    """LN_f unfolded (w2g = W2 diag(gf), b2' = b2 + W2 bf, c1 = rowsum w2g, built in fp64 so that the
    folding itself costs nothing), F.layer_norm and F.leaky_relu, both entry points."""
    g = T._gen(D, 1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    att, x, w_o, w1, w2 = rn(45, D), rn(45, D), rn(D, D) / D ** 0.5, rn(4 * D, D) / D ** 0.5, rn(D, 4 * D) / (4 * D) ** 0.5
    b_o, g1, be1, b1, b2, gf, bf, g2, be2 = rn(D), 1 + 0.2 * rn(D), rn(D), rn(4 * D), rn(D), 1 + 0.2 * rn(4 * D), rn(4 * D), rn(D), rn(D)
    w2g = w2 * gf
    vec = torch.cat([b1, b2 + w2 @ bf, w2g.sum(1), g2, be2])
    eps = 1e-5

    def ffn(x1):
        hn = F.layer_norm(F.leaky_relu(x1 @ w1.T + b1, 0.1), (4 * D,), gf, bf, eps)
        return F.layer_norm(x1 + F.leaky_relu(hn @ w2.T + b2, 0.1), (D,), g2, be2, eps)

    x1 = F.layer_norm(x + att @ w_o.T + b_o, (D,), g1, be1, eps)
    r = T.tail_ref(att, x, w_o, w1, w2g, b_o, g1, be1, vec, eps, True, rounding=False)
    torch.testing.assert_close(r.out, ffn(x1), **TOL)
    assert not r.x1_flag.any() and not r.h_flag.any()
    r = T.tail_ref(None, x, None, w1, w2g, None, None, None, vec, eps, False, rounding=False)
    torch.testing.assert_close(r.out, ffn(x), **TOL)


def test_tail_ref_rounds_where_the_kernels_round():
    """With the roundings on, x1 and h are bf16 numbers, LN_f's statistics are those of the unrounded a
    and the residual of LN2 is the rounded x1."""
    c = T.case("sparse", 128, M)
    r = _ref("sparse", 128)
    assert torch.equal(T.rne_bf16(r.x1), r.x1) and torch.equal(T.rne_bf16(r.h), r.h) and not torch.equal(r.h, r.a)
    torch.testing.assert_close(r.hm, r.a.mean(-1, keepdim=True), **TOL)
    b1, b2, c1, g2, be2 = T.split_vec(c.vec, 128, "cpu")
    v2 = r.x1 + F.leaky_relu(r.hr * (r.h @ c.w2g.double().T - r.hm * c1) + b2, 0.1)
    torch.testing.assert_close(r.out, F.layer_norm(v2, (128,), g2, be2, T.f32(1e-5)), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("D,NC", [(128, 3), (384, 1)])
def test_proj_ref_matches_torch(D, NC):
    c = T.dense_proj(D, NC, 45)
    r = T.proj_ref(c.x, c.w, c.b)
    torch.testing.assert_close(r.out, F.linear(c.x.double(), c.w.double(), c.b.double()), **TOL)
    assert bool((r.bound >= T.bf16_ulp(r.out) / 2).all())


# ------------------------------------------------------------ b. the families --
@pytest.mark.parametrize("D", T.DS)
def test_every_weight_fragment_holds_a_non_zero(D):
    for fam in ("sparse", "low_var"):
        c = T.case(fam, D, 4)
        assert T.fragments_covered(c.w_o, "w") and T.fragments_covered(c.w1, "w") and T.fragments_covered(c.w2g, "w2")
        for w in (c.w_o, c.w1, c.w2g):
            assert bool(((w.float() != 0).sum(1) == 4).all())
    p = T.sparse_proj(D, 3, 4)
    assert T.fragments_covered(p.w, "w")
    assert not bool(T.case("phase_a", D, 4).w1.float().any())
    # frag_cols restates mfma32.h in_feat(s, kh, j) = 32 (s >> 1) + 16 kh + 8 (s & 1) + j
    for s in range(D // 16):
        assert sorted(T.frag_cols("w", s)) == sorted(32 * (s >> 1) + 16 * kh + 8 * (s & 1) + j for kh in (0, 1) for j in range(8))


@pytest.mark.parametrize("eps", T.EPS_LIST)
@pytest.mark.parametrize("D", T.DS)
def test_low_var_is_within_a_factor_4_of_eps(D, eps):
    for pre in (True, False):
        r = T.ref_of(T.case("low_var", D, M, eps), eps, pre)
        for name in (("var1",) if pre else ()) + ("varf", "var2"):
            v = getattr(r, name)
            print(f"low_var D={D} eps={eps} pre={pre} {name}/eps: {float(v.min()) / eps:.2f} .. {float(v.max()) / eps:.2f}")
            assert eps / 4 <= float(v.min()) and float(v.max()) <= 4 * eps, name


def test_ln_rows_are_the_rows_described():
    for D in T.DS:
        c = T.case("ln_rows", D, M)
        r = _ref("ln_rows", D) if D != 256 else T.ref_of(c, 1e-5, True)
        v1 = c.x.double() + c.att.double() @ c.w_o.double().T + c.b_o.double()
        const, one, far = (v1[i] for i in T.SPECIAL_ROWS)
        assert bool((const == 1).all()) and float(r.var1[T.SPECIAL_ROWS[0]]) == 0.0
        assert int((one != 0).sum()) == 1
        assert float(far.mean() / far.std(unbiased=False)) == 64.0
        # the constant row: rstd = 1 / sqrt(eps), LN1's output is be1
        torch.testing.assert_close(r.x1[T.SPECIAL_ROWS[0]], T.rne_bf16(c.be1.double()), rtol=0, atol=0)


def test_ln_rows_reach_the_32_row_bodies():
    """At M_SPLIT the same three rows lie in the last 229 rows, which tail_split = 64 runs as eight 32-row
    workgroups: the constant row in the ragged last one, the other two in two others."""
    c = T.case("ln_rows", 384, T.M_SPLIT)
    first = T.M_SPLIT - 229
    groups = [(r - first) // 32 for r in T.SPLIT_ROWS]
    assert first % 128 == 0 and all(first <= r < T.M_SPLIT for r in T.SPLIT_ROWS)
    assert groups[0] == 7 and len(set(groups)) == 3
    rows = list(T.SPLIT_ROWS)
    v1 = c.x[rows].double() + c.att[rows].double() @ c.w_o.double().T + c.b_o.double()
    const, one, far = v1
    assert bool((const == 1).all()) and int((one != 0).sum()) == 1
    assert float(far.mean() / far.std(unbiased=False)) == 64.0
    assert all(torch.equal(c.x1[r].double(), v) for r, v in zip(rows, v1))


def test_shape_tables():
    assert T.M_SPLIT == 257 * 128 + 32 * 3 + 5 and max(T.tail_m(384)) == 3073
    for D in T.DS:
        m = T.tail_m(D)
        assert {1, 31, 32, 33, 127, 128, 129} <= set(m) and (m[-1] - 1) // 128 == T.NCH[D] == 4 * D // 64
        for NC in (1, 3):
            assert T.proj_m(D, NC)[-1] == 128 * NC + 1 and set(T.M_SMALL) <= set(T.proj_m(D, NC))
            assert set(T.proj_m(D, NC, True)) == set(T.proj_m(D, NC)) | {160} and len(set(T.proj_m(D, NC, True))) == len(T.proj_m(D, NC, True))
    assert 160 in T.WIDE_M
    # tailw_launch's split: T tiles, rem = T % 256; rem <= tail_split: 4 rem' workgroups of 32 rows
    tiles = -(-T.M_SPLIT // 128)
    rem = tiles % 256
    assert tiles > 256 and 0 < rem <= 64
    rest = T.M_SPLIT - (tiles - rem) * 128
    assert rest == 128 + 96 + 5 and -(-rest // 32) == 8 and rest % 32 == 5      # the last 32-row workgroup: 5 rows


# ----------------------------------------------------- c. the f32 emulation --
def _lrelu32(z):
    return torch.maximum(z, z * torch.tensor(0.1, dtype=F32))


def _stats32(v):
    """The one-pass sums of the rows of v in f32: (sum, sum of squares)."""
    return v.sum(-1, keepdim=True), (v * v).sum(-1, keepdim=True)


def _finish32(s, q, n, eps):
    """(mean, rstd) of n values from their one-pass sums, as the kernels take them."""
    mean = s * torch.tensor(1.0 / n, dtype=F32)
    var = (q * torch.tensor(1.0 / n, dtype=F32) - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))


def _frag(w, kind, tile, s, what):
    """Fault: the 32 x 16 fragment (tile, k16 step s) of w zeroed, or swapped with that of step s ^ 1."""
    w = w.clone()
    rows = slice(32 * tile, 32 * tile + 32)
    a, b = T.frag_cols(kind, s), T.frag_cols(kind, s ^ 1)
    if what == "zero":
        w[rows, a] = 0
    else:
        blk = w[rows][:, a].clone()
        w[rows, a] = w[rows][:, b]
        w[rows, b] = blk
    return w


def emulate(c, eps, pre=True, fault=None):
    """The tail in f32 on the CPU (torch's blocked matmul and pairwise sums: another order than either
    kernel's), with the bf16 roundings of x1, the hidden and the output.  fault: one (name, *args)."""
    name, *fa = fault or ("none",)
    f = lambda t: t.float().clone()
    D = c.D
    e = dict(ln1=eps, lnf=eps, ln2=eps)
    if name == "eps":
        e[fa[0]] = fa[1]
    w = dict(w_o=f(c.w_o), w1=f(c.w1), w2g=f(c.w2g))
    if name == "frag":
        which, tile, s, what = fa
        w[which] = _frag(w[which], "w2" if which == "w2g" else "w", tile, s, what)
    v = dict(b_o=f(c.b_o), b1=f(c.b1), b2=f(c.b2), c1=f(c.c1), g2=f(c.g2), be2=f(c.be2))
    if name == "shift":
        v[fa[0]] = torch.roll(v[fa[0]], 1)
    e32 = {k: T.f32(x) for k, x in e.items()}

    def same_stats(mean, rstd, which):
        if name == "stats_rows" and fa[0] == which:            # rows 32 .. 63 with the statistics of 0 .. 31
            mean, rstd = mean.clone(), rstd.clone()
            mean[32:64], rstd[32:64] = mean[0:32], rstd[0:32]
        return mean, rstd

    if pre:
        v1 = (f(c.att) @ w["w_o"].T + v["b_o"]) + f(c.x)
        s, q = _stats32(v1)
        if name == "ln1_partial":                              # wave 2's 96 features, token group 1 of tile 0
            part = v1[32:64, 192:288]
            k = fa[0]                                          # -1: dropped, +1: counted twice
            s, q = s.clone(), q.clone()
            s[32:64] += k * part.sum(-1, keepdim=True)
            q[32:64] += k * (part * part).sum(-1, keepdim=True)
        mean, rstd = same_stats(*_finish32(s, q, D, e32["ln1"]), "ln1")
        y1 = (v1 - mean) * rstd * f(c.g1) + f(c.be1)
        x1 = y1.to(BF16).float()
        if name == "flip_x1":                                  # the listed elements as their other bf16 neighbour
            x1 = torch.where(fa[0], fa[1], x1)
    else:
        y1 = x1 = f(c.x1)
    a = _lrelu32(x1 @ w["w1"].T + v["b1"])
    h = a.to(BF16).float()
    src = h if name == "lnf_rounded" else a
    hm, hr = same_stats(*_finish32(*_stats32(src), 4 * D, e32["lnf"]), "lnf")
    if name == "swap_hidden":
        j1, j2 = fa
        h[:, [j1, j2]] = h[:, [j2, j1]]
    p = hr * (h @ w["w2g"].T - hm * v["c1"]) + v["b2"]
    v2 = (y1 if name == "unrounded_resid" else x1) + _lrelu32(p)
    mean, rstd = same_stats(*_finish32(*_stats32(v2), D, e32["ln2"]), "ln2")
    return ((v2 - mean) * rstd * v["g2"] + v["be2"]).to(BF16)


@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("D", [128, 384])
def test_emulation_stays_within_the_bound(D, pre):
    for fam, eps in _families():
        if fam == "phase_a" and not pre:
            continue
        c = T.case(fam, D, M, eps)
        r = _ref(fam, D, eps, pre)
        got = emulate(c, eps, pre)
        q = ((got.double() - r.out).abs() / r.bound)
        print(f"{fam} D={D} eps={eps} pre={pre}: emulation err/bound max {float(q.max()):.3f} median {float(q.median()):.3f}; "
              f"bound / half ulp median {float((r.bound / r.half_ulp).median()):.3f} max {float((r.bound / r.half_ulp).max()):.1f}")
        assert T.ratio(got, r.out, r.bound) <= 1.0, (fam, D, eps, pre)


def test_proj_emulation_stays_within_the_bound():
    for make in (T.dense_proj, T.sparse_proj):
        c = make(384, 3, M)
        r = T.proj_ref(c.x, c.w, c.b)
        got = (c.x.float() @ c.w.float().T + c.b).to(BF16)
        q = T.ratio(got, r.out, r.bound)
        print(f"proj {make.__name__}: emulation err/bound {q:.3f}; bound / half ulp max {float((r.bound / (T.bf16_ulp(r.out) / 2)).max()):.3f}")
        assert q <= 1.0


# ------------------------------------------------------- d. fault injection --
def _hidden_pair(c):
    """Two hidden units of chunk 1 that feed different outputs (w2g columns with a non-zero each)."""
    nz = (c.w2g.float() != 0).any(0).nonzero().flatten()
    nz = nz[(nz >= 64) & (nz < 128)]
    return int(nz[0]), int(nz[-1])


def _frag_faults():
    out = []
    for which, tiles, steps in (("w_o", 12, 24), ("w1", 48, 24), ("w2g", 12, 96)):
        for what in ("zero", "swap"):
            out += [("frag", which, t, s, what) for t, s in ((0, 0), (tiles // 2, steps // 2 - 1), (tiles - 1, steps - 1))]
    return out


SPARSE_FAULTS = ([("lnf_rounded",), ("ln1_partial", -1), ("ln1_partial", 1), ("swap_hidden",), ("unrounded_resid",)]
                 + [("shift", k) for k in ("b_o", "b1", "b2", "c1", "g2", "be2")]
                 + [("stats_rows", k) for k in ("ln1", "lnf", "ln2")] + _frag_faults())


@pytest.mark.parametrize("fault", SPARSE_FAULTS, ids=lambda f: "-".join(str(x) for x in f))
def test_fault_leaves_the_bound_on_sparse(fault):
    """Each single fault of the emulation pushes at least one element past the bound (D = 384, M = 129)."""
    c = T.case("sparse", 384, M)
    r = _ref("sparse", 384)
    if fault[0] == "swap_hidden":
        fault = ("swap_hidden", *_hidden_pair(c))
    got = emulate(c, 1e-5, True, fault)
    assert not torch.equal(got, emulate(c, 1e-5, True)), "the fault changes nothing"
    q = (got.double() - r.out).abs() / r.bound
    print(f"{fault}: err/bound max {float(q.max()):.2f}, {int((q > 1).sum())} elements past the bound")
    assert float(q.max()) > 1.0, fault


def test_flagged_allowance_carries_the_pre_rounding_error():
    """A flagged element's allowance is e = d + ulp, not one ulp.  The effect: the kernel rounds a flagged
    x1 to its other neighbour (x1's own error d is an f32 rounding, so the neighbour is one ulp away); a
    hidden unit it feeds then moves by |w1| ulp(x1), several of its own ulps where |a| is small, before
    it is rounded.  The emulation with every flagged x1 so rounded stays inside the bound, and leaves
    the bound that allows a flagged hidden unit one ulp alone (tail_ref's carry_d = False)."""
    c = T.case("sparse", 384, M)
    r = _ref("sparse", 384)
    lo, hi = T.rne_bf16(r.y1 - r.dy1), T.rne_bf16(r.y1 + r.dy1)
    other = torch.where(lo != r.x1, lo, hi)
    flip = r.x1_flag & (other != r.x1)
    assert int(flip.sum()) > 0 and bool(((other - r.x1).abs() <= T.bf16_ulp(r.y1.abs() + r.dy1) + r.dy1)[flip].all())
    got = emulate(c, 1e-5, True, ("flip_x1", flip, other.float()))
    assert not torch.equal(got, emulate(c, 1e-5, True))
    one_ulp = T.ref_of(c, 1e-5, True, carry_d=False)
    assert torch.equal(one_ulp.out, r.out) and bool((one_ulp.bound <= r.bound).all())
    q, q1 = T.ratio(got, r.out, r.bound), T.ratio(got, one_ulp.out, one_ulp.bound)
    print(f"{int(flip.sum())} flagged x1 as their other neighbour: err/bound {q:.3f} with e = d + ulp, {q1:.3f} with e = ulp")
    assert q <= 1.0 < q1


@pytest.mark.parametrize("eps", T.EPS_LIST)
@pytest.mark.parametrize("which", ["ln1", "lnf", "ln2"])
@pytest.mark.parametrize("D", [128, 384])
def test_wrong_eps_leaves_the_bound_on_low_var(D, which, eps):
    """eps = 0 and the other eps of the pair, one LayerNorm at a time."""
    c = T.case("low_var", D, M, eps)
    r = _ref("low_var", D, eps)
    other = T.EPS_LIST[1 - T.EPS_LIST.index(eps)]
    for wrong in (0.0, other):
        got = emulate(c, eps, True, ("eps", which, wrong))
        q = (got.double() - r.out).abs() / r.bound
        print(f"low_var D={D} eps={eps}: {which} run with eps = {wrong}: err/bound max {float(q.max()):.1f}, "
              f"{float((q > 1).double().mean()):.3f} of the elements past the bound")
        assert float(q.max()) > 1.0, (which, wrong)


@pytest.mark.parametrize("fault", ["k_step", "bias"])
def test_proj_fault_leaves_the_bound_on_dense(fault):
    c = T.dense_proj(384, 3, M)
    r = T.proj_ref(c.x, c.w, c.b)
    w, b = c.w.float().clone(), c.b.clone()
    if fault == "k_step":
        w[:, T.frag_cols("w", 11)] = 0
    else:
        b = torch.roll(b, 1)
    got = (c.x.float() @ w.T + b).to(BF16)
    assert T.ratio(got, r.out, r.bound) > 1.0


# ------------------------------------------------------------------ e. caps --
@pytest.mark.parametrize("D", T.DS)
def test_flag_caps(D):
    """On sparse, phase_a and low_var: at most 5 % of x1 and 10 % of the hidden flagged, and no row whose
    every output carries a flagged allowance above its half ulp.  Conditions on the reference alone."""
    for fam, eps in _families():
        if fam == "ln_rows":
            continue
        for pre in (True, False):
            r = _ref(fam, D, eps, pre) if D != 256 else T.ref_of(T.case(fam, D, M, eps), eps, pre)
            sx, sh = float(r.x1_flag.double().mean()), float(r.h_flag.double().mean())
            over = (r.flag_term > r.half_ulp)
            print(f"{fam} D={D} eps={eps} pre={pre}: flagged x1 {sx:.4f}, hidden {sh:.4f}; outputs with a flagged allowance "
                  f"above the half ulp {float(over.double().mean()):.4f}, worst row {float(over.double().mean(-1).max()):.3f}")
            assert sx <= 0.05 and sh <= 0.10, (fam, D, eps, pre)
            assert not bool(over.all(-1).any()), (fam, D, eps, pre)
