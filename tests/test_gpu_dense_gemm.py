"""Every instantiation of the dense layer (csrc/gemm_rows.hip: 32 rows_gemm_kernel forms; csrc/gemm.hip:
4 linear_kernel forms) through the C ABI snvrag_linear_ex, against the fp64 reference of
tests/dense_refs.py within its derived per-element bounds: at 1, 2 and 3 K-tiles (both exits of the
stage ring) and K tails, M on both sides of the 64-row half and the 128-row tile, one and several
column tiles, grids beyond 8 workgroups that are no multiple of 8 (the remap's remainder path), every
row_period / stride / post_af_period kind, padded and contiguous leading dimensions, and the exact
family bit for bit (tests/test_dense_refs_cpu.py proves the reference, the bounds, their teeth and the
tables).

Every input (A, W, bias, rank vectors, residual, post_base, post_af, ln_g / ln_b, row-norm stats, c1)
is a prefix of NaN-continued storage sized exactly, padding columns of padded leading dimensions are
NaN, every output and stats_out lives in sentinel-filled storage whose guard row and padding columns
must be unchanged, and every case is launched twice and must give the same bits.  max err / bound is
printed per case with the instantiation's name.  The fp64 GEMM of a (type, K, N) is evaluated once on
the device at the largest M and shared by row prefix."""
import ctypes as C

import pytest
import torch

import dense_refs as D
import sgemm_refs as S
from test_gpu_stream_gemm import DEV, PAD, SENT, K, N, _check, _in, _same_bits

pytestmark = pytest.mark.gpu

BF16, F32, F64 = D.BF16, D.F32, D.F64
CODE = {F32: 0, BF16: 1}
NAN = float("nan")
_IDS = [f"{D.TN[a]}-{D.TN[b]}" for a, b in D.PAIRS]
_CACHE = {}


# ------------------------------------------------------------- guarded calls --
def _pad2(t, ld):
    """[R, C] values as R rows of ld elements, the padding columns and what follows NaN."""
    R, Cc = t.shape
    buf = torch.full((R * ld + PAD,), NAN, dtype=t.dtype, device=DEV)
    buf[:R * ld].view(R, ld)[:, :Cc] = t.to(DEV)
    return buf


def _operand(key, t, ld):
    """A or W storage, once per (operand, leading dimension)."""
    if key is None:
        return _pad2(t, ld)
    if (key, ld) not in _CACHE:
        _CACHE[(key, ld)] = _pad2(t, ld)
    return _CACHE[(key, ld)]


def _guarded(buf, rows, ld, cols, what):
    v = buf.cpu()
    assert bool((v[rows * ld:] == SENT).all()), f"{what}: wrote past its {rows} rows"
    v = v[:rows * ld].view(rows, ld)
    assert bool((v[:, cols:] == SENT).all()), f"{what}: wrote into the padding columns"
    return v[:, :cols].clone()


def call(M, Nn, Kk, tin, tout, x, w, e, pad=False, tile128=0, nw=0, keys=(None, None), what="", null_epi=False):
    """Two guarded launches of snvrag_linear_ex: (out [M, N], stats [T, M, 2] or None) on the CPU."""
    n = N()
    p = D.PADS if pad else dict.fromkeys(D.PADS, 0)
    lda, ldw, ldc = Kk + p["lda"], Kk + p["ldw"], Nn + p["ldc"]
    xs, ws = _operand(keys[0] and (keys[0], M), x[:M], lda), _operand(keys[1], w, ldw)
    hold = []

    def put(t, dt=F32):
        hold.append(_in(t.to(dt)))
        return n.ptr(hold[-1])

    def put2(t, ld):
        hold.append(_pad2(t.to(tout), ld))
        return n.ptr(hold[-1])
    E = n.Epilogue()
    if e.bias is not None:
        E.bias = put(e.bias)
    if e.row1 is not None:
        E.row1, E.row1_stride, E.col1 = put(e.row1), e.s1, put(e.col1)
    if e.row2 is not None:
        E.row2, E.row2_stride, E.col2 = put(e.row2), e.s2, put(e.col2)
    E.row_period, E.act, E.slope = e.period, e.act, e.slope
    if e.resid is not None:
        E.resid, E.ld_resid = put2(e.resid[:M], Nn + p["ld_resid"]), Nn + p["ld_resid"]
    if e.ln_g is not None:
        E.ln_g, E.ln_b, E.ln_eps, E.ln_act = put(e.ln_g), put(e.ln_b), e.ln_eps, e.ln_act
    if e.post_base is not None:
        E.post_base, E.ld_post, E.post_scale = put2(e.post_base[:M], Nn + p["ld_post"]), Nn + p["ld_post"], e.post_scale
    if e.post_af is not None:
        E.post_af, E.post_af_period, E.post_maf = put(e.post_af), e.post_af_period, e.post_maf
    RN = None
    if e.rownorm is not None:
        r = e.rownorm
        assert r.stats.shape[1] == M
        RN = n.RowNormS(put(r.stats[:r.n_parts].contiguous()), r.n_parts, r.dim, r.eps, put(r.c1))
    T = D.dispatch(tin, tout, M, Nn, Kk, e.ln_g is not None, e.stats, RN is not None, tile128, nw).tiles_n
    res = []
    for _ in range(2):
        out = torch.full(((M + 1) * ldc,), SENT, dtype=tout, device=DEV)
        st = torch.full((T * M * 2 + 64,), SENT, dtype=F32, device=DEV) if e.stats else None
        E.stats_out = n.ptr(st)
        with K().option("gemm_tile128", tile128), K().option("gemm_nw", nw):
            rc = n.lib().snvrag_linear_ex(CODE[tin], CODE[tout], M, Nn, Kk, n.ptr(xs), lda, n.ptr(ws), ldw, n.ptr(out), ldc,
                                          None if null_epi else C.byref(E), None if RN is None else C.byref(RN),
                                          n.stream_ptr())
        n.check(rc, f"linear_ex {what}")
        res.append((out, st))
    torch.cuda.synchronize()
    _same_bits(res[0][0], res[1][0], what)
    got = _guarded(res[0][0], M, ldc, Nn, f"out {what}")
    stats = None
    if e.stats:
        _same_bits(res[0][1], res[1][1], f"stats {what}")
        stats = _guarded(res[0][1], T * M, 2, 2, f"stats {what}").view(T, M, 2)
    return got, stats


def _sweep_case(tin, tout, M, Nn, Kk, e, pad, tag, tile128=0):
    """One dense table case against the shared fp64 GEMM; returns the launch's plan."""
    d = D.dispatch(tin, tout, M, Nn, Kk, e.ln_g is not None, e.stats, e.rownorm is not None, tile128)
    c = D.base(tin, Kk, Nn)
    what = f"{d.name} {tag} M={M} N={Nn} K={Kk} pad={int(pad)} grid={d.grid}"
    got, st = call(M, Nn, Kk, tin, tout, c.x, c.w, e, pad, tile128, keys=(("x", tin, Kk, Nn), ("w", tin, Kk, Nn)), what=what)
    ref = D.linear(c.x, c.w, e, tin, tout, d.kernel, d.bn, D.base_gemm(tin, Kk, Nn, DEV), M)
    _check(got, ref.out, ref.bound, f"out {what}")
    if st is not None:
        _check(st, ref.stats, ref.stats_bound, f"stats {what}")
    return d


def _bits_equal(got, want, what):
    bits = torch.int16 if got.dtype == BF16 else torch.int32
    bad = (got.view(bits) != want.view(bits)).nonzero()
    if bad.numel():
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: [{i}] = {float(got[i])}, expected {float(want[i])}; {bad.shape[0]} elements differ")


# ----------------------------------------------------- per-instantiation sweeps --
@pytest.mark.parametrize("nw", D.NWS)
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_rows_epilogue_vs_fp64(tin, tout, nw):
    """rows_gemm_kernel<TI, TO, NW, false> without LN: the (M, N, K) table of the NW, the six epilogue
    forms against the five row periods, padded and contiguous leading dimensions; then GELU on a
    selection matrix, where the bound is the activation's own error."""
    for M, Nn, Kk, i in D.rows_cases(tin, nw):
        form, period = D.form_of(i, M)
        d = _sweep_case(tin, tout, M, Nn, Kk, D.make_spec(tout, Nn, M, form, period), form["pad"], f"form={i % 6} period={period}")
        assert d.name == D.rows_name(tin, tout, nw, False)
    M, Nn, Kk = 129, D.ROWS_N[nw][1], D.ROWS_K[tin][2]
    e = D.spec(act=D.ACT_GELU, bias=D.vecs(tout, Nn).bias)
    x, w = D.base(tin, Kk, Nn).x[:M], D.selection_w(tin, Kk, Nn)
    what = f"{D.rows_name(tin, tout, nw, False)} GELU on a selection M={M} N={Nn} K={Kk}"
    got, _ = call(M, Nn, Kk, tin, tout, x, w, e, what=what)
    ref = D.linear(x.to(DEV), w, e, tin, tout)
    _check(got, ref.out, ref.bound, f"out {what}")


@pytest.mark.parametrize("nw", D.NWS)
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_rows_ln_tail_vs_fp64(tin, tout, nw):
    """The fused LayerNorm tail at N = 64 NW: ln_act, post_base, the MAF weight with and without
    post_af_period, over the same epilogue forms."""
    for M, Nn, Kk, i in D.ln_cases(tin, nw):
        form, period = D.form_of(i, M)
        e = D.make_spec(tout, Nn, M, form, period, D.LN_FORMS[i % 5])
        d = _sweep_case(tin, tout, M, Nn, Kk, e, form["pad"], f"LN form={i % 6} tail={i % 5} period={period}")
        assert d.name == D.rows_name(tin, tout, nw, False) and d.tiles_n == 1


@pytest.mark.parametrize("nw", D.NWS)
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_rows_stats_out_vs_fp64(tin, tout, nw):
    """stats_out [tile][M] (sum, sumsq) element by element, one and several column tiles."""
    for M, Nn, Kk, i in D.rows_cases(tin, nw):
        form, period = D.form_of(i + 1, M)
        e = D.make_spec(tout, Nn, M, form, period, stats=True)
        _sweep_case(tin, tout, M, Nn, Kk, e, form["pad"], f"stats form={(i + 1) % 6} period={period}")


@pytest.mark.parametrize("nw", D.NWS)
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_rows_rownorm_vs_fp64(tin, tout, nw):
    """rows_gemm_kernel<TI, TO, NW, true> in isolation: (sum, sumsq) partials written from fp64 and
    rounded to f32, exactly n_parts x M of them, n_parts = 1, 2, 5."""
    for M, Nn, Kk, i in D.rows_cases(tin, nw):
        form, period = D.form_of(i + 2, M)
        e = D.make_spec(tout, Nn, M, form, period)
        e.rownorm = D.make_rownorm(tin, tout, Kk, Nn, M, D.RN_PARTS[i % 3])
        d = _sweep_case(tin, tout, M, Nn, Kk, e, form["pad"], f"rownorm parts={e.rownorm.n_parts} form={(i + 2) % 6} period={period}")
        assert d.name == D.rows_name(tin, tout, nw, True)


@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_tile128_vs_fp64(tin, tout):
    """linear_kernel<TI, TO>: N of a partial first and second tile, K tails, M around the tile and 641
    (12 workgroups at N = 200), and row-panel shapes through gemm_tile128, where the same case must also
    land within its bound on the row-panel kernel."""
    for M, Nn, Kk, t, i in D.tile_cases(tin):
        form, period = D.form_of(i, M)
        e = D.make_spec(tout, Nn, M, form, period)
        d = _sweep_case(tin, tout, M, Nn, Kk, e, form["pad"], f"form={i % 6} period={period}", tile128=t)
        assert d.name == D.tile_name(tin, tout)
        if t:
            _sweep_case(tin, tout, M, Nn, Kk, e, form["pad"], f"(tile128 off) form={i % 6} period={period}")


@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_exact_answers(tin, tout):
    """The exact family, bit for bit: every NW plain (rank strides, periods, residual, stats_out, padded
    leading dimensions), every NW under row-norm, and the 128-tile kernel with a K tail."""
    i = 0
    for nw in D.NWS:
        for Nn in D.ROWS_N[nw]:
            for M in (1, 65, 129, 257):
                Kk = D.ROWS_K[tin][i % 3]
                period = D.periods(M)[i % 5]
                strides = ((1, 1), (2, 1), (1, 2))[i % 3]
                c = D.exact_case(tin, tout, Kk, M, Nn, period, strides, resid=bool(i % 2), stats_bn=64 * nw)
                what = f"{D.rows_name(tin, tout, nw, False)} exact M={M} N={Nn} K={Kk} period={period}"
                got, st = call(M, Nn, Kk, tin, tout, c.x, c.w, c.e, pad=bool(i % 4 < 2), what=what)
                _bits_equal(got, c.out, f"out {what}")
                _bits_equal(st, c.stats, f"stats {what}")
                c = D.exact_case(tin, tout, Kk, M, Nn, strides=None, rownorm=D.RN_PARTS[i % 3])
                what = f"{D.rows_name(tin, tout, nw, True)} exact M={M} N={Nn} K={Kk} parts={c.e.rownorm.n_parts}"
                got, _ = call(M, Nn, Kk, tin, tout, c.x, c.w, c.e, pad=bool(i % 2), what=what)
                _bits_equal(got, c.out, f"out {what}")
                i += 1
    for Nn in D.TILE_N:
        for M in (3, 129, 641):
            Kk = D.TILE_K[tin][i % 3]
            period = D.periods(M)[i % 5]
            c = D.exact_case(tin, tout, Kk, M, Nn, period, ((1, 1), (2, 1), (1, 2))[i % 3], resid=bool(i % 2))
            what = f"{D.tile_name(tin, tout)} exact M={M} N={Nn} K={Kk} period={period}"
            got, _ = call(M, Nn, Kk, tin, tout, c.x, c.w, c.e, pad=bool(i % 4 < 2), what=what)
            _bits_equal(got, c.out, f"out {what}")
            i += 1


# ---------------------------------------------------------- additional cases --
@pytest.mark.parametrize("tin,tout", [(BF16, BF16), (F32, F32)], ids=["bf16", "float"])
def test_rownorm_chained_to_stats_producer(tin, tout):
    """h = lrelu(x W1^T + b1) with stats_out over 3 column tiles, then lrelu(LN(h) W2^T + b2) with the LN
    folded into the second GEMM, whose partials are the first launch's own f32 stats: each launch
    against the reference of its given inputs."""
    M, D1, H = 257, D.ROWS_K[tin][2], 1152
    c = D.base(tin, D1, H)
    e1 = D.make_spec(tout, H, M, D.FORMS[2], 0, stats=True)
    d1 = D.dispatch(tin, tout, M, H, D1, stats=True)
    h, st = call(M, H, D1, tin, tout, c.x, c.w, e1, what=f"{d1.name} producer")
    r1 = D.linear(c.x, c.w, e1, tin, tout, bn=d1.bn, g=D.base_gemm(tin, D1, H, DEV), M=M)
    _check(h, r1.out, r1.bound, f"out {d1.name} chained producer M={M} N={H} K={D1}")
    _check(st, r1.stats, r1.stats_bound, f"stats {d1.name} chained producer M={M} N={H} K={D1}")
    assert d1.tiles_n == 3 == K().stat_tiles(H)
    g = S._gen(H, 43)
    w2 = torch.randn(384, H, generator=g) / H ** 0.5
    gam, beta, b2 = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g), torch.randn(384, generator=g)
    w2g, b2g, c1 = K().fold_layernorm(w2, b2, gam, beta, tin)
    e2 = D.spec(act=D.ACT_LRELU, slope=D.SLOPE, bias=b2g, rownorm=D.SimpleNamespace(stats=st, n_parts=3, dim=H, eps=S.f32(D.EPS), c1=c1))
    d2 = D.dispatch(tin, tout, M, 384, H, rownorm=True)
    h_in = h.to(tin)
    got, _ = call(M, 384, H, tin, tout, h_in, w2g, e2, what=f"{d2.name} consumer")
    r2 = D.linear(h_in.to(DEV), w2g, e2, tin, tout)
    _check(got, r2.out, r2.bound, f"out {d2.name} chained consumer M={M} N=384 K={H}")
    want = torch.nn.functional.leaky_relu(torch.nn.functional.layer_norm(h_in.double(), (H,), gam.double(), beta.double(), 1e-5)
                                          @ w2.double().T + b2.double(), D.SLOPE)
    torch.testing.assert_close(got.double(), want, rtol=2e-2, atol=8e-2)      # the existing test's tolerance, as a sanity check


@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_IDS)
def test_forced_tile_width_gives_the_same_bits(tin, tout):
    """N = 384 without LN and without stats_out under gemm_nw 1, 2, 4 (refused: 384 % 256) and 6: the K
    order of an element does not depend on the tile width."""
    M, Nn, Kk = 257, 384, D.ROWS_K[tin][2]
    c = D.base(tin, Kk, Nn)
    e = D.make_spec(tout, Nn, M, D.FORMS[1], 37)
    outs = [call(M, Nn, Kk, tin, tout, c.x, c.w, e, True, nw=nw, what=f"gemm_nw={nw}")[0] for nw in (0, 1, 2, 4, 6)]
    ref = D.linear(c.x, c.w, e, tin, tout, g=D.base_gemm(tin, Kk, Nn, DEV), M=M)
    for nw, o in zip((1, 2), outs[1:3]):
        _check(o, ref.out, ref.bound, f"out {D.rows_name(tin, tout, nw, False)} forced M={M} N={Nn} K={Kk}")
    for o in outs[1:]:
        _same_bits(outs[0], o, "gemm_nw")


def test_null_epilogue_and_no_rows():
    """epi == NULL on both kernels; M = 0 returns 0 and touches nothing."""
    n = N()
    for tin, tout in D.PAIRS:
        for M, Nn, Kk in ((129, 128, D.ROWS_K[tin][1]), (129, 72, D.TILE_K[tin][1])):
            d = D.dispatch(tin, tout, M, Nn, Kk)
            c = D.base(tin, Kk, Nn)
            got, _ = call(M, Nn, Kk, tin, tout, c.x, c.w, D.spec(), what=f"{d.name} null epi", null_epi=True)
            ref = D.linear(c.x[:M].to(DEV), c.w, None, tin, tout, d.kernel)
            _check(got, ref.out, ref.bound, f"out {d.name} null epi M={M} N={Nn} K={Kk}")
        out = torch.full((256,), SENT, dtype=tout, device=DEV)
        x = _in(torch.zeros(8, dtype=tin))
        rc = n.lib().snvrag_linear_ex(CODE[tin], CODE[tout], 0, 64, 64, n.ptr(x), 64, n.ptr(x), 64, n.ptr(out), 64, None, None,
                                      n.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and bool((out == SENT).all())


def test_training_call_sites_by_shape():
    """dX = dY W with a fused bf16 residual (autograd_ops.py) and the [M, 8] bf16 -> f32 coefficient
    gradient (128-tile kernel, no epilogue)."""
    M = 257
    c = D.base(BF16, 128, 384)
    e = D.spec(resid=D.vecs(BF16, 384).resid[:M])
    d = D.dispatch(BF16, BF16, M, 384, 128)
    got, _ = call(M, 384, 128, BF16, BF16, c.x, c.w, e, what="dX")
    ref = D.linear(c.x, c.w, e, g=D.base_gemm(BF16, 128, 384, DEV), M=M)
    _check(got, ref.out, ref.bound, f"out {d.name} dX + resid M={M} N=384 K=128")
    c = D.base(BF16, 384, 8)
    d = D.dispatch(BF16, F32, M, 8, 384)
    assert d.name == D.tile_name(BF16, F32)
    got, _ = call(M, 8, 384, BF16, F32, c.x, c.w, D.spec(), what="coef grad", null_epi=True)
    ref = D.linear(c.x[:M].to(DEV), c.w, None, BF16, F32, "tile")
    _check(got, ref.out, ref.bound, f"out {d.name} [M, 8] coefficient gradient M={M} N=8 K=384")
