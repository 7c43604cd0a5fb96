"""The training LayerNorm family and the bf16 column sum (csrc/train.hip: ln_fwd_train_kernel<1..4>,
ln_fwd_train_g16<1..4>, ln_bwd_kernel<1..4, 1>, ln_bwd_pf_kernel<2..4>, ln_part_sum_kernel,
colsum_part_kernel, colsum_f32_kernel) through the C ABI, against the fp64 references of
tests/ln_refs.py within its derived per-element bounds, at every chunk, row and reduction-loop
edge (test_ln_refs_cpu.py proves the references, the bounds, their teeth and that each shape of
the tables reaches the branch it is there for).

Every input is a prefix view of NaN-padded storage (an over-read shows up as NaN); every output
lives in sentinel-filled storage with one guard row (or 16 guard elements) that must be unchanged
afterwards; dg / db are NaN before an overwriting call and hold known values before an
accumulating one; the workspace is NaN-filled and guarded too.  The backward is isolated: it is
given the s and the f32 statistics of the reference, not the forward kernel's.  max err / bound is
printed per case."""
from types import SimpleNamespace

import pytest
import torch

import ln_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -776.0                      # bf16-exact sentinel
PAD = 4096                         # NaN elements behind every input
GUARD = 16                         # guard elements behind dg / db / the column sums / the workspace


def K():
    from src import kernels
    return kernels


def N():
    from src import native
    return native


# ------------------------------------------------------------- guarded calls --
def _in(t):
    if t is None:
        return None
    return torch.cat([t.reshape(-1), torch.full((PAD,), float("nan"), dtype=t.dtype)]).to(DEV)


def _out(rows, cols, dtype):
    return torch.full(((rows + 1) * cols,), SENT, dtype=dtype, device=DEV)


def _take(buf, rows, cols, what):
    v = buf.cpu()
    assert bool((v[rows * cols:] == SENT).all()), f"{what}: wrote past its {rows} x {cols} block"
    return v[:rows * cols].view(rows, cols).clone()


def _vec(n, fill):
    """f32 [n] + GUARD sentinels; fill: NaN (must be overwritten) or the values to accumulate into."""
    head = torch.full((n,), float("nan"), dtype=F32) if fill is None else fill.to(F32)
    return torch.cat([head, torch.full((GUARD,), SENT, dtype=F32)]).to(DEV)


def _take_vec(buf, n, what):
    v = buf.cpu()
    assert bool((v[n:] == SENT).all()), f"{what}: wrote past its {n} elements"
    return v[:n].clone()


def _ws(nbytes):
    return torch.full((nbytes // 4 + GUARD,), float("nan"), dtype=F32, device=DEV)


def fwd_raw(c, rows1=0, **ov):
    """(status, y, s_out, stats buffers); ov overrides N / slopes for the argument checks."""
    n = N()
    M, Nn = c.M, ov.get("N", c.N)
    ins = [_in(c.x), _in(c.r), _in(c.g), _in(c.b)]
    y, st = _out(M, c.N, BF16), _out(M, 2, F32)
    s = _out(M, c.N, BF16) if c.r is not None else None
    with K().option("ln_rows1", rows1):
        rc = n.lib().snvrag_ln_fwd_train_act(M, Nn, n.ptr(ins[0]), n.ptr(ins[1]), n.ptr(ins[2]), n.ptr(ins[3]), c.eps,
                                             n.ptr(y), n.ptr(s), n.ptr(st), c.p_r, c.p_out, c.seed,
                                             ov.get("slope_x", c.slope_x), ov.get("slope_r", c.slope_r), n.stream_ptr())
    torch.cuda.synchronize()
    return rc, y, s, st


def ln_fwd(c, rows1=0):
    rc, y, s, st = fwd_raw(c, rows1)
    N().check(rc, "ln_fwd_train_act")
    return (_take(y, c.M, c.N, "y"), None if s is None else _take(s, c.M, c.N, "s_out"), _take(st, c.M, 2, "stats"))


def bwd_raw(c, nopf=0, prefill=None, **ov):
    """(status, ds, dres, dg, db, workspace, workspace bytes)."""
    n = N()
    M, Nn = c.M, ov.get("N", c.N)
    ins = [_in(c.dy), _in(c.s), _in(c.stats), _in(c.g), _in(c.r) if ov.get("r_pre", c.slope_r != 0.0) else None]
    ds = _out(M, c.N, BF16)
    dres = _out(M, c.N, BF16) if (c.p_r > 0 or c.slope_r != 0.0) else None
    dg = _vec(c.N, None if prefill is None else prefill[0])
    db = _vec(c.N, None if prefill is None else prefill[1])
    wsb = n.lib().snvrag_ln_bwd_ws_bytes(M, c.N)
    ws = _ws(wsb)
    with K().option("ln_bwd_nopf", nopf):
        rc = n.lib().snvrag_ln_bwd_act(M, Nn, n.ptr(ins[0]), n.ptr(ins[1]), n.ptr(ins[2]), n.ptr(ins[3]), n.ptr(ds),
                                       n.ptr(dres), n.ptr(ins[4]), n.ptr(dg), n.ptr(db), 0 if prefill is None else 1,
                                       c.p_r, c.p_out, c.seed, c.slope_x, ov.get("slope_r", c.slope_r), n.ptr(ws),
                                       wsb - ov.get("ws_short", 0), n.stream_ptr())
    torch.cuda.synchronize()
    return rc, ds, dres, dg, db, ws, wsb


def ln_bwd(c, nopf=0, prefill=None):
    rc, ds, dres, dg, db, ws, wsb = bwd_raw(c, nopf, prefill)
    N().check(rc, "ln_bwd_act")
    assert bool(torch.isnan(ws[wsb // 4:]).all()), "wrote past the workspace"
    return SimpleNamespace(ds=_take(ds, c.M, c.N, "ds"), dres=None if dres is None else _take(dres, c.M, c.N, "dres"),
                           dg=_take_vec(dg, c.N, "dg"), db=_take_vec(db, c.N, "db"))


def colsum_raw(x, M, Nn, ws_short=0):
    n = N()
    xin, out = _in(x), _vec(x.shape[1], None)
    wsb = n.lib().snvrag_colsum_ws_bytes(M, x.shape[1])
    ws = _ws(wsb)
    rc = n.lib().snvrag_colsum_bf16(M, Nn, n.ptr(xin), n.ptr(out), n.ptr(ws), wsb - ws_short, n.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, ws, wsb


def _check(got, ref, bound, what):
    r = R.ratio(got, ref, bound)
    print(f"{what}: max err/bound {r:.3f}")
    assert r <= 1.0, what
    return r


# ----------------------------------------------------------------- checkers --
def check_forward(c, rows1, kernel):
    d = R.fwd_dispatch(c.M, c.N, rows1)
    assert d["kernel"] == kernel
    y, s, st = ln_fwd(c, rows1)
    ref = R.forward(c)
    by, _, bm, br = R.forward_bounds(c, ref, d["lanes"], d["nch"])
    tag = f"{kernel}<{d['inst']}> M={c.M} N={c.N} {c.mode}"
    _check(y, ref.y, by, f"y {tag}")
    _check(st[:, 0], ref.mean, bm, f"mean {tag}")
    _check(st[:, 1], ref.rstd, br, f"rstd {tag}")
    if c.res:
        _check(s, c.s64, R.bf16_ulp(c.s64) / 2 + R.C["s"] * R.U * c.A_s, f"s {tag}")
    if c.keep_o is not None:
        assert bool((y[~c.keep_o] == 0).all()) and bool((y[c.keep_o & (ref.y != 0)] != 0).all()), f"output mask {tag}"
    if c.keep_r is not None:
        assert torch.equal(s[~c.keep_r], c.xa[~c.keep_r]), f"residual mask {tag}"


def check_backward(c, nopf=0, accumulate=False):
    d = R.bwd_dispatch(c.M, c.N, nopf)
    pre = None
    if accumulate:
        pre = (torch.linspace(-3, 3, c.N), torch.linspace(2, -2, c.N))
    got = ln_bwd(c, nopf, pre)
    ref = R.backward(c)
    bds, _, bdr, _, bdg, bdb = R.backward_bounds(c, ref, d["depth"], *(pre or (None, None)))
    tag = f"{d['kernel']}<{d['inst']}> M={c.M} N={c.N} {c.mode} acc={int(accumulate)}"
    _check(got.ds, ref.ds, bds, f"ds {tag}")
    assert (got.dres is None) == (ref.dres is None)
    if ref.dres is not None:
        _check(got.dres, ref.dres, bdr, f"dres {tag}")
        if c.keep_r is not None:
            assert bool((got.dres[~c.keep_r] == 0).all()), f"residual mask {tag}"
    _check(got.dg, ref.dg + (pre[0].to(F64) if pre else 0), bdg, f"dg {tag}")
    _check(got.db, ref.db + (pre[1].to(F64) if pre else 0), bdb, f"db {tag}")


# ------------------------------------------------------------------ forward --
@pytest.mark.parametrize("Nn", R.ROW_N)
def test_forward_one_row_per_wave(Nn):
    """ln_fwd_train_kernel<1..4> (ln_rows1 = 1 keeps N = 512 on it): 1, 8, 17, 63 and 64 live
    lanes in the last chunk, M on both sides of the 4-row block."""
    for M, n, mode in R.fwd_row_cases():
        if n == Nn:
            check_forward(R.build(M, n, mode), 1, "row")


@pytest.mark.parametrize("Nn", R.G16_N)
def test_forward_16_lane_groups(Nn):
    """ln_fwd_train_g16<1..4>: rows on both sides of the 4-row wave and the 16-row block (the idle
    groups' loads are clamped to row M - 1, their stores guarded)."""
    for M, n, mode in R.fwd_g16_cases():
        if n == Nn:
            check_forward(R.build(M, n, mode), 0, "g16")


@pytest.mark.parametrize("M,Nn", R.EXACT_ROW + R.EXACT_G16)
def test_forward_position_coded_exact(M, Nn):
    """Every y[m, n] is a bf16-exact number that names its column, its row's sign code names (row,
    chunk): bit for bit, for every forward instance, M straddling a block."""
    c = R.exact_case(M, Nn)
    c.p_r = c.p_out = c.slope_x = c.slope_r = 0.0
    c.seed = R.SEED
    y, s, st = ln_fwd(c, 0)
    assert torch.equal(s, c.s), "s_out"
    assert torch.equal(st[:, 0].to(F64), c.mean), "mean"
    _check(st[:, 1], c.rstd, c.rstd * 5 * R.U, f"rstd M={M} N={Nn}")
    bad = (y.view(torch.int16) != c.y.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"y differs first at (row, column) {bad[0].tolist()}"


# ----------------------------------------------------------------- backward --
@pytest.mark.parametrize("Nn,nopf", [(n, 0) for n in R.ROW_N] + [(n, 1) for n in R.ROW_N if n > 512])
def test_backward(Nn, nopf):
    """ln_bwd_kernel<1..4, 1> (N <= 512, or ln_bwd_nopf = 1) and ln_bwd_pf_kernel<2..4>: M = 1
    (three waves without a row), 31 / 32 / 33 (a short wave; an empty one at 33), 45 (two blocks
    at 6 rows per wave), 257 (9 blocks); N = 2048 asks for exactly 64 KiB of dynamic LDS."""
    for M, n, mode in R.bwd_cases():
        if n == Nn:
            check_backward(R.build(M, n, mode), nopf)


@pytest.mark.parametrize("M,Nn,mode", R.CAP)
def test_backward_past_the_block_cap(M, Nn, mode):
    """nblk = 2048, 9 rows per wave, 906 waves without a row."""
    check_backward(R.build(M, Nn, mode))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("Rr", R.PART_R)
def test_part_sum_edges(Rr, acc):
    """ln_part_sum_kernel over R = M / 32 block partials: both sides of every trip count of its
    four-way unrolled loop and of its tail; written, and added to known values."""
    check_backward(R.build(32 * Rr, 8, "p_out"), 0, bool(acc))


# -------------------------------------------------------------------- modes --
@pytest.mark.parametrize("mode", R.MODE_NAMES)
@pytest.mark.parametrize("M,Nn", R.MODE_SHAPES)
def test_modes(M, Nn, mode):
    """No residual, residual, either dropout, both, and the fused LeakyReLUs (inputs hold +0.0 and
    -0.0), forward on the kernel the dispatch picks and backward overwriting and accumulating."""
    c = R.build(M, Nn, mode)
    check_forward(c, 0, R.fwd_dispatch(M, Nn)["kernel"])
    check_backward(c, 0, False)
    check_backward(c, 0, True)


# --------------------------------------------------------------- column sums --
def check_colsum(M, Nn):
    x = R.colsum_input(M, Nn)
    d = R.colsum_dispatch(M, Nn)
    rc, out, ws, wsb = colsum_raw(x, M, Nn)
    N().check(rc, "colsum_bf16")
    assert bool(torch.isnan(ws[wsb // 4:]).all()), "wrote past the workspace"
    _check(_take_vec(out, Nn, "colsum"), R.colsum(x), R.colsum_bound(x, d["depth"]), f"colsum M={M} N={Nn}")


@pytest.mark.parametrize("Nn", R.COLSUM_N)
def test_colsum_thread_mapping(Nn):
    """per = 256 / nc row lanes: 256, 85 (+ 1 idle thread), 5, 3, 1 (+ 127 idle), 1; M = 0 is the
    memset path, 257 two blocks."""
    for M in R.COLSUM_M:
        check_colsum(M, Nn)


@pytest.mark.parametrize("M", [256 * r for r in R.COLSUM_R] + [R.COLSUM_BIG_M])
def test_colsum_reduction_edges(M):
    """colsum_f32_kernel over 15 .. 1024 block partials; 262 444 rows: 257 rows a block."""
    check_colsum(M, 8)


# ---------------------------------------------------------- argument checks --
def _all_sentinel(*bufs):
    for b in bufs:
        if b is not None:
            v = b.cpu()
            assert bool(((v == SENT) | torch.isnan(v)).all()), "a rejected call wrote an output"


def _plain(M, Nn, res):
    gen = torch.Generator().manual_seed(Nn)
    mk = lambda: torch.randn(M, Nn, generator=gen).to(BF16)
    c = SimpleNamespace(M=M, N=Nn, x=mk(), r=mk() if res else None, dy=mk(), g=torch.ones(Nn), b=torch.zeros(Nn),
                        eps=R.f32(R.EPS), p_r=0.0, p_out=0.0, seed=R.SEED, slope_x=0.0, slope_r=0.0)
    c.s, c.stats = c.x, torch.ones(M, 2)
    return c


@pytest.mark.parametrize("Nn", [12, 2056])
def test_rejects_bad_widths(Nn):
    c = _plain(4, 2056, True)
    rc, *bufs = fwd_raw(c, N=Nn)
    assert rc != 0
    _all_sentinel(*bufs)
    rc, ds, dres, dg, db, ws, _ = bwd_raw(c, N=Nn)
    assert rc != 0
    _all_sentinel(ds, dres, dg, db, ws)
    rc, out, ws, _ = colsum_raw(c.x, 4, Nn)
    assert rc != 0
    _all_sentinel(out, ws)


def test_rejects_bad_activations_and_short_workspaces():
    c = _plain(33, 136, True)
    for ov in (dict(slope_x=0.05), ):                          # an input activation with a residual
        rc, *bufs = fwd_raw(c, **ov)
        assert rc != 0
        _all_sentinel(*bufs)
    rc, *bufs = fwd_raw(_plain(33, 136, False), slope_r=0.05)  # a residual activation without one
    assert rc != 0
    _all_sentinel(*bufs)
    c.slope_r = R.f32(0.05)                                    # dres is passed, the pre-activation r is not
    rc, ds, dres, dg, db, ws, _ = bwd_raw(c, r_pre=False)
    assert rc != 0 and dres is not None
    _all_sentinel(ds, dres, dg, db, ws)
    c.slope_r = 0.0
    rc, ds, dres, dg, db, ws, _ = bwd_raw(c, ws_short=1)
    assert rc != 0
    _all_sentinel(ds, dres, dg, db, ws)
    rc, out, ws, _ = colsum_raw(c.x, 33, 136, ws_short=1)
    assert rc != 0
    _all_sentinel(out, ws)
