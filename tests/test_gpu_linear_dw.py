"""The weight-gradient kernel (csrc/dw.hip: dw_dma_kernel<DET>, dw_reduce_kernel) through the C ABI
snvrag_linear_dw, snvrag_linear_dw_parts, snvrag_linear_dw_det and snvrag_linear_dw_parts_det, per
element against the fp64 reference of tests/dw_refs.py: every exit of the 4-slot stage ring (1 to 10,
12 and 13 stages), every row tail of a DMA piece and an MFMA half, short last chunks, fewer chunks than
splits, one-stage chunks, the reduce loop's unroll remainders (S = 1, 2, 3, 4, 5, 9), N != K tiles, grids
of 2 to 24 workgroups on both sides of the 8-XCD remap, 2 to 4 output parts with and without db, padded
and sliced leading dimensions, accumulation onto a prior value, M = 0, and the host's chunking
(tests/test_dw_refs_cpu.py proves the reference, the bounds, their teeth and the shape table).

dy and x are prefixes of NaN-continued storage sized exactly; padding columns, and the columns outside
a slice, are NaN; every dW / db buffer or part is allocated on its own with a sentinel guard behind it
that must be unchanged; the deterministic workspace is exactly snvrag_linear_dw_det_ws_bytes long with a
guard behind it.  Every case runs with dw_xcd 0 and 1, atomic and deterministic, twice.  The exact
inputs (integers: the bound is 0) must equal the fp64 result bit for bit in every one of those runs; the
random inputs must stay within bound_w / bound_b, the deterministic runs equal to each other bit for
bit.  max err / bound is printed per case.

Largest max err / bound on the MI355X (pytest -s): ring, tail, chunk, tile, parts and ld (exact inputs)
0.000, bit-equal in every run; random dW 0.018, db 0.004; scaled dW 0.037, db 0.017 (the bound is a worst
case, one rounding per product all of one sign: random roundings reach a few hundredths of it)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import dw_refs as R
from test_gpu_stream_gemm import DEV, PAD, SENT, K, N

pytestmark = pytest.mark.gpu

BF16, F32, F64 = R.BF16, R.F32, R.F64
NAN = float("nan")
GUARD = 1024
ENTRIES = ("snvrag_linear_dw", "snvrag_linear_dw_parts", "snvrag_linear_dw_det", "snvrag_linear_dw_parts_det")


# ------------------------------------------------------------- guarded calls --
def _store(t, ld, off):
    """[M, C] bf16 values at columns off .. off + C of M rows of ld elements; every other element, and
    what follows row M - 1, NaN.  (storage, address of element [0, off])."""
    M, Cc = t.shape
    buf = torch.full((M * ld + PAD,), NAN, dtype=BF16, device=DEV)
    if M:
        buf[:M * ld].view(M, ld)[:, off:off + Cc] = t.to(DEV)
    return buf, buf.data_ptr() + 2 * off


def _operands(c, dy, x):
    ldy, oy, _, ldx, ox, _ = R.lds(c)
    sy, py = _store(dy, ldy, oy)
    sx, px = _store(x, ldx, ox)
    return SimpleNamespace(sy=sy, py=py, ldy=ldy, sx=sx, px=px, ldx=ldx)


def _guarded(n, init):
    """n f32 values (init: [n] or None = zeros) with a sentinel guard behind them."""
    buf = torch.full((n + GUARD,), SENT, dtype=F32, device=DEV)
    buf[:n] = 0.0 if init is None else init.reshape(-1).to(DEV)
    return buf


def _take(buf, n, what):
    v = buf.cpu()
    assert bool((v[n:] == SENT).all()), f"{what}: wrote past its {n} elements"
    return v[:n].clone()


def _arr(bufs):
    a = (C.c_void_p * 4)()
    for i, b in enumerate(bufs):
        a[i] = b.data_ptr()
    return a


def launch(c, ops, det, xcd, pw=None, pb=None, what=""):
    """One guarded launch of the entry point the case calls for: (dW [N, K], db [N] or None) on the CPU."""
    n, lib = N(), N().lib()
    seg = c.N // c.parts
    ws_ = [_guarded(seg * c.K, None if pw is None else pw[i * seg:(i + 1) * seg]) for i in range(c.parts)]
    bs_ = [_guarded(seg, None if pb is None else pb[i * seg:(i + 1) * seg]) for i in range(c.parts)] if c.db else None
    head = (c.M, c.N, c.K, ops.py, ops.ldy, ops.px, ops.ldx)
    out = (n.ptr(ws_[0]), n.ptr(bs_[0]) if c.db else None) if c.parts == 1 else \
        (c.parts, _arr(ws_), _arr(bs_) if c.db else None)
    ws = None
    with K().option("dw_xcd", xcd):
        if det:
            nbytes = int(lib.snvrag_linear_dw_det_ws_bytes(c.M, c.N, c.K, c.splits))
            assert nbytes == R.chunks(c.M, c.N, c.K, c.splits).ws_bytes and nbytes % 16 == 0
            ws = torch.full((nbytes // 4 + GUARD,), SENT, dtype=F32, device=DEV)
            fn = lib.snvrag_linear_dw_det if c.parts == 1 else lib.snvrag_linear_dw_parts_det
            rc = fn(*head, *out, c.splits, n.ptr(ws) if nbytes else None, nbytes, n.stream_ptr())
        else:
            fn = lib.snvrag_linear_dw if c.parts == 1 else lib.snvrag_linear_dw_parts
            rc = fn(*head, *out, c.splits, n.stream_ptr())
    n.check(rc, f"{fn.__name__} {what}")
    torch.cuda.synchronize()
    if ws is not None:
        assert bool((ws[ws.numel() - GUARD:] == SENT).all()), f"{what}: wrote past the workspace"
    w = torch.cat([_take(b, seg * c.K, f"dW part {i} {what}") for i, b in enumerate(ws_)]).view(c.N, c.K)
    b = torch.cat([_take(b, seg, f"db part {i} {what}") for i, b in enumerate(bs_)]) if c.db else None
    return w, b


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bit_equal(got, want, what):
    bad = (_bits(got) != _bits(want)).nonzero()
    if bad.numel():
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: [{i}] = {float(got[i])}, expected {float(want[i])}; {bad.shape[0]} elements differ")


WORST = {}


def _ratio(c, kind, got, ref, bound, what):
    r = R.ratio(got, ref, bound)
    print(f"{what} {kind}: max err/bound {r:.3f}")
    WORST[(c.fam, kind)] = max(WORST.get((c.fam, kind), 0.0), r)
    assert r <= 1.0, f"{what} {kind}"


def _to_cpu(r):
    return R.Ref(*(t.cpu() for t in r))


def run_exact(c):
    """Every run of an exact case equals the fp64 result bit for bit: zero start and onto the integer
    prior, dw_xcd 0 and 1, atomic and deterministic, two launches."""
    dy, x, pw, pb = R.inputs(c)
    ch = R.chunks(c.M, c.N, c.K, c.splits)
    for key, val in c.want.items():
        assert dict(chunk=ch.chunk, S=ch.S, last=ch.rows[-1], nst=ch.stages[0], grid=ch.grid)[key] == val, (c.id, key)
    ops = _operands(c, dy, x)
    r0, r1 = _to_cpu(R.ref(dy.to(DEV), x.to(DEV))), _to_cpu(R.ref(dy.to(DEV), x.to(DEV), pw, pb))
    assert not R.bound_w(dy, x, ch, pw).any() and not R.bound_b(dy, ch, pb).any(), "exact inputs: the bound is 0"
    zero_w, zero_b = torch.zeros(c.N, c.K, dtype=F64), torch.zeros(c.N, dtype=F64)
    for xcd in (0, 1):
        for det in (False, True):
            for tag, r, prior in (("first", r0, (None, None)), ("again", r0, (None, None)), ("prior", r1, (pw, pb))):
                what = f"{c.id} S={ch.S} grid={ch.grid} xcd={xcd} {'det' if det else 'atomic'} {tag}"
                w, b = launch(c, ops, det, xcd, *prior, what=what)
                _ratio(c, "dW", w, r.w, zero_w, what)
                _bit_equal(w, r.w.to(F32), f"dW {what}")
                if c.db:
                    _ratio(c, "db", b, r.b, zero_b, what)
                    _bit_equal(b, r.b.to(F32), f"db {what}")
                else:
                    assert b is None


def run_random(c):
    """Within the derived bounds in every run; the deterministic runs bit-equal across launches and
    dw_xcd, and onto a prior bit-equal to prior + (zero-start result) in f32."""
    dy, x, pw, pb = R.inputs(c)
    ch = R.chunks(c.M, c.N, c.K, c.splits)
    ops = _operands(c, dy, x)
    dyd, xd = dy.to(DEV), x.to(DEV)
    r0, r1 = _to_cpu(R.ref(dyd, xd)), _to_cpu(R.ref(dyd, xd, pw, pb))
    bw0, bb0 = R.bound_w(dyd, xd, ch).cpu(), R.bound_b(dyd, ch).cpu()
    bw1, bb1 = R.bound_w(dyd, xd, ch, pw).cpu(), R.bound_b(dyd, ch, pb).cpu()
    assert bool((bw0 > 0).all() and (bb0 > 0).all())
    det0 = None
    for xcd in (0, 1):
        for det in (False, True):
            got = {}
            for tag, r, bw, bb, prior in (("first", r0, bw0, bb0, (None, None)), ("again", r0, bw0, bb0, (None, None)),
                                          ("prior", r1, bw1, bb1, (pw, pb))):
                what = f"{c.id} S={ch.S} grid={ch.grid} xcd={xcd} {'det' if det else 'atomic'} {tag}"
                w, b = launch(c, ops, det, xcd, *prior, what=what)
                _ratio(c, "dW", w, r.w, bw, what)
                _ratio(c, "db", b, r.b, bb, what)
                got[tag] = (w, b)
            if det or ch.S == 1:                           # one add per element: nothing left to the atomics' order
                _bit_equal(got["again"][0], got["first"][0], f"{c.id} xcd={xcd} det={det}: two launches, dW")
                _bit_equal(got["again"][1], got["first"][1], f"{c.id} xcd={xcd} det={det}: two launches, db")
            if det:
                _bit_equal(got["prior"][0], pw + got["first"][0], f"{c.id} xcd={xcd}: prior + zero-start result, dW")
                _bit_equal(got["prior"][1], pb + got["first"][1], f"{c.id} xcd={xcd}: prior + zero-start result, db")
                det0 = det0 or got["first"]
                _bit_equal(got["first"][0], det0[0], f"{c.id}: dw_xcd 0 and 1, dW")
                _bit_equal(got["first"][1], det0[1], f"{c.id}: dw_xcd 0 and 1, db")


# -------------------------------------------------------------------- sweeps --
def test_ring_exits_exact():
    """N = K = 128, one chunk of 1 .. 10, 12, 13 stages: the prologue's min(3, nst), the unrolled loop's
    exit, every slot of the tail loop's switch and every counted vmcnt wait."""
    for c in R.cases("ring"):
        run_exact(c)


def test_row_tails_exact():
    """M = 128 + r: the last stage holds r rows, the rest of it must read the resource's zeros."""
    for c in R.cases("tail"):
        run_exact(c)


def test_chunking_exact():
    """Short last chunks, fewer chunks than splits, one-stage chunks, the auto-split path, and the reduce
    kernel's loop at S = 2, 3, 4, 5, 9; onto a prior in both modes."""
    for c in R.cases("chunk"):
        run_exact(c)


_TILE_NK = sorted({(c.N, c.K) for c in R.cases("tile")})


@pytest.mark.parametrize("Nn,Kk", _TILE_NK, ids=[f"{a}x{b}" for a, b in _TILE_NK])
def test_tiles_exact(Nn, Kk):
    """N != K, several tiles each way, grids of 2 .. 24 workgroups: n0 / k0, the (wn, wk) sub-tiles, db from
    the k0 == 0 tiles alone, and the XCD remap at grids below, at and beyond 8 that are no multiple of 8."""
    for c in R.cases("tile"):
        if (c.N, c.K) == (Nn, Kk):
            run_exact(c)


@pytest.mark.parametrize("Nn,parts", R.PARTS, ids=[f"{a}in{b}" for a, b in R.PARTS])
def test_parts_exact(Nn, parts):
    """part = n0 / seg and nbase in both kernels, with and without db."""
    for c in R.cases("parts"):
        if (c.N, c.parts) == (Nn, parts):
            run_exact(c)


def test_leading_dimensions_exact():
    """ldy = N + 8, ldx = K + 8; dy and x as column slices at 128 and at N / K of a three times wider tensor."""
    for c in R.cases("ld"):
        run_exact(c)


_RANDOM = R.random_cases()


@pytest.mark.parametrize("c", _RANDOM, ids=[c.id for c in _RANDOM])
def test_random_within_bound(c):
    run_random(c)


def test_worst_ratios_reported():
    """(after the sweeps, for the record under profiles/)"""
    for (fam, kind), r in sorted(WORST.items()):
        print(f"worst {fam:8s} {kind}: {r:.3f}")


# ---------------------------------------------------------- additional cases --
def test_m_zero_touches_nothing():
    n, lib = N(), N().lib()
    nan = torch.full((PAD,), NAN, dtype=BF16, device=DEV)
    w = [torch.full((128 * 128 + GUARD,), SENT, dtype=F32, device=DEV) for _ in range(2)]
    b = [torch.full((128 + GUARD,), SENT, dtype=F32, device=DEV) for _ in range(2)]
    head = (0, 256, 128, n.ptr(nan), 256, n.ptr(nan), 128)
    for splits in (0, 3):
        assert lib.snvrag_linear_dw_det_ws_bytes(0, 256, 128, splits) == 0
        n.check(lib.snvrag_linear_dw(*head, n.ptr(w[0]), n.ptr(b[0]), splits, n.stream_ptr()), "M = 0")
        n.check(lib.snvrag_linear_dw_parts(*head, 2, _arr(w), _arr(b), splits, n.stream_ptr()), "M = 0 parts")
        n.check(lib.snvrag_linear_dw_det(*head, n.ptr(w[0]), n.ptr(b[0]), splits, None, 0, n.stream_ptr()), "M = 0 det")
        n.check(lib.snvrag_linear_dw_parts_det(*head, 2, _arr(w), _arr(b), splits, None, 0, n.stream_ptr()), "M = 0 parts det")
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in w + b)


def test_host_chunking_matches_the_restatement():
    lib = N().lib()
    for M, Nn, Kk, splits in R.HOST_TABLE:
        ch = R.chunks(M, Nn, Kk, splits)
        assert lib.snvrag_dw_splits(M, Nn, Kk) == R.dw_splits(M, Nn, Kk), (M, Nn, Kk)
        assert lib.snvrag_linear_dw_det_ws_bytes(M, Nn, Kk, splits) == ch.ws_bytes, (M, Nn, Kk, splits)
    assert {(49440, a, b, 0) for a, b in ((1152, 384), (384, 384), (1536, 384), (384, 1536))} <= set(R.HOST_TABLE)


def test_det_parts_reject_db_for_some_parts_only():
    n, lib = N(), N().lib()
    c = next(c for c in R.cases("parts") if c.db and c.parts == 3)
    dy, x, _, _ = R.inputs(c)
    ops = _operands(c, dy, x)
    seg = c.N // 3
    ws_ = [torch.zeros(seg * c.K, device=DEV) for _ in range(3)]
    bs_ = [torch.zeros(seg, device=DEV) for _ in range(3)]
    nbytes = int(lib.snvrag_linear_dw_det_ws_bytes(c.M, c.N, c.K, c.splits))
    ws = torch.zeros(nbytes // 4, device=DEV)
    some = _arr(bs_)
    some[1] = None
    for fn, tail in ((lib.snvrag_linear_dw_parts_det, (n.ptr(ws), nbytes, n.stream_ptr())), (lib.snvrag_linear_dw_parts, (n.stream_ptr(),))):
        rc = fn(c.M, c.N, c.K, ops.py, ops.ldy, ops.px, ops.ldx, 3, _arr(ws_), some, c.splits, *tail)
        assert rc != 0 and lib.snvrag_last_error().decode() == "dw_parts_out: null db part"
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in ws_ + bs_ + [ws])


def test_linear_dw_rejects_spans_past_int32():
    """The kernel carries M as int and addresses a chunk's rows with 32-bit byte offsets: M = 2^31, and a
    chunk of 2^20 rows of 1152 elements (2.25 GiB), are refused by all four entry points before any
    launch, not truncated or clamped."""
    n, lib = N(), N().lib()
    dy, x = torch.zeros(1, 1152, device=DEV, dtype=BF16), torch.zeros(1, 128, device=DEV, dtype=BF16)
    w, b = [torch.zeros(128, 128, device=DEV) for _ in range(4)], [torch.zeros(128, device=DEV) for _ in range(4)]
    span = "dw_plan: a chunk of rows spans 2 GiB or more (32-bit DMA offsets): use more splits"
    for M, ldy, splits, msg in ((2 ** 31, 128, 0, "dw_check: bad M"), (2 ** 31, 128, 1, "dw_check: bad M"), (2 ** 20, 1152, 1, span)):
        nbytes = int(lib.snvrag_linear_dw_det_ws_bytes(M, 128, 128, splits))
        assert nbytes == R.chunks(M, 128, 128, splits).ws_bytes
        ws = torch.zeros(nbytes // 4, device=DEV)
        head = (M, 128, 128, n.ptr(dy), ldy, n.ptr(x), 128)
        for name in ENTRIES:
            out = (1, _arr(w[:1]), _arr(b[:1])) if "parts" in name else (n.ptr(w[0]), n.ptr(b[0]))
            tail = (n.ptr(ws), nbytes, n.stream_ptr()) if name.endswith("det") else (n.stream_ptr(),)
            rc = getattr(lib, name)(*head, *out, splits, *tail)
            assert rc != 0 and lib.snvrag_last_error().decode() == msg, (name, M, lib.snvrag_last_error().decode())
        torch.cuda.synchronize()
        assert not any(bool(t.any()) for t in w + b + [ws])
    # the same rows in enough chunks are addressable: the plan accepts what the check is not about
    assert R.chunks(2 ** 20, 128, 128, 2).chunk * 1152 * 2 < 2 ** 31
