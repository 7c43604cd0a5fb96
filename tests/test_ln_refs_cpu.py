"""CPU proofs behind tests/test_gpu_layernorm_train.py (tests/ln_refs.py): the fp64 restatement is
torch's fp64 autograd of layer_norm with the LeakyReLUs and the explicit masks; a plain f32
evaluation meets every bound on every input set the GPU tests use (a miss there is the kernel's);
the constants C are 4 times what is measured here; the exact cases are exact in f32 whatever the
last bits of rstd; the shape tables reach the branches they name; and the bounds have teeth: four
single-fault perturbations of the f32 evaluation each fail their check."""
import copy

import pytest
import torch
import torch.nn.functional as F

import ln_refs as R

F64, F32, BF16 = R.F64, R.F32, R.BF16


# ------------------------------------------------ a. reference == torch autograd --
@pytest.mark.parametrize("mode", R.MODE_NAMES)
@pytest.mark.parametrize("M,N", [(5, 136), (33, 384)])
def test_reference_matches_torch_fp64_autograd(M, N, mode):
    """Forward, dx, dr, dg, db.  The bf16 roundings of xa, ra and s are carried through autograd
    as straight-through constants; the backward is given the fp64 statistics here (its f32 ones
    are an input of the isolated reference, not part of the operation).  The inputs hold +0.0 and
    -0.0 under both slopes."""
    c = copy.copy(R.build(M, N, mode))
    for t in (c.x, c.r):
        if t is not None:
            z = t.view(torch.int16)
            assert bool((z == 0).any()) and bool((z == -32768).any()), "inputs lack +0.0 / -0.0"
    x = c.x.to(F64).requires_grad_()
    g, b = c.g.to(F64).requires_grad_(), c.b.to(F64).requires_grad_()
    xa = F.leaky_relu(x, c.slope_x) if c.slope_x else x
    xa = xa + (c.xa.to(F64) - xa).detach()
    s, r = xa, None
    if c.res:
        r = c.r.to(F64).requires_grad_()
        ra = F.leaky_relu(r, c.slope_r) if c.slope_r else r
        ra = ra + (c.ra.to(F64) - ra).detach()
        s = xa + ra * R._keep(c.keep_r, c.sc_r, x.shape, F64)
        s = s + (c.s.to(F64) - s).detach()
    y = F.layer_norm(s, (N,), g, b, c.eps) * R._keep(c.keep_o, c.sc_o, x.shape, F64)
    y.backward(c.dy.to(F64))
    f = R.forward(c, F64)
    c.stats = torch.stack([f.mean, f.rstd], -1)
    bw = R.backward(c, F64)
    tol = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(f.y, y.detach(), **tol)
    torch.testing.assert_close(bw.ds, x.grad, **tol)
    if c.res:
        torch.testing.assert_close(bw.ds if bw.dres is None else bw.dres, r.grad, **tol)
    torch.testing.assert_close(bw.dg, g.grad, **tol)
    torch.testing.assert_close(bw.db, b.grad, **tol)


# ---------------------------------------- b. f32 meets every bound; constants --
def f32_ratios(c, accumulate=False):
    """max err / bound of every output of the f32 evaluation of one input set."""
    out = {}
    f64 = R.forward(c, F64)
    if c.res:
        out["s"] = R.ratio(c.s, c.s64, R.bf16_ulp(c.s64) / 2 + R.C["s"] * R.U * c.A_s)
    for rows1 in (0, 1):
        d = R.fwd_dispatch(c.M, c.N, rows1)
        f = R.forward(c, F32, d["lanes"])
        by, _, bm, br = R.forward_bounds(c, f64, d["lanes"], d["nch"])
        k = d["kernel"]
        out[f"y/{k}"] = R.ratio(R.to_bf16(f.y), f64.y, by)
        out[f"mean/{k}"] = R.ratio(f.mean, f64.mean, bm)
        out[f"rstd/{k}"] = R.ratio(f.rstd, f64.rstd, br)
    b64, b32 = R.backward(c, F64), R.backward(c, F32)
    pg = pb = None
    if accumulate:
        pg, pb = torch.linspace(-3, 3, c.N), torch.linspace(2, -2, c.N)
    bds, _, bdr, _, bdg, bdb = R.backward_bounds(c, b64, R.bwd_dispatch(c.M, c.N)["depth"], pg, pb)
    out["ds"] = R.ratio(R.to_bf16(b32.ds), b64.ds, bds)
    if b64.dres is not None:
        out["dres"] = R.ratio(R.to_bf16(b32.dres), b64.dres, bdr)
    add = (lambda t, p: t) if not accumulate else (lambda t, p: t + p.to(t.dtype))
    out["dg"] = R.ratio(add(b32.dg, pg), add(b64.dg, pg), bdg)
    out["db"] = R.ratio(add(b32.db, pb), add(b64.db, pb), bdb)
    return out


GROUPS = dict(fwd_row=R.fwd_row_cases, fwd_g16=R.fwd_g16_cases, bwd=R.bwd_cases, part=R.part_cases,
              modes=R.mode_cases, cap=lambda: list(R.CAP))
_measured = {}


@pytest.mark.parametrize("group", list(GROUPS))
def test_f32_evaluation_meets_every_bound(group):
    """Every input set of the GPU tests: the f32 evaluation is inside every bound (so the inputs
    are benign), s does not depend on fma contraction, and the calibration is recorded."""
    worst, meas = {}, dict(s=0.0, y=0.0, ds=0.0, dres=0.0)
    for M, N, mode in GROUPS[group]():
        c = R.build(M, N, mode)
        assert c.s_ambiguous == 0, (M, N, mode)
        for acc in (False, True) if group == "part" else (False,):
            for k, v in f32_ratios(c, acc).items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= 1.0, (M, N, mode, k, v)
        for k, v in R.calibrate(c).items():
            meas[k] = max(meas[k], v)
    _measured[group] = meas
    print(group, {k: round(v, 3) for k, v in worst.items()}, "calibration", {k: round(v, 3) for k, v in meas.items()})


def test_calibration_constants():
    """C is 4 times the measured worst case over all input sets (rounded up to the next half)."""
    for group in GROUPS:
        if group not in _measured:
            test_f32_evaluation_meets_every_bound(group)
    for k in R.C:
        m = max(v[k] for v in _measured.values())
        print(f"{k}: measured {m:.3f}, C {R.C[k]}")
        assert 4 * m <= R.C[k] <= 4 * m + 0.5, (k, m, R.C[k])


@pytest.mark.parametrize("M,N", R.colsum_cases())
def test_colsum_f32_meets_bound(M, N):
    x = R.colsum_input(M, N)
    d = R.colsum_dispatch(M, N)
    assert R.ratio(R.colsum(x, F32), R.colsum(x), R.colsum_bound(x, d["depth"])) <= 1.0


# ------------------------------------------------------------ c. exact cases --
@pytest.mark.parametrize("M,N", R.EXACT_ROW + R.EXACT_G16)
def test_exact_cases_are_exact_in_f32(M, N):
    """y rounds to the position-coded bf16 value for rstd off by up to +-4 f32 ulp (twice the +-2
    a 1-ulp sqrtf and a 1-ulp divide can give), in both lane layouts; every chunk of y is unlike
    the same chunk of the other rows of its 16-row group and every other chunk of its row, and no
    two rows are alike."""
    c = R.exact_case(M, N)
    assert bool((c.sig.sum(-1) == 0).all())
    for lanes in (64, 16):
        for k in (-4, -2, -1, 0, 1, 2, 4):
            f = R.forward(c, F32, lanes, rstd_scale=torch.tensor(1.0 + k * 2.0 ** -23, dtype=F32))
            assert torch.equal(f.mean, torch.zeros(M)) and torch.equal(f.var.to(F64), c.rstd ** -2)
            assert torch.equal(R.to_bf16(f.y), c.y), (lanes, k)
    bits = c.y.view(torch.int16).view(M, N // 8, 8)
    for m0 in range(0, M, 16):                                # unlike the same chunk of its 16-row group
        grp = bits[m0:m0 + 16]
        for j in range(N // 8):
            assert len({tuple(v) for v in grp[:, j].tolist()}) == grp.shape[0], (m0, j)
    for m in range(M):                                        # unlike every other chunk of its row
        assert len({tuple(v) for v in bits[m].tolist()}) == N // 8, m
    assert len({tuple(r) for r in c.y.view(torch.int16).tolist()}) == M
    assert bool((c.y.to(F64).abs() > 0).all())


# ---------------------------------------------------------- d. shape tables --
def _loop_trips(R_, groups):
    """The two loops run literally."""
    tails, t4_0 = set(), 0
    for gi in range(groups):
        r, t4, t1 = gi, 0, 0
        while r + 3 * groups < R_:
            r, t4 = r + 4 * groups, t4 + 1
        while r < R_:
            r, t1 = r + groups, t1 + 1
        tails.add(t1)
        t4_0 = t4 if gi == 0 else t4_0
    return t4_0, sorted(tails)


def test_strided_trips_is_the_loop():
    for groups in (64, 16):
        for R_ in list(range(1, 600)) + [1024, 2048]:
            assert R.strided_trips(R_, groups) == _loop_trips(R_, groups), (R_, groups)


def test_forward_shapes_reach_their_branches():
    want = {8: (1, 1), 64: (1, 8), 136: (1, 17), 504: (1, 63), 512: (1, 64), 520: (2, 1), 1024: (2, 64), 1032: (3, 1),
            1536: (3, 64), 1544: (4, 1), 2040: (4, 63), 2048: (4, 64)}
    assert set(want) == set(R.ROW_N)
    for N, (inst, last) in want.items():
        d = R.fwd_dispatch(5, N, rows1=1)
        assert (d["kernel"], d["inst"], d["last_chunk_lanes"]) == ("row", inst, last), N
        if N not in R.G16_N:
            assert R.fwd_dispatch(5, N, rows1=0) == d, N      # ln_rows1 changes nothing there
    assert {m: (R.fwd_dispatch(m, 8)["blocks"], R.fwd_dispatch(m, 8)["idle_rows"]) for m in R.ROW_M} == \
        {1: (1, 3), 3: (1, 1), 4: (1, 0), 5: (2, 3)}
    for i, N in enumerate(R.G16_N):
        d = R.fwd_dispatch(17, N)
        assert (d["kernel"], d["inst"], d["lanes"]) == ("g16", i + 1, 16)
    assert {m: (R.fwd_dispatch(m, 256)["blocks"], R.fwd_dispatch(m, 256)["idle_rows"]) for m in R.G16_M} == \
        {1: (1, 15), 15: (1, 1), 16: (1, 0), 17: (2, 15), 33: (3, 15)}
    for M, N in R.EXACT_ROW:
        assert R.fwd_dispatch(M, N)["kernel"] == "row" and R.fwd_dispatch(M, N)["blocks"] == 2
    assert [R.fwd_dispatch(M, N)["inst"] for M, N in R.EXACT_ROW] == [1, 2, 3, 4, 4]
    assert [R.fwd_dispatch(M, N)["inst"] for M, N in R.EXACT_G16] == [1, 2, 3, 4]
    assert all(R.fwd_dispatch(M, N)["blocks"] == 2 for M, N in R.EXACT_G16)
    modes = {mode for _, _, mode in R.fwd_row_cases()} & {mode for _, _, mode in R.fwd_g16_cases()}
    assert modes == set(R.MODE_NAMES)


def test_backward_shapes_reach_their_branches():
    got = {m: R.bwd_dispatch(m, 8) for m in R.BWD_M}
    # (blocks, rows per wave, waves with no row, waves with a short range)
    assert {m: (d["nblk"], d["rpw"], d["empty_waves"], d["short_waves"]) for m, d in got.items()} == \
        {1: (1, 1, 3, 0), 31: (1, 8, 0, 1), 32: (1, 8, 0, 0), 33: (2, 5, 1, 1), 45: (2, 6, 0, 1), 257: (9, 8, 3, 1)}
    for N in R.ROW_N:
        d0, d1 = R.bwd_dispatch(45, N, 0), R.bwd_dispatch(45, N, 1)
        assert d1["kernel"] == "plain" and d0["kernel"] == ("pf" if N > 512 else "plain")
        assert d0["inst"] == R.fwd_dispatch(45, N, 1)["inst"]
    assert R.bwd_dispatch(1, 2048)["lds_bytes"] == 65536
    for M, N, _ in R.CAP:
        d = R.bwd_dispatch(M, N)
        assert (d["nblk"], d["rpw"], d["empty_waves"], d["short_waves"]) == (2048, 9, 906, 1) and N <= 136
    # ln_part_sum_kernel: (trips of the unrolled loop, tail trips over the 64 groups) at R blocks
    want = {1: (0, [0, 1]), 63: (0, [0, 1]), 64: (0, [1]), 65: (0, [1, 2]), 192: (0, [3]), 193: (1, [0, 3]),
            256: (1, [0]), 257: (1, [0, 1]), 449: (2, [0, 3]), 2048: (8, [0])}
    assert set(want) == set(R.PART_R)
    for M, N, _ in R.part_cases():
        d = R.bwd_dispatch(M, N)
        assert d["nblk"] == M // 32 and d["rpw"] == 8 and (d["sum_t4"], d["sum_tails"]) == want[M // 32], M
    assert {mode for _, _, mode in R.bwd_cases()} == set(R.MODE_NAMES)


def test_colsum_shapes_reach_their_branches():
    # (chunks, row lanes, idle threads)
    want = {8: (1, 256, 0), 24: (3, 85, 1), 384: (48, 5, 16), 520: (65, 3, 61), 1032: (129, 1, 127), 2048: (256, 1, 0)}
    for N, (nc, per, idle) in want.items():
        d = R.colsum_dispatch(257, N)
        assert (N // 8, d["per"], d["idle_threads"]) == (nc, per, idle)
        assert (d["nblk"], d["rpb"], d["last_block_rows"]) == (2, 129, 128)
        assert d["per"] * N * 4 <= 65536
    assert R.colsum_dispatch(0, 24)["kernel"] == "memset"
    assert [R.colsum_dispatch(m, 24)["nblk"] for m in (1, 255, 256)] == [1, 1, 1]
    want = {15: (0, [0, 1]), 16: (0, [1]), 17: (0, [1, 2]), 48: (0, [3]), 49: (1, [0, 3]), 64: (1, [0]),
            65: (1, [0, 1]), 1024: (16, [0])}
    assert set(want) == set(R.COLSUM_R)
    for r, w in want.items():
        d = R.colsum_dispatch(256 * r, 8)
        assert d["nblk"] == r and d["rpb"] == 256 and (d["sum_t4"], d["sum_tails"]) == w, r
    d = R.colsum_dispatch(R.COLSUM_BIG_M, 8)
    assert (d["nblk"], d["rpb"], d["rows_per_lane"]) == (1024, 257, 2)


# ------------------------------------------------------------------ e. teeth --
def test_a_chunk_from_the_neighbouring_row_fails_y():
    c = R.build(5, 1032, "plain")
    f64, y = R.forward(c, F64), R.to_bf16(R.forward(c, F32).y)
    by, _, _, _ = R.forward_bounds(c, f64, 64, 3)
    assert R.ratio(y, f64.y, by) <= 1.0
    y[2, 520:528] = y[3, 520:528]
    assert R.ratio(y, f64.y, by) > 1.0


def test_a_dropped_dg_row_fails_dg():
    for M, N, mode in [(257, 136, "res"), R.CAP[1]]:
        c = R.build(M, N, mode)
        b64, b32 = R.backward(c, F64), R.backward(c, F32)
        _, _, _, _, bdg, bdb = R.backward_bounds(c, b64, R.bwd_dispatch(M, N)["depth"])
        assert R.ratio(b32.dg, b64.dg, bdg) <= 1.0 and R.ratio(b32.db, b64.db, bdb) <= 1.0
        m = M - 1
        dg = b32.dg - (b32.dyk[m] * b32.xh[m])
        assert R.ratio(dg, b64.dg, bdg) > 1.0
        # one lane's partial (8 columns of one row) is enough
        dg = b32.dg.clone()
        dg[8:16] -= (b32.dyk[m] * b32.xh[m])[8:16]
        assert R.ratio(dg, b64.dg, bdg) > 1.0
        assert R.ratio(b32.db - b32.dyk[m], b64.db, bdb) > 1.0


def test_a_mask_shifted_by_one_pair_fails():
    c = copy.copy(R.build(33, 384, "both"))
    f64, b64 = R.forward(c, F64), R.backward(c, F64)
    by, _, _, _ = R.forward_bounds(c, f64, 16, 3)
    bds, _, bdr, _, _, _ = R.backward_bounds(c, b64, R.bwd_dispatch(33, 384)["depth"])
    ko, kr = c.keep_o, c.keep_r
    c.keep_o, c.keep_r = ko.clone(), kr.clone()
    c.keep_o[:, 128:136] = ko[:, 130:138]                 # one chunk, one column pair along
    c.keep_r[:, 128:136] = kr[:, 130:138]
    y = R.to_bf16(R.forward(c, F32, 16).y)
    b32 = R.backward(c, F32)
    assert R.ratio(y, f64.y, by) > 1.0
    assert not torch.equal(y == 0, ~ko)
    assert R.ratio(R.to_bf16(b32.ds), b64.ds, bds) > 1.0      # dy masked at the wrong columns
    assert R.ratio(R.to_bf16(b32.dres), b64.dres, bdr) > 1.0


@pytest.mark.parametrize("mode", ["slope_x", "slope_r"])
def test_a_flipped_derivative_at_zero_fails(mode):
    c = R.build(5, 136, mode)
    b64, b32 = R.backward(c, F64), R.backward(c, F32)
    bds, _, bdr, _, _, _ = R.backward_bounds(c, b64, R.bwd_dispatch(5, 136)["depth"])
    pre, slope = (c.s, c.slope_x) if mode == "slope_x" else (c.r, c.slope_r)
    zero = pre.to(F32) == 0
    assert bool(zero.any()) and bool((b64.o[zero] != 0).all())
    got = b32.ds if mode == "slope_x" else b32.dres
    ref, bound = (b64.ds, bds) if mode == "slope_x" else (b64.dres, bdr)
    assert R.ratio(R.to_bf16(got), ref, bound) <= 1.0
    flipped = torch.where(zero, got / slope, got)             # v >= 0 ? 1 : slope
    assert R.ratio(R.to_bf16(flipped), ref, bound) > 1.0
