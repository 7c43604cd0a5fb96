"""CPU proof of tests/dw_refs.py, which test_gpu_linear_dw.py holds csrc/dw.hip to:

  * ref equals a plain triple loop;
  * chunks partitions [0, M) for M = 1 .. 600 against every kind of split count, and every entry of
    the shape table produces the stage count, chunk size, chunk count, last chunk and grid it is
    listed for (the table checks itself: a row that does not reach its edge fails here);
  * work_item is a permutation of range(grid) for every grid from 1 to 200, remapped or not;
  * teeth: every planted fault exceeds the bound on random inputs, and differs on the exact inputs,
    at every shape of the table where the fault can exist; where it cannot, the (fault, shape) pair is
    listed by `applicable`, printed, and checked to be listed for exactly the stated reason;
  * the bound is not below what f32 arithmetic does: an f32 emulation of the chunked sum (float32
    matmul per chunk, sequential adds, prior last) stays inside it on the random inputs and equals
    the fp64 result bit for bit on the exact ones."""
import pytest
import torch

import dw_refs as R

F64, F32 = R.F64, R.F32
ALL = R.cases() + R.random_cases()


# ------------------------------------------------------------ the reference --
def test_ref_is_the_triple_loop():
    g = torch.Generator().manual_seed(3)
    M, N, K = 5, 4, 3
    dy, x = torch.randn(M, N, generator=g).to(R.BF16), torch.randn(M, K, generator=g).to(R.BF16)
    pw, pb = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    w = [[float(pw[n, k]) for k in range(K)] for n in range(N)]
    aw = [[0.0] * K for _ in range(N)]
    b, ab = [float(pb[n]) for n in range(N)], [0.0] * N
    for m in range(M):
        for n in range(N):
            b[n] += float(dy[m, n])
            ab[n] += abs(float(dy[m, n]))
            for k in range(K):
                w[n][k] += float(dy[m, n]) * float(x[m, k])
                aw[n][k] += abs(float(dy[m, n]) * float(x[m, k]))
    r = R.ref(dy, x, pw, pb)
    for got, want in ((r.w, w), (r.b, b), (r.A_w, aw), (r.A_b, ab)):
        assert got.dtype == F64
        torch.testing.assert_close(got, torch.tensor(want, dtype=F64), rtol=0, atol=1e-14)
    r0 = R.ref(dy, x)
    torch.testing.assert_close(r0.w + pw.double(), r.w, rtol=0, atol=1e-14)
    assert torch.equal(r0.A_w, r.A_w) and torch.equal(r0.A_b, r.A_b)


# ---------------------------------------------------------------- dispatch --
def test_chunks_partition_the_rows():
    for M in range(1, 601):
        for splits in (0, 1, 2, 3, 7, 50, 64):
            ch = R.chunks(M, 128, 128, splits)
            used = splits if splits > 0 else R.dw_splits(M, 128, 128)
            assert ch.splits == used and ch.chunk % R.DW_R == 0 and ch.chunk >= R.cdiv(M, used)
            assert 1 <= ch.S <= used and len(ch.rows) == ch.S == len(ch.stages)
            assert sum(ch.rows) == M and all(r == ch.chunk for r in ch.rows[:-1]) and 1 <= ch.rows[-1] <= ch.chunk
            assert all(st == R.cdiv(r, R.DW_R) and st >= 1 for st, r in zip(ch.stages, ch.rows))
            assert ch.grid == ch.S and ch.ws_bytes == ch.S * (128 * 128 + 128) * 4
    assert R.chunks(0, 128, 128, 0).S == 0 and R.chunks(0, 128, 128, 0).ws_bytes == 0


def test_dw_splits_restated():
    # tiles >= 16 take the 512-workgroup target; max_s (eight stages per chunk) binds at small M
    assert R.dw_splits(49440, 1152, 384) == 18 and R.dw_splits(49440, 384, 384) == 28
    assert R.dw_splits(49440, 1536, 384) == 14 and R.dw_splits(49440, 384, 1536) == 14
    assert R.dw_splits(700, 128, 128) == 3 and R.dw_splits(1, 128, 128) == 1
    assert R.dw_splits(49440, 512, 512) == 32 and R.dw_splits(49440, 512, 384) == 21


def test_shape_table_reaches_what_it_lists():
    seen = {"nst": set(), "S": set(), "grid": set(), "tail": set()}
    for c in ALL:
        ch = R.chunks(c.M, c.N, c.K, c.splits)
        got = dict(chunk=ch.chunk, S=ch.S, last=ch.rows[-1], nst=ch.stages[0], grid=ch.grid)
        for key, val in c.want.items():
            assert got[key] == val, (c.id, key, got[key], val)
        assert c.M <= R.MMAX and c.N % 128 == 0 and c.K % 128 == 0 and c.N % c.parts == 0 and (c.N // c.parts) % 128 == 0
        if c.fam == "ring":
            seen["nst"].add(ch.stages[0])
        if c.fam == "tail":
            seen["tail"].add(c.M % 32)
        if c.fam == "chunk":
            seen["S"].add(ch.S)
        if c.fam == "tile":
            seen["grid"].add(ch.grid)
    assert seen["nst"] == R.RING_NST and set(R.TAIL_R) == seen["tail"]
    assert seen["S"] == R.CHUNK_S and seen["grid"] == R.TILE_GRIDS
    assert len({c.id for c in ALL}) == len(ALL)
    # the issue's own lists are all here (additions are allowed, omissions not)
    assert {1, 32, 33, 64, 96, 97, 128, 129, 160, 224, 256, 257, 289, 384, 416} <= set(R.RING)
    assert {(200, 3), (100, 50), (33, 64), (290, 2), (290, 5), (290, 9), (700, 0)} <= {(r[0], r[1]) for r in R.CHUNKING}
    assert {(N, K, s) for N, K in ((256, 128), (128, 256), (384, 256), (512, 384)) for s in (1, 2)} <= \
        {(N, K, s) for N, K, M, s, _ in R.TILES if M == 97}
    # one-stage chunks, a chunk count below the split count, the auto-split path with max_s binding
    assert R.chunks(100, 128, 128, 50).stages == [1, 1, 1, 1] and R.chunks(33, 128, 128, 64).S == 2 < 64
    assert R.dw_splits(700, 128, 128) == R.cdiv(700, 256) < 256
    # grids on both sides of 8 and non-multiples of 8; ring tails that leave the unrolled loop at every slot
    assert any(g < 8 for g in seen["grid"]) and any(g > 8 and g % 8 for g in seen["grid"]) and 8 in seen["grid"]
    assert {n % 4 for n in seen["nst"] if n >= 4} == {0, 1, 2, 3}
    kinds = {c.ld for c in R.cases("ld")}
    assert kinds == set(R.LD_KINDS)
    for c in R.cases("ld"):
        ldy, oy, wy, ldx, ox, wx = R.lds(c)
        assert ldy >= c.N and ldx >= c.K and ldy % 8 == 0 and ldx % 8 == 0 and oy % 8 == 0 and ox % 8 == 0
        assert oy + c.N <= wy == ldy and ox + c.K <= wx == ldx and (ldy > c.N or ldx > c.K)


def test_work_item_is_a_permutation():
    for grid in range(1, 201):
        for xcd_map in (0, 1):
            assert sorted(R.work_item(b, grid, xcd_map) for b in range(grid)) == list(range(grid)), (grid, xcd_map)
    # the blocks of one XCD (b % 8 equal) take consecutive work items
    for grid in (7, 8, 9, 17, 24, 199):
        for xcd in range(min(grid, 8)):
            w = [R.work_item(b, grid, 1) for b in range(xcd, grid, 8)]
            assert w == list(range(w[0], w[0] + len(w)))
    assert R.decode(5, 384, 256) == (0, 256, 128) and R.decode(6, 384, 256) == (1, 0, 0)


# ------------------------------------------------------------------- teeth --
def _planted(c, exact):
    """{fault: max err / bound (random inputs) or differs (exact inputs)} and the faults listed as not
    applicable at the case."""
    if exact:
        src = R.exact_inputs(c.N, c.K)
    else:
        src = R.random_inputs(c.N, c.K, c.fam == "scaled")
    dy, x, pw, pb = src.dy[:c.M], src.x[:c.M], src.pw, src.pb
    ch = R.chunks(c.M, c.N, c.K, c.splits)
    r = R.ref(dy, x, pw, pb)
    bw, bb = R.bound_w(dy, x, ch, pw), R.bound_b(dy, ch, pb)
    assert bw.shape == (c.N, c.K) and bb.shape == (c.N,) and bool(torch.isfinite(bw).all() and torch.isfinite(bb).all())
    if exact:
        assert not bw.any() and not bb.any(), "exact inputs: the bound is 0"
    else:
        assert bool((bw > 0).all() and (bb > 0).all())
    caught, na = {}, []
    for name in R.MUTANTS:
        if not R.applicable(name, c, ch):
            na.append(name)
            continue
        w, b = R.mutate(name, c, ch, r, dy, x, pw, pb)
        rw = R.ratio(w, r.w, bw)
        rb = R.ratio(b, r.b, bb) if c.db else 0.0
        caught[name] = max(rw, rb)
    return caught, na


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_every_fault_is_caught_where_it_applies(exact):
    listed = {}
    for c in ALL:
        caught, na = _planted(c, exact)
        for name, r in caught.items():
            assert r > 1.0, f"{c.id}: fault {name} stays inside the bound (max err / bound {r:.3g})"
        for name in na:
            listed.setdefault(name, []).append(c.id)
        assert set(caught) | set(na) == set(R.MUTANTS)
    for name, ids in listed.items():
        print(f"{name}: not applicable at {len(ids)} of {len(ALL)} shapes: {' '.join(ids)}")
    # exactly the faults whose branch a shape may lack are ever listed, each for the stated reason
    assert set(listed) <= {"chunk_first_row_twice", "stale_ring_stage", "db_from_k128_tile", "db_upper_lanes_lost", "parts_exchanged"}
    for c in ALL:
        ch = R.chunks(c.M, c.N, c.K, c.splits)
        assert (c.id in listed.get("chunk_first_row_twice", [])) == (ch.S == 1)
        assert (c.id in listed.get("stale_ring_stage", [])) == (max(ch.stages) <= R.RING_SLOTS)
        assert (c.id in listed.get("parts_exchanged", [])) == (c.parts == 1)
        assert (c.id in listed.get("db_from_k128_tile", [])) == (not c.db)
        assert (c.id in listed.get("db_upper_lanes_lost", [])) == (not c.db or max(ch.rows) <= 8)
    for name in R.MUTANTS:
        assert len(listed.get(name, [])) < len(ALL), f"{name} applies nowhere"


def test_db_faults_show_in_db_alone():
    c = next(c for c in R.cases("parts") if c.db and c.N == 384)
    dy, x, pw, pb = R.inputs(c)
    ch = R.chunks(c.M, c.N, c.K, c.splits)
    r = R.ref(dy, x, pw, pb)
    for name in ("db_from_k128_tile", "db_upper_lanes_lost"):
        w, b = R.mutate(name, c, ch, r, dy, x, pw, pb)
        assert torch.equal(w, r.w) and not torch.equal(b, r.b)
    w, b = R.mutate("db_from_k128_tile", c, ch, r, dy, x, pw, pb)
    assert torch.equal(b - pb.double(), 2 * (r.b - pb.double()))
    c1 = R.cases("ring")[5]
    d1, x1, pw1, pb1 = R.inputs(c1)
    _, b = R.mutate("db_from_k128_tile", c1, R.chunks(c1.M, 128, 128, 1), R.ref(d1, x1, pw1, pb1), d1, x1, pw1, pb1)
    assert torch.equal(b, pb1.double())                       # K = 128: no such tile, nothing added


# ------------------------------------------------- the bound against f32 --
def test_f32_emulation_stays_inside_the_bound():
    worst = 0.0
    for c in ALL:
        for fam_exact in (False, True):
            src = R.exact_inputs(c.N, c.K) if fam_exact else R.random_inputs(c.N, c.K, c.fam == "scaled")
            dy, x = src.dy[:c.M], src.x[:c.M]
            ch = R.chunks(c.M, c.N, c.K, c.splits)
            for pw, pb in ((None, None), (src.pw, src.pb)):
                w, b = R.emulate_f32(dy, x, ch, pw, pb)
                r = R.ref(dy, x, pw, pb)
                rw, rb = R.ratio(w, r.w, R.bound_w(dy, x, ch, pw)), R.ratio(b, r.b, R.bound_b(dy, ch, pb))
                if fam_exact:
                    assert rw == 0.0 and rb == 0.0, c.id
                    assert torch.equal(w.double(), r.w) and torch.equal(b.double(), r.b)
                else:
                    assert rw <= 1.0 and rb <= 1.0, (c.id, rw, rb)
                    worst = max(worst, rw, rb)
    print(f"f32 emulation: worst max err / bound {worst:.3f}")
    assert worst > 0.0                                        # and f32 does round here: the bound has work to do


def test_exact_inputs_are_exact_and_use_their_range():
    e = R.exact_inputs(512, 384)
    for t in (e.dy, e.x):
        v = t.double()
        assert torch.equal(v, v.round()) and float(v.min()) == -4 and float(v.max()) == 4
        assert not bool((v == 0).all(1).any()), "a row of zeros would hide its stage"
    assert float(e.pw.abs().max()) == 8 and float(e.pb.abs().max()) == 8
    r = R.ref(e.dy, e.x, e.pw, e.pb)
    assert float(r.A_w.max()) + 8 < 2 ** 24 and R.is_exact(e.dy, e.x, e.pw, r.A_w)
    s = R.random_inputs(384, 256, True)
    assert not R.is_exact(s.dy[:97], s.x[:97], None, R.ref(s.dy[:97], s.x[:97]).A_w)
    # scaled: the per-element bound spans orders of magnitude
    c = R.random_cases()[-1]
    dy, x, pw, pb = R.inputs(c)
    bw = R.bound_w(dy, x, R.chunks(c.M, c.N, c.K, c.splits))
    assert c.fam == "scaled" and float(bw.max() / bw.min()) > 1000.0
    rows = dy.double().abs().max(1).values
    assert float(rows.max() / rows.min()) > 2.0 ** 20
