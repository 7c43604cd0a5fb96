"""fp64 restatement of the weight-gradient kernel (csrc/dw.hip: dw_dma_kernel<DET>, dw_reduce_kernel;
snvrag_linear_dw, snvrag_linear_dw_parts and their *_det forms) for the kernel-level tests, with
derived per-element bounds, a restatement of the host's chunking and of the workgroup remap, and the
shape table the tests sweep (tests/test_dw_refs_cpu.py proves them, tests/test_gpu_linear_dw.py runs
them).  ratio, F64, U and the accumulation constant are those of tests/sgemm_refs.py, not restated.

What the kernels compute, in their order
  chunk  the M rows are cut into S chunks of `chunk` rows (chunks()); a workgroup owns one 128 x 128
         tile of one chunk and walks the chunk's rows in 32-row stages through a 4-slot LDS ring:
         acc[n][k] = sum_m dy[m, n] x[m, k] in f32 32x32x16 bf16 MFMA accumulators, stage after stage.
         The k0 == 0 tiles also sum dy[m, n] over m in f32: a lane adds its 8 values of each 16-row
         half serially, one shuffle folds lanes 32 .. 63 into lanes 0 .. 31.
  atomic every chunk's tile (and bias sums) is added into the output with one f32 atomic per element:
         out = ((prior + p_a) + p_b) + ..., the chunks in any order.
  det    every chunk's tile is stored to ws[zc][n][k] (bias: ws + S N K, [zc][n]); dw_reduce_kernel
         forms ((p_0 + p_1) + ... + p_(S-1)) and adds the prior value last.
  parts  row n of dW / entry n of db lives in part n / seg of separately allocated buffers.

Bounds, per element, u = U = 2^-24
  A product of two bf16 numbers is exact in f32, so a chunk's partial p_c carries one f32 rounding per
  accumulated non-zero product (adding an exact zero is exact) - the accumulation model of
  sgemm_refs.pre / dense_refs.linear for the same 32x32x16 bf16 MFMA chain, with its constant:
      |p_c - exact_c| <= (Kn_c + S.C["acc"]) u A_c,
  A_c = sum over the chunk's rows of |dy||x|, Kn_c the number of its non-zero products.  The bias sum
  of a lane is a serial f32 sum of at most Kn_c non-zero values plus the shuffle's add: the same
  expression with A_c = sum |dy| and Kn_c the non-zero dy of the column.
  Joining the partials takes S f32 adds whether atomic or in the reduce kernel (the first may be exact)
  and the prior one more; every intermediate sum is at most A + |prior| in magnitude (to first order:
  the spare unit of C["acc"] is what second-order terms live in), so
      bound = sum_c (Kn_c + C["acc"]) u A_c + (S + 1) u (A + |prior|),   A = sum_c A_c.
  Exact inputs: where dy, x and the prior hold integers and A + |prior| < 2^24, every partial sum in any
  order is an integer below 2^24 and so exact in f32: the bound is 0, and atomic, deterministic and
  fp64 results agree bit for bit.
The bounds are never measured against a kernel.

Inputs.  Random: randn dy and x rounded to bf16 (no subnormals), amplitude 1, or with dy's rows scaled by
2^e, e spread over -12 .. 12, and x's columns by 2^(3 k % 13 - 6), so the bound differs from element to
element by three orders of magnitude.  Exact: integers in [-4, 4] from a fixed hash of (m, n) / (m, k), integer
priors in [-8, 8]: |sum| <= 16 M + 8 < 2^24."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

import sgemm_refs as S
from sgemm_refs import BF16, F32, F64, U, ratio  # noqa: F401

DW_T = 128          # output tile (n and k)
DW_R = 32           # rows per stage
RING_SLOTS = 4      # ring slots

Ref = namedtuple("Ref", "w b A_w A_b")


def cdiv(a, b):
    return -(-a // b)


def _d(t):
    return t.detach().to(F64)


# --------------------------------------------------------------- the reference --
def ref(dy, x, prior_w=None, prior_b=None):
    """fp64 (dW [N, K], db [N], A_w = |dy|^T |x|, A_b = sum |dy|) of dy [M, N], x [M, K], on the device of
    dy; the priors are added to dW / db (not to the absolute sums)."""
    d, xx = _d(dy), _d(x)
    w, b = d.T @ xx, d.sum(0)
    if prior_w is not None:
        w = w + _d(prior_w).to(w.device)
    if prior_b is not None:
        b = b + _d(prior_b).to(b.device)
    return Ref(w, b, d.abs().T @ xx.abs(), d.abs().sum(0))


# ------------------------------------------------------------------- dispatch --
def dw_splits(M, N, K):
    """snvrag_dw_splits."""
    tiles = (N // DW_T) * (K // DW_T)
    target = 512 if tiles >= 16 else 256
    s = target // max(tiles, 1)
    max_s = (M + 8 * DW_R - 1) // (8 * DW_R)
    return min(max(s, 1), max(max_s, 1))


def chunks(M, N, K, splits):
    """dw_chunks: splits (as used), chunk (rows per chunk), S (non-empty chunks), rows [S], stages [S],
    grid (workgroups) and ws_bytes of the deterministic pair."""
    if splits <= 0:
        splits = dw_splits(M, N, K)
    chunk = cdiv(cdiv(M, splits), DW_R) * DW_R
    Sn = cdiv(M, chunk) if M > 0 else 0
    rows = [min(M, (c + 1) * chunk) - c * chunk for c in range(Sn)]
    return SimpleNamespace(splits=splits, chunk=chunk, S=Sn, rows=rows, stages=[cdiv(r, DW_R) for r in rows],
                           grid=(N // DW_T) * (K // DW_T) * Sn, ws_bytes=Sn * (N * K + N) * 4 if M > 0 else 0)


def work_item(b, grid, xcd_map):
    """The work item (chunk-major, tiles inner) that workgroup b of `grid` takes."""
    if not xcd_map:
        return b
    xcd, per, rem = b & 7, grid >> 3, grid & 7
    return xcd * per + min(xcd, rem) + (b >> 3)


def decode(w, N, K):
    """(chunk index, n0, k0) of work item w."""
    nx = N // DW_T
    ntile = nx * (K // DW_T)
    tile = w % ntile
    return w // ntile, (tile % nx) * DW_T, (tile // nx) * DW_T


# --------------------------------------------------------------------- bounds --
def is_exact(dy, x, prior=None, A=None):
    """Integer operands whose absolute sums stay below 2^24 (module docstring)."""
    ts = [dy, x] + ([] if prior is None else [prior])
    if not all(bool((_d(t) == _d(t).round()).all()) for t in ts):
        return False
    top = float(A.max()) + (float(_d(prior).abs().max()) if prior is not None else 0.0)
    return top < 2.0 ** 24


def _bound(parts, ch, prior, exact):
    """parts: per chunk (A_c, Kn_c)."""
    A = sum(a for a, _ in parts)
    if exact:
        return torch.zeros_like(A)
    p = torch.zeros_like(A) if prior is None else _d(prior).to(A.device).abs()
    return sum((kn + S.C["acc"]) * U * a for a, kn in parts) + (ch.S + 1) * U * (A + p)


def _chunk_rows(ch):
    return [(c * ch.chunk, c * ch.chunk + r) for c, r in enumerate(ch.rows)]


def bound_w(dy, x, ch, prior_w=None):
    """[N, K] bound of dW for the chunking ch (module docstring)."""
    d, xx = _d(dy), _d(x)
    parts = [(d[a:b].abs().T @ xx[a:b].abs(), (d[a:b] != 0).to(F64).T @ (xx[a:b] != 0).to(F64)) for a, b in _chunk_rows(ch)]
    return _bound(parts, ch, prior_w, is_exact(dy, x, prior_w, sum(a for a, _ in parts)))


def bound_b(dy, ch, prior_b=None):
    """[N] bound of db."""
    d = _d(dy)
    parts = [(d[a:b].abs().sum(0), (d[a:b] != 0).to(F64).sum(0)) for a, b in _chunk_rows(ch)]
    return _bound(parts, ch, prior_b, is_exact(dy, dy, prior_b, sum(a for a, _ in parts)))


# -------------------------------------------------------------------- shapes --
# Every case: fam, M, N, K, splits, parts (output buffers), db, ld (leading-dimension kind) and `want`,
# what the (M, splits) is listed for: chunk, S, last (rows of the last chunk), nst (stages of chunk 0),
# grid.  test_dw_refs_cpu.py checks every `want` against chunks().
LD_KINDS = ("pad", "dy@128", "dy@N", "x@128", "x@K")

# N = K = 128, splits = 1: one chunk of nst stages.  The prologue issues min(3, nst) stages, the
# unrolled loop runs while st + 4 <= nst, the tail loop takes the rest: nst 1 .. 10, 12, 13.
RING = {1: 1, 32: 1, 33: 2, 64: 2, 96: 3, 97: 4, 128: 4, 129: 5, 160: 5, 161: 6, 192: 6, 224: 7, 256: 8, 257: 9,
        289: 10, 384: 12, 416: 13}
RING_NST = set(range(1, 11)) | {12, 13}
TAIL_R = (1, 3, 4, 5, 15, 16, 17, 31)
# (M, splits, chunk, S, rows of the last chunk).  290 / 9 rounds up to 64-row chunks, so it has 5
# chunks, not 9: 270 / 9 is the case with nine (the reduce loop's unroll by 4 leaves S % 4 = 1).
CHUNKING = ((200, 3, 96, 3, 8), (100, 50, 32, 4, 4), (33, 64, 32, 2, 1), (290, 2, 160, 2, 130), (290, 5, 64, 5, 34),
            (290, 9, 64, 5, 34), (270, 9, 32, 9, 14), (700, 0, 256, 3, 188))
CHUNK_S = {2, 3, 4, 5, 9}
# (N, K, M, splits, grid): both sides of 8 workgroups, non-multiples of 8, exactly 8, 9 and 17
TILES = ((256, 128, 97, 1, 2), (256, 128, 97, 2, 4), (128, 256, 97, 1, 2), (128, 256, 97, 2, 4), (384, 256, 97, 1, 6),
         (384, 256, 97, 2, 12), (512, 384, 97, 1, 12), (512, 384, 97, 2, 24), (384, 128, 97, 1, 3), (256, 128, 97, 4, 8),
         (384, 128, 70, 3, 9), (128, 128, 539, 17, 17))
TILE_GRIDS = {2, 3, 4, 6, 8, 9, 12, 17, 24}
PARTS = ((384, 3), (512, 2), (512, 4), (256, 2))
# (M, N, K, splits, parts, scaled)
RANDOM = ((97, 256, 128, 2, 1, False), (290, 384, 256, 5, 3, False), (416, 128, 256, 1, 1, False),
          (290, 384, 256, 5, 3, True))
MMAX = 700


def _case(fam, M, N, K, splits, parts=1, db=True, ld=None, **want):
    c = SimpleNamespace(fam=fam, M=M, N=N, K=K, splits=splits, parts=parts, db=db, ld=ld, want=want)
    c.id = f"{fam}-M{M}-N{N}-K{K}-s{splits}-p{parts}{'' if db else '-nodb'}{'-' + ld if ld else ''}"
    return c


def cases(fam=None):
    """The exact-input shape table, or one family of it."""
    out = [_case("ring", M, 128, 128, 1, nst=nst, S=1) for M, nst in RING.items()]
    out += [_case("tail", 128 + r, 128, 128, 1, nst=5, S=1, last=128 + r) for r in TAIL_R]
    out += [_case("chunk", M, 128, 128, s, chunk=ck, S=Sn, last=last) for M, s, ck, Sn, last in CHUNKING]
    out += [_case("tile", M, N, K, s, grid=g) for N, K, M, s, g in TILES]
    out += [_case("parts", 97, N, 256, 2, parts=p, db=db, S=2) for N, p in PARTS for db in (True, False)]
    out += [_case("ld", 97, 256, 128, 2, ld=kind, S=2) for kind in LD_KINDS]
    return [c for c in out if fam is None or c.fam == fam]


def random_cases():
    return [_case("scaled" if sc else "random", M, N, K, s, parts=p) for M, N, K, s, p, sc in RANDOM]


# (M, N, K, splits) of the host restatement: the table's own, the bench's 2 B L = 49 440 rows with the
# model's four layer shapes, sizes around the thresholds of snvrag_dw_splits (16 tiles, 256-row stages)
HOST_TABLE = ([(c.M, c.N, c.K, c.splits) for c in cases()]
              + [(49440, N, K, s) for N, K in ((1152, 384), (384, 384), (1536, 384), (384, 1536)) for s in (0, 1, 14, 29)]
              + [(M, N, K, 0) for M in (1, 255, 256, 257, 4097, 65536) for N, K in ((128, 128), (512, 384), (512, 512), (1536, 1536))])


def lds(c):
    """(ldy, dy column offset, dy storage width, ldx, x offset, x width) of a case."""
    ldy, oy, wy, ldx, ox, wx = c.N, 0, c.N, c.K, 0, c.K
    if c.ld == "pad":
        ldy, ldx, wy, wx = c.N + 8, c.K + 8, c.N + 8, c.K + 8
    elif c.ld in ("dy@128", "dy@N"):
        ldy = wy = 3 * c.N
        oy = 128 if c.ld == "dy@128" else c.N
    elif c.ld in ("x@128", "x@K"):
        ldx = wx = 3 * c.K
        ox = 128 if c.ld == "x@128" else c.K
    return ldy, oy, wy, ldx, ox, wx


# -------------------------------------------------------------------- inputs --
def _hash(m, j, salt):
    """Integers in [-4, 4] from a fixed multiplicative hash of (m, j)."""
    h = (m * 7919 + j * 104729 + (m * j) % 1013 + salt) * 2654435761
    return ((h >> 13) % 9 - 4).to(F64)


@functools.lru_cache(maxsize=None)
def exact_inputs(N, K):
    """dy [MMAX, N], x [MMAX, K] in bf16, prior_w [N, K], prior_b [N] in f32: every M of the table is a
    row prefix.  Do not modify."""
    m = torch.arange(MMAX, dtype=torch.int64)[:, None]
    dy, x = _hash(m, torch.arange(N)[None, :], 1), _hash(m, torch.arange(K)[None, :], 2)
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    pw = ((3 * n + 5 * k) % 17 - 8).to(F64)
    pb = ((7 * n[:, 0]) % 17 - 8).to(F64)
    assert 16 * MMAX + 8 < 2 ** 24
    return SimpleNamespace(dy=dy.to(BF16), x=x.to(BF16), pw=pw.to(F32), pb=pb.to(F32))


@functools.lru_cache(maxsize=None)
def random_inputs(N, K, scaled=False):
    """randn dy [MMAX, N], x [MMAX, K] rounded to bf16, f32 priors; scaled: module docstring.  Do not modify."""
    g = S._gen(N, K, 51)
    dy, x = torch.randn(MMAX, N, generator=g), torch.randn(MMAX, K, generator=g)
    if scaled:
        m = torch.arange(MMAX)
        dy = dy * (2.0 ** ((m * 7) % 25 - 12).float())[:, None]
        x = x * (2.0 ** ((3 * torch.arange(K)) % 13 - 6).float())[None, :]
    return SimpleNamespace(dy=S._bf(dy), x=S._bf(x), pw=torch.randn(N, K, generator=g), pb=torch.randn(N, generator=g))


def inputs(c):
    """(dy [M, N], x [M, K], prior_w, prior_b) of a case."""
    src = exact_inputs(c.N, c.K) if c.fam not in ("random", "scaled") else random_inputs(c.N, c.K, c.fam == "scaled")
    return src.dy[:c.M], src.x[:c.M], src.pw, src.pb


# ------------------------------------------------------------------- mutants --
MUTANTS = ("last_row_dropped", "chunk_first_row_twice", "stale_ring_stage", "tile_transposed", "wk_halves_swapped",
           "db_from_k128_tile", "db_upper_lanes_lost", "parts_exchanged", "prior_twice", "prior_missing")


def applicable(name, c, ch):
    """Whether the fault `name` can exist at case c (a fault changes nothing where its branch is not taken)."""
    if name == "chunk_first_row_twice":
        return ch.S >= 2
    if name == "stale_ring_stage":
        return max(ch.stages) > RING_SLOTS
    if name == "db_from_k128_tile":
        return c.db
    if name == "db_upper_lanes_lost":                       # rows 8 .. 15 of a 16-row half: a chunk of 9 rows has one
        return c.db and max(ch.rows) > 8
    if name == "parts_exchanged":
        return c.parts >= 2
    return True


def mutate(name, c, ch, r, dy, x, pw, pb):
    """The fp64 result r = ref(dy, x, pw, pb) with the fault `name` planted: (dW, db)."""
    d, xx = _d(dy), _d(x)
    w, b = r.w.clone(), r.b.clone()
    if name == "last_row_dropped":
        w -= torch.outer(d[-1], xx[-1])
        b -= d[-1]
    elif name == "chunk_first_row_twice":
        m = ch.chunk                                        # first row of chunk 1, also added to chunk 0
        w += torch.outer(d[m], xx[m])
        b += d[m]
    elif name == "stale_ring_stage":                        # the last stage of the longest chunk reads its slot's
        ci = max(range(ch.S), key=lambda i: ch.stages[i])   # earlier content: the stage 4 back, all 32 rows of it
        st, base = ch.stages[ci] - 1, ci * ch.chunk
        a0, a1 = base + st * DW_R, base + ch.rows[ci]
        o0 = base + (st - RING_SLOTS) * DW_R
        w += d[o0:o0 + DW_R].T @ xx[o0:o0 + DW_R] - d[a0:a1].T @ xx[a0:a1]
        b += d[o0:o0 + DW_R].sum(0) - d[a0:a1].sum(0)
    elif name == "tile_transposed":
        w[:DW_T, :DW_T] = w[:DW_T, :DW_T].T.clone()
    elif name == "wk_halves_swapped":
        w[:DW_T, :DW_T] = torch.cat([w[:DW_T, 64:DW_T], w[:DW_T, :64]], 1)
    elif name == "db_from_k128_tile":                       # taken from the k0 = 128 tiles too: doubled; only
        b = 2 * b - _d(pb) if c.K >= 2 * DW_T else _d(pb).clone()    # from them where there is none: zero
    elif name == "db_upper_lanes_lost":                     # lanes 32 .. 63 hold rows 8 .. 15 of every 16
        for a0, a1 in _chunk_rows(ch):
            m = torch.arange(a1 - a0)
            b -= d[a0:a1][(m % 16) >= 8].sum(0)
    elif name == "parts_exchanged":
        seg = c.N // c.parts
        w[:2 * seg] = torch.cat([w[seg:2 * seg], w[:seg]])
        b[:2 * seg] = torch.cat([b[seg:2 * seg], b[:seg]])
    elif name == "prior_twice":
        w += _d(pw)
        b += _d(pb)
    elif name == "prior_missing":
        w -= _d(pw)
        b -= _d(pb)
    else:
        raise KeyError(name)
    return w, b


def emulate_f32(dy, x, ch, pw=None, pb=None):
    """The chunked sum in f32: torch.float32 matmul per chunk, then sequential adds, the prior last."""
    d, xx = dy.to(F32), x.to(F32)
    w = b = None
    for a0, a1 in _chunk_rows(ch):
        pwc, pbc = d[a0:a1].T @ xx[a0:a1], d[a0:a1].sum(0)
        w, b = (pwc, pbc) if w is None else (w + pwc, b + pbc)
    if pw is not None:
        w = w + pw
    if pb is not None:
        b = b + pb
    return w, b
