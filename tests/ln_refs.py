"""Plain torch restatements of the training LayerNorm family and the bf16 column sum
(csrc/train.hip: ln_fwd_train_kernel / ln_fwd_train_g16, ln_bwd_kernel / ln_bwd_pf_kernel,
ln_part_sum_kernel, colsum_part_kernel / colsum_f32_kernel) for the kernel-level tests, with the
shape tables those tests sweep and a restatement of the integer arithmetic of the dispatch.
Everything runs on the CPU; ``dtype=float64`` is the reference, ``float32`` the calibration
evaluation that shows a test's inputs are benign (test_ln_refs_cpu.py).

The operation, with the kernels' own rounding points (lrelu_a(v) = v > 0 ? v : a v, sc = f32(1 /
(1 - p)), keep_* = attn_helpers.ln_keep_mask, stream 0 for the residual and 1 for the output):

  xa = bf16(lrelu_sx(x)),  ra = bf16(lrelu_sr(r))         one f32 multiply, one conversion each
  s  = bf16(xa + ra keep_r sc_r)                          (s = x, the pre-activation, without r)
  (mean, rstd) of the bf16 s (of xa without r), biased variance, eps an f32
  y  = ((s - mean) rstd g + b) keep_o sc_o
  xh = (s - mean) rstd,  gy = dy keep_o sc_o g
  ds = rstd (gy - mean_n(gy) - xh mean_n(gy xh)) lrelu_sx'(x)
  dres = rstd (...) keep_r sc_r lrelu_sr'(r)
  dg = sum_m dy keep_o sc_o xh,  db = sum_m dy keep_o sc_o

xa and ra are single correctly-rounded f32 operations, the same bits on every IEEE machine, so
they are computed in f32 in both evaluations.  s is one bf16 rounding of a two-term sum whose f32
evaluation may or may not be contracted into an fma by the compiler; build() zeroes r at the few
elements where the two roundings differ, so that s is one definite bf16 tensor and the forward
reference normalises exactly what the kernel normalises.  The backward reference is isolated: it
takes s and the f32 stats as given and never recomputes them.

Bounds, per element, u = 2^-24:
  bf16 outputs   |got - ref| <= ulp_bf16(ref) / 2 + c u A, A the sum of the magnitudes of the
                 terms of that element:
                   s     |xa| + |ra| keep_r sc_r
                   y     keep_o sc_o (rstd |g| (|s| + mean_n|s|) + |b|)
                   ds    rstd (|gy| + mean_n|gy| + |xh| mean_n|gy xh|) |lrelu'|
                   dres  the same times keep_r sc_r |lrelu_sr'|
                 A dropped element has ref = 0 and A = 0: it must be exactly 0.
  mean           (d + 1) u mean_n|s|, d = 8 nch + log2(lanes): the serial adds of a lane, then the
                 shuffle tree; + 1 for the division
  rstd           rstd (e_var / (2 (var + eps)) + 5 u), e_var = ((d + 3) u sum d^2 + 2 e_mean
                 sum|d| + N e_mean^2) / N + u var: the rounding of each d = s - mean and d^2, the
                 sum, the mean's own error, the division; 5 u for the add of eps, a 1-ulp sqrtf
                 and a 1-ulp divide
  dg             (D + 4) u sum_m |dy keep sc xh| (+ u |prefill| when accumulating): 2 u |xh| is
                 the propagated error of xh from the given s and stats, u the product dy sc, u the
                 product with xh; D is the longest accumulation chain:
                   rows per wave + 3 (four waves) + T4 + T1 + 2 + 64 (+ 1 accumulating)
                 T4 / T1 the trips of the four-way unrolled and of the tail loop of
                 ln_part_sum_kernel, 2 the (a0 + a1) + (a2 + a3) fold, 64 the final serial sum
  db             (D + 1) u sum_m |dy keep sc|
  colsum         D u sum_m |x|, D = ceil(rows per block / per) + per + T4 + T1 + 2 + 16

c is not chosen in advance: calibrate() measures, over every input set the GPU tests use, the
worst |f32 evaluation - fp64 reference| of the un-rounded value in units of u A; the f32
evaluation sums each row in the kernel's own order (lane_sum).  C holds 4 times that, rounded up
to the next half: the factor covers the compiler's fma contraction and the device's 1-ulp sqrtf
and divide.  Measured (test_ln_refs_cpu.py::test_calibration_constants re-measures and asserts
4 measured <= C):

  output   measured   C
  s        1.47       6.0
  y        5.78       23.5
  ds       3.60       14.5
  dres     3.79       15.5

The bounds are never measured against a kernel.

Exact, position-coded cases (exact_case): s[m, n] = sigma(m, n) 2^k(m) with sigma(m, 2 i + 1) =
-sigma(m, 2 i), eps = 0: every partial sum of the row is a multiple of 2^k below 2^(k + 12), so
mean == 0 and var == 4^k in any order; rstd == 2^-k up to the device's sqrtf and divide.  g[n] =
(32 + n % 32) 2^(n / 32 - 32) and b[n] = 2 g[n]: y[m, n] is g[n] or 3 g[n], at most 8 significant
bits, so bf16-exact, distinct in every column of a row; the four free signs of a chunk spell
(m + (3 + 2 (m / 16)) chunk) % 16, so a chunk differs from the same chunk of every other row of its
16-row group and whole rows are all different.  A relative error of a few 2^-24 in rstd cannot move g (1 + e) + 2 g off its own bf16 value, so
torch.equal is legitimate (test_ln_refs_cpu.py shows it for +-4 ulp)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from attn_helpers import ln_keep_mask

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
SEED = 0x5EED0123456789AB
EPS = 1e-5
LN_BWD_RPW = 8                     # rows per wave of ln_bwd below the block cap

C = {"s": 6.0, "y": 23.5, "ds": 14.5, "dres": 15.5}


def f32(x) -> float:
    return float(np.float32(x))


def drop_scale(p) -> float:
    """make_attn_drop's f32 1 / (1 - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def bf16_ulp(ref):
    """bf16 spacing at each reference value (0 at 0)."""
    _, e = torch.frexp(ref.double())
    return torch.where(ref == 0, torch.zeros_like(ref, dtype=F64), torch.ldexp(torch.ones_like(ref, dtype=F64), e - 8))


def lrelu_bf16(v, slope):
    """bf16(v > 0 ? v : v * slope) of a bf16 tensor, the multiply in f32 as in the kernels."""
    if slope == 0.0:
        return v
    vf = v.to(F32)
    return torch.where(vf > 0, vf, vf * torch.tensor(slope, dtype=F32)).to(BF16)


def lrelu_grad(pre, slope, dtype):
    """v > 0 ? 1 : slope of the pre-activation (so slope at +0.0 and -0.0)."""
    one = torch.ones(pre.shape, dtype=dtype)
    return one if slope == 0.0 else torch.where(pre.to(F32) > 0, one, one * slope)


def ratio(got, ref, bound):
    """max |got - ref| / bound; a difference where the bound is 0, or a NaN, gives inf."""
    d = (got.detach().cpu().to(F64) - ref).abs()
    r = torch.where(d > 0, d / bound, torch.zeros_like(d))
    return float("inf") if torch.isnan(d).any() else float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------ dispatch --
def cdiv(a, b):
    return -(-a // b)


def strided_trips(R, groups):
    """The two loops of ln_part_sum_kernel (groups = 64) and colsum_f32_kernel (16): group gi
    starts at r = gi, takes four rows a trip while r + 3 groups < R, then one row a trip while
    r < R.  Returns (trips of the unrolled loop of group 0, sorted set of tail trips over the
    groups)."""
    tails, t4_0 = set(), 0
    for gi in range(groups):
        r, t4, t1 = gi, 0, 0
        if r + 3 * groups < R:
            t4 = (R - 1 - 3 * groups - r) // (4 * groups) + 1
            r += 4 * groups * t4
        if r < R:
            t1 = (R - 1 - r) // groups + 1
        tails.add(t1)
        if gi == 0:
            t4_0 = t4
    return t4_0, sorted(tails)


def fwd_dispatch(M, N, rows1=0):
    nc = N // 8
    nch = cdiv(nc, 64)
    if nc % 16 == 0 and nc <= 64 and not rows1:
        blocks = cdiv(M, 16)
        return dict(kernel="g16", inst=nc // 16, blocks=blocks, idle_rows=blocks * 16 - M, lanes=16, nch=nc // 16,
                    last_chunk_lanes=16)
    blocks = cdiv(M, 4)
    return dict(kernel="row", inst=nch, blocks=blocks, idle_rows=blocks * 4 - M, lanes=64, nch=nch,
                last_chunk_lanes=nc - 64 * (nch - 1))


def bwd_dispatch(M, N, nopf=0):
    nblk = min(cdiv(M, 4 * LN_BWD_RPW), 2048)
    rpw = cdiv(M, nblk * 4)
    nc = N // 8
    nch = cdiv(nc, 64)
    t4, tails = strided_trips(nblk, 64)
    return dict(kernel="pf" if (not nopf and nch > 1) else "plain", inst=nch, nblk=nblk, rpw=rpw,
                empty_waves=sum(1 for w in range(nblk * 4) if w * rpw >= M),
                short_waves=sum(1 for w in range(nblk * 4) if w * rpw < M < (w + 1) * rpw),
                last_chunk_lanes=nc - 64 * (nch - 1), lds_bytes=4 * 2 * N * 4, ws_bytes=nblk * 2 * N * 4,
                sum_t4=t4, sum_tails=tails, depth=rpw + 3 + t4 + max(tails) + 2 + 64)


def colsum_dispatch(M, N):
    nblk = min(cdiv(M, 256), 1024)
    nc = N // 8
    per = 256 // nc
    if M == 0:
        return dict(kernel="memset", nblk=0, rpb=0, per=per, idle_threads=256 - per * nc, depth=0, ws_bytes=0)
    rpb = cdiv(M, nblk)
    t4, tails = strided_trips(nblk, 16)
    return dict(kernel="sum", nblk=nblk, rpb=rpb, per=per, idle_threads=256 - per * nc,
                rows_per_lane=cdiv(rpb, per), last_block_rows=M - (nblk - 1) * rpb, ws_bytes=nblk * N * 4,
                sum_t4=t4, sum_tails=tails, depth=cdiv(rpb, per) + per + t4 + max(tails) + 2 + 16)


# -------------------------------------------------------------------- shapes --
MODES = {
    "plain": dict(),
    "res": dict(res=True),
    "p_r": dict(res=True, p_r=0.25),
    "p_out": dict(p_out=0.19),
    "both": dict(res=True, p_r=0.1, p_out=0.19),
    "slope_x": dict(slope_x=0.05),
    "slope_r": dict(res=True, slope_r=0.05),
    "slope_r+p_r": dict(res=True, slope_r=0.05, p_r=0.25),
}
MODE_NAMES = tuple(MODES)

ROW_N = (8, 64, 136, 504, 512, 520, 1024, 1032, 1536, 1544, 2040, 2048)
ROW_M = (1, 3, 4, 5)
G16_N = (128, 256, 384, 512)
G16_M = (1, 15, 16, 17, 33)
BWD_M = (1, 31, 32, 33, 45, 257)
CAP_M = 65536 + 37
CAP = ((CAP_M, 8, "slope_r+p_r"), (CAP_M, 136, "slope_x"))
PART_R = (1, 63, 64, 65, 192, 193, 256, 257, 449, 2048)
MODE_SHAPES = ((5, 136), (33, 384), (45, 1032))
EXACT_ROW = tuple((6, n) for n in (8, 520, 1032, 1544, 2048))
EXACT_G16 = tuple((18, n) for n in G16_N)
COLSUM_N = (8, 24, 384, 520, 1032, 2048)
COLSUM_M = (0, 1, 255, 256, 257)
COLSUM_R = (15, 16, 17, 48, 49, 64, 65, 1024)
COLSUM_BIG_M = 262144 + 300


def sweep_mode(i, j):
    """The mode of the j-th M at the i-th N of a sweep: every mode meets many shapes."""
    return MODE_NAMES[(3 * i + j) % len(MODE_NAMES)]


def fwd_row_cases():
    return [(m, n, sweep_mode(i, j)) for i, n in enumerate(ROW_N) for j, m in enumerate(ROW_M)]


def fwd_g16_cases():
    return [(m, n, sweep_mode(i + 1, j)) for i, n in enumerate(G16_N) for j, m in enumerate(G16_M)]


def bwd_cases():
    return [(m, n, sweep_mode(i + 2, j)) for i, n in enumerate(ROW_N) for j, m in enumerate(BWD_M)]


def part_cases():
    return [(32 * r, 8, "p_out") for r in PART_R]


def mode_cases():
    return [(m, n, mode) for m, n in MODE_SHAPES for mode in MODE_NAMES]


def all_ln_cases():
    seen, out = set(), []
    for c in fwd_row_cases() + fwd_g16_cases() + bwd_cases() + part_cases() + mode_cases() + list(CAP):
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def colsum_cases():
    out = [(m, n) for n in COLSUM_N for m in COLSUM_M] + [(256 * r, 8) for r in COLSUM_R] + [(COLSUM_BIG_M, 8)]
    return list(dict.fromkeys(out))


# -------------------------------------------------------------------- inputs --
def _rand_bf16(gen, M, N, amp):
    t = (torch.randn(M, N, generator=gen) * amp).to(BF16)
    t[0, ::5] = 0.0                                       # exact +0.0 and -0.0 under both slopes
    t[-1, 1::7] = -0.0
    return t


def make_s(x, r, keep_r, sc_r, slope_x, slope_r):
    """(xa, ra, s as the kernel's mul-then-add, s as an fma, un-rounded fp64 s, A_s)."""
    xa = lrelu_bf16(x, slope_x)
    if r is None:
        return xa, None, x, x, x.to(F64), x.to(F64).abs()
    ra = lrelu_bf16(r, slope_r)
    k32 = torch.ones(x.shape, dtype=F32) if keep_r is None else keep_r.to(F32) * torch.tensor(sc_r, dtype=F32)
    s_ma = (xa.to(F32) + ra.to(F32) * k32).to(BF16)
    s64 = xa.to(F64) + ra.to(F64) * k32.to(F64)           # exact: 8 + 24 bits, nearby exponents
    return xa, ra, s_ma, s64.to(F32).to(BF16), s64, xa.to(F64).abs() + (ra.to(F64) * k32.to(F64)).abs()


@functools.lru_cache(maxsize=3)
def build(M, N, mode):
    """The input set of (M, N, mode), deterministic; the same object serves the CPU proofs and the
    GPU tests (do not modify it)."""
    o = dict(res=False, p_r=0.0, p_out=0.0, slope_x=0.0, slope_r=0.0)
    o.update(MODES[mode])
    gen = torch.Generator().manual_seed(1000003 * M + 101 * N + MODE_NAMES.index(mode))
    c = SimpleNamespace(M=M, N=N, mode=mode, eps=f32(EPS), seed=SEED, res=o["res"], p_r=o["p_r"], p_out=o["p_out"],
                        slope_x=f32(o["slope_x"]), slope_r=f32(o["slope_r"]))
    c.sc_r, c.sc_o = drop_scale(c.p_r), drop_scale(c.p_out)
    c.x = _rand_bf16(gen, M, N, 1.0)
    c.r = _rand_bf16(gen, M, N, 0.5) if c.res else None
    c.dy = _rand_bf16(gen, M, N, 1.0)
    c.g = (1.0 + 0.5 * torch.randn(N, generator=gen)).to(F32)
    c.b = (0.1 * torch.randn(N, generator=gen)).to(F32)
    c.keep_r = torch.from_numpy(ln_keep_mask(SEED, 0, M, N, c.p_r)) if c.p_r > 0 else None
    c.keep_o = torch.from_numpy(ln_keep_mask(SEED, 1, M, N, c.p_out)) if c.p_out > 0 else None
    for _ in range(4):                                    # make s independent of fma contraction
        c.xa, c.ra, s_ma, s_fma, c.s64, c.A_s = make_s(c.x, c.r, c.keep_r, c.sc_r, c.slope_x, c.slope_r)
        bad = s_ma.view(torch.int16) != s_fma.view(torch.int16)
        if not bool(bad.any()):
            break
        c.r = torch.where(bad, torch.zeros_like(c.r), c.r)
    c.s_ambiguous = int(bad.sum())
    c.s = s_ma                                            # what the backward is given (x without r)
    c.v = c.s if c.res else c.xa                          # what is normalised
    mean, var, rstd = row_stats(c.v, c.eps, F64)
    c.stats = torch.stack([mean, rstd], -1).to(F32)       # the backward's given f32 statistics
    return c


def exact_case(M, N):
    """Position-coded inputs with an exact answer (module docstring): x = 3 s / 4, r = s / 4."""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    code = (m + (3 + 2 * (m // 16)) * (n // 8)) % 16      # 4 sign bits per 8-column chunk: (m, chunk)
    sig = (1 - 2 * ((code >> ((n // 2) % 4)) & 1)) * (1 - 2 * (n % 2))
    k = (m % 7) - 3
    s = sig.to(F64) * torch.exp2(k.to(F64))
    g = ((32 + n[0] % 32).to(F64) * torch.exp2((n[0] // 32 - 32).to(F64)))
    c = SimpleNamespace(M=M, N=N, eps=0.0, x=(0.75 * s).to(BF16), r=(0.25 * s).to(BF16), s=s.to(BF16),
                        g=g.to(F32), b=(2 * g).to(F32), sig=sig)
    c.v = c.s
    c.y = (sig.to(F64) * g + 2 * g).to(BF16)
    c.mean = torch.zeros(M, dtype=F64)
    c.rstd = torch.exp2(-k[:, 0].to(F64))
    assert torch.equal(c.x.to(F64) + c.r.to(F64), s) and torch.equal(c.y.to(F64), sig.to(F64) * g + 2 * g)
    return c


# ------------------------------------------------------------ the operations --
def lane_sum(v, lanes):
    """Row sums of v [M, N] in the kernels' order: chunk cc of 8 columns belongs to lane cc %
    lanes; a lane adds its values serially (chunk by chunk, column by column), then the xor
    shuffle tree folds the lanes (wave_sum / gsum16)."""
    M, n = v.shape
    nch = cdiv(n // 8, lanes)
    t = torch.zeros(M, nch * lanes * 8, dtype=v.dtype)
    t[:, :n] = v
    t = t.view(M, nch, lanes, 8)
    acc = torch.zeros(M, lanes, dtype=v.dtype)
    for ch in range(nch):
        for j in range(8):
            acc = acc + t[:, ch, :, j]
    o, idx = lanes // 2, torch.arange(lanes)
    while o >= 1:
        acc = acc + acc[:, idx ^ o]
        o //= 2
    return acc[:, 0]


def _rowsum(v, dtype, lanes):
    return v.sum(-1) if dtype == F64 else lane_sum(v, lanes)


def row_stats(v, eps, dtype, lanes=64):
    """(mean, var, rstd) of the bf16 rows v."""
    N = v.shape[1]
    vv = v.to(dtype)
    mean = _rowsum(vv, dtype, lanes) / N
    d = vv - mean[:, None]
    var = _rowsum(d * d, dtype, lanes) / N
    return mean, var, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dtype))


def _keep(keep, sc, shape, dtype):
    return torch.ones(shape, dtype=dtype) if keep is None else keep.to(dtype) * torch.tensor(sc, dtype=F32).to(dtype)


def forward(c, dtype=F64, lanes=64, rstd_scale=None):
    """Un-rounded (y, mean, rstd) from the definite bf16 c.v."""
    mean, var, rstd = row_stats(c.v, c.eps, dtype, lanes)
    if rstd_scale is not None:
        rstd = rstd * rstd_scale
    ko = _keep(getattr(c, "keep_o", None), getattr(c, "sc_o", 1.0), c.v.shape, dtype)
    y = ((c.v.to(dtype) - mean[:, None]) * rstd[:, None] * c.g.to(dtype) + c.b.to(dtype)) * ko
    return SimpleNamespace(y=y, mean=mean, var=var, rstd=rstd)


def forward_bounds(c, ref, lanes, nch):
    """(bound of y, A of y, bound of mean, bound of rstd) around the fp64 ``ref``."""
    N = c.N
    v = c.v.to(F64)
    d = 8 * nch + int(math.log2(lanes))
    mabs = v.abs().mean(-1)
    ko = _keep(getattr(c, "keep_o", None), getattr(c, "sc_o", 1.0), v.shape, F64)
    A = ko * (ref.rstd[:, None] * c.g.to(F64).abs() * (v.abs() + mabs[:, None]) + c.b.to(F64).abs())
    by = bf16_ulp(ref.y) / 2 + C["y"] * U * A
    bm = (d + 1) * U * mabs
    dd = v - ref.mean[:, None]
    evar = ((d + 3) * U * (dd * dd).sum(-1) + 2 * bm * dd.abs().sum(-1) + N * bm * bm) / N + U * ref.var
    br = ref.rstd * (0.5 * evar / (ref.var + c.eps) + 5 * U)
    return by, A, bm, br


def backward(c, dtype=F64):
    """Un-rounded (ds, dres, dg, db) from the given c.s, c.stats, c.dy: isolated from the forward."""
    N = c.N
    v = (lrelu_bf16(c.s, c.slope_x) if c.slope_x != 0.0 else c.s).to(dtype)
    mean, rstd = c.stats[:, 0:1].to(dtype), c.stats[:, 1:2].to(dtype)
    dyk = c.dy.to(dtype) * _keep(c.keep_o, c.sc_o, v.shape, dtype)
    xh = (v - mean) * rstd
    gy = dyk * c.g.to(dtype)
    a1 = _rowsum(gy, dtype, 64)[:, None] / N
    a2 = _rowsum(gy * xh, dtype, 64)[:, None] / N
    o = rstd * (gy - a1 - xh * a2)
    r = SimpleNamespace(o=o, ds=o * lrelu_grad(c.s, c.slope_x, dtype), dres=None, xh=xh, gy=gy, dyk=dyk,
                        dg=(dyk * xh).sum(0), db=dyk.sum(0))
    if c.p_r > 0 or c.slope_r != 0.0:
        r.dres = o * _keep(c.keep_r, c.sc_r, v.shape, dtype) * lrelu_grad(c.r, c.slope_r, dtype)
    return r


def backward_bounds(c, ref, depth, prefill_g=None, prefill_b=None):
    """(bound ds, A ds, bound dres, A dres, bound dg, bound db) around the fp64 ``ref``."""
    rstd = c.stats[:, 1:2].to(F64)
    A = rstd * (ref.gy.abs() + ref.gy.abs().mean(-1, keepdim=True)
                + ref.xh.abs() * (ref.gy * ref.xh).abs().mean(-1, keepdim=True))
    Ads = A * lrelu_grad(c.s, c.slope_x, F64)
    bds = bf16_ulp(ref.ds) / 2 + C["ds"] * U * Ads
    Adr = bdr = None
    if ref.dres is not None:
        Adr = A * _keep(c.keep_r, c.sc_r, A.shape, F64) * lrelu_grad(c.r, c.slope_r, F64)
        bdr = bf16_ulp(ref.dres) / 2 + C["dres"] * U * Adr
    acc = 0 if prefill_g is None else 1
    bdg = (depth + acc + 4) * U * (ref.dyk * ref.xh).abs().sum(0)
    bdb = (depth + acc + 1) * U * ref.dyk.abs().sum(0)
    if acc:
        bdg = bdg + U * prefill_g.to(F64).abs()
        bdb = bdb + U * prefill_b.to(F64).abs()
    return bds, Ads, bdr, Adr, bdg, bdb


def to_bf16(t):
    """The bf16 rounding of an evaluation's un-rounded value (through f32, as the kernels store)."""
    return t.to(F32).to(BF16)


def colsum_input(M, N):
    gen = torch.Generator().manual_seed(7919 * M + N)
    return torch.randn(M, N, generator=gen).to(BF16)


def colsum(x, dtype=F64):
    return x.to(dtype).sum(0)


def colsum_bound(x, depth):
    return depth * U * x.to(F64).abs().sum(0)


# --------------------------------------------------------------- calibration --
def calibrate(c):
    """Worst |f32 evaluation - fp64 reference| / (u A) of the un-rounded s, y, ds, dres of one
    input set (the f32 rows summed in the kernels' order, 64 and 16 lanes)."""
    def worst(a, b, A):
        d = (a.to(F64) - b).abs()
        assert bool((d[A == 0] == 0).all())
        return float((d[A > 0] / (U * A[A > 0])).max()) if bool((A > 0).any()) else 0.0

    out = dict(s=0.0, y=0.0, ds=0.0, dres=0.0)
    if c.res:
        k32 = _keep(c.keep_r, c.sc_r, c.x.shape, F32)
        out["s"] = worst(c.xa.to(F32) + c.ra.to(F32) * k32, c.s64, c.A_s)
    f64 = forward(c, F64)
    for lanes in (64, 16) if (c.N // 8) % 16 == 0 and c.N <= 512 else (64,):
        nch = cdiv(c.N // 8, lanes)
        _, A, _, _ = forward_bounds(c, f64, lanes, nch)
        out["y"] = max(out["y"], worst(forward(c, F32, lanes).y, f64.y, A))
    b64, b32 = backward(c, F64), backward(c, F32)
    _, Ads, _, Adr, _, _ = backward_bounds(c, b64, 0)
    out["ds"] = worst(b32.ds, b64.ds, Ads)
    if b64.dres is not None:
        out["dres"] = worst(b32.dres, b64.dres, Adr)
    return out
