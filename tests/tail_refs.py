"""fp64 restatements of the block-tail family (csrc/tail.hip tail_kernel<D, PRE, NC>, csrc/tailw.hip
tailw_body<G, PROJ> and projw_kernel) for the kernel-level tests, with the kernels' two inner bf16
roundings, derived per-element bounds, the input families and the shape tables
(tests/test_tail_refs_cpu.py proves them, tests/test_gpu_block_tail.py runs them).  Every function
takes the operand VALUES as the kernels receive them (bf16 att, x, w_o, w1, w2g; f32 b_o, g1, be1 and
the ffn_vec table [b1 | b2' | c1 | g2 | be2]; eps) and evaluates in float64 on the device of its
first tensor.  bf16_ulp, rne_bf16, near_midpoint, ratio and the constants C come from sgemm_refs.

The function (tail_ref; pre = False starts at x1, the input of snvrag_tail_ffn_forward)
  v1  = x + att W_o^T + b_o                x1 = bf16(LN1(v1) g1 + be1)
  a   = lrelu(x1 W1^T + b1)                (hm, hr) = LN_f mean / rstd of the UNROUNDED a over 4 D
  h   = bf16(a)                            p  = hr (h W2g^T - hm c1) + b2'
  v2  = x1 + lrelu(p)                      out = LN2(v2) g2 + be2   (the residual is the bf16 x1)
  every LayerNorm one-pass, as the kernels take it: rstd = 1 / sqrt(max(E[v^2] - mean^2, 0) + eps);
  lrelu's slope is 0.1.

Roundings.  x1 (packed into B fragments) and h (epi_pair / epi_piece) are rounded to bf16 inside the
kernel.  As sgemm_refs does for the MLP hidden, the reference rounds its fp64 value and FLAGS the
elements whose fp64 value lies within the element's own pre-rounding error of a bf16 midpoint: only
those may come out as another bf16 number.  An unflagged element is the same bf16 number in the
kernel and here, so its pre-rounding error does not reach the next GEMM.  A flagged element's two
roundings are at most its pre-rounding error + one ulp apart (|rne(y) - rne(y')| <= ulp / 2 + d + ulp / 2):
e = d + ulp.  Where d is a rounding error of f32 arithmetic that is one ulp; but a hidden unit fed by
a flagged x1_k has d = |w1[j, k]| e1_k, which is several of ITS ulps when |a_j| is small, and all of
it arrives (test_flagged_allowance_carries_the_pre_rounding_error: with e = ulp alone, an emulation
whose flagged x1 take their other neighbour leaves the bound).  A flagged x1_k moves z1_j by at most
|w1[j, k]| e1_k and its own residual by e1_k; a flagged h_j moves h W2g^T by |w2g[n, j]| eh_j, scaled
by hr; both then pass through LN2 like any other error of v2.

Bounds, per element, u = 2^-24, constants in C (sgemm_refs.C where the operation is the same)
  GEMM  z = x W^T + b:  dz = (Kn + C.acc) u (sum_k |x_k||w_k| + |b|),  Kn the number of non-zero
        products (adding an exact zero is exact): Kn roundings of the MFMA accumulation, one of the
        bias (the C operand in tail.hip, an add after the drain in tailw.hip), three to spare.
  lrelu a = max(z, 0.1f z):  da = dz + 2 u |a|  (the product's rounding and the f32 constant 0.1f,
        which is 0.1 (1 + 0.25 u)).
  stats one-pass sums of n values v with errors dv, the longest serial chain d of either kernel: in
        tail.hip a lane adds D / 2 values and one shuffle for LN1 and LN2 (d = D / 2 + 1) and 2 D
        values and one shuffle for LN_f (d = 2 D + 1); tailw.hip adds 24 (LN1, LN2) or 192 (LN_f)
        per lane, the shuffle and a four-way LDS combine, which is shorter.  With the multiply by
        the rounded 1 / n:
          amean = (d + 2) u mean|v|                      dmean = amean + mean(dv)
          dvar  = 2 mean(|v - mean| dv) + mean(dv^2)       the inputs' errors: the variance of v + e is
                                                           that of v + 2 mean((v - mean) e) + var(e)
                + (d + 3) u mean(v^2) + 2 |mean| amean + amean^2 + 3 u mean(v^2)
                                                           the one-pass arithmetic on those inputs: the sum
                                                           of squares, the mean squared, the subtraction
        rstd is then taken over the INTERVAL [max(var - dvar, 0), var + dvar] + eps, not to first
        order (sgemm_refs._ln_tail linearises, fixes d = D / 2 + 1 and has no folded form; a
        constant row has dvar above eps and only the clamp keeps rstd bounded):
          drstd = max(1 / sqrt(lo) - rstd, rstd - 1 / sqrt(hi)) + (3 + C.sqrt + C.div) u / sqrt(lo)
  LN    y = (v - mean) rstd g + be:  dy = |g| ((rstd + drstd)(dv + dmean) + |v - mean| drstd) + C.ln u
        (|g| (rstd + drstd)(|v| + |mean|) + |be|)  — the forms of both kernels ((v - mean) rstd g + be;
        fma(fma(v, rstd, -mean rstd), g, be)) are four roundings against these magnitudes.
  x1    v1 = z + x with dv1 = dz + u |v1|; x1 = bf16(y1), flagged by near_midpoint(y1, dy1), allowance
        e1 = [flagged] (ulp(|y1| + dy1) + dy1).
  FFN1  dz1 = (Kn + C.acc) u A1 + sum_k |w1[j, k]| e1_k; da as above; h flagged by near_midpoint(a, da),
        allowance eh = [flagged] (ulp(|a| + da) + da).
  FFN2  s = h W2g^T:  ds = (Kn + C.acc) u sum |h||w2g| + sum_j |w2g[n, j]| eh_j.  The folded LN_f is
        hr fma(-hm, c1, s) + b2' in tail.hip and fma(s, hr, fma(c1, -hm hr, b2')) in tailw.hip; one
        bound covers both:  dp = (hr + dhr)(ds + |c1| dhm) + |s - hm c1| dhr + C.fold u (hr (|s| + |hm c1|) +
        |b2'|)  (both forms multiply s and hm c1 by the one computed hr, so its error meets their
        difference; the cancellation between them is in the rounding term).
  LN2   v2 = x1 + lrelu(p):  dv2 = dp + 2 u |lrelu(p)| + u |v2| + e1, then the LN bound with d = D / 2 + 1.
  out   ulp_bf16(out) / 2 + dout.
  proj  ref = x W^T + b:  ulp_bf16(ref) / 2 + (Kn + C.acc) u (sum |x||w| + |b|).
The bounds are never measured against a kernel.

Families (named constructors, seeded, bf16-exact, no subnormals), D in 128, 256, 384
  sparse   W_o, W1, W2g with four non-zeros per row, +-1/4 or +-1/2, placed so that every (k16 step,
           32-row tile) fragment of every weight holds one (W_o / W1 in the B fragments' feature
           order of mfma32.h in_feat, W2g in the packed hidden order: 16 consecutive units); x, att,
           g1, g2, be2 at the existing tests' scale; b1 and b2' randn in full f32 (with bf16-exact
           biases a sum of four bf16 products +-2^-k x1 lands exactly on a bf16 midpoint for one
           hidden unit in six, which the reference must flag); b_o a multiple of 1/32 (ln_rows needs
           x - b_o exact); be1 = 2 + 0.1 randn, so that |x1| is seldom below 1/4 — LN1's error is
           absolute, bf16 spacing relative, and small x1 would be flagged wholesale.
  phase_a  sparse with W1 = 0: the hidden is lrelu(b1) for every row, a flagged x1 moves only its
           own output.
  low_var  every scale proportional to delta = 2^-9 (eps = 1e-5) or 2^-6 (eps = 1e-3), about sqrt(eps / 2):
           x, b_o, be1, b1, b2' = (a constant of 4 to 8 + a small integer) delta, att a small integer times
           delta, g1 about 2 delta, W1 sparse with entries of 1/16 and 1/8, W2g sparse with entries of
           delta / 2 and delta: the variance LN1, LN_f and LN2 see is within a factor 4 of eps on every
           row, and no mean is above 8 standard deviations (the one-pass cancellation stays small).
  ln_rows  sparse with three rows written in (att = 0 there): v1 constant 1 (variance 0: the clamp
           decides, rstd = 1 / sqrt(eps)), v1 = 2 e_5 (one non-zero), v1 = 4 +- 1/16, half of the features each (the
           mean 64 standard deviations) — in the first tile (SPECIAL_ROWS) and again in the last 229
           rows of M_SPLIT (SPLIT_ROWS), which tail_split = 64 gives to the 32-row bodies.  The
           bound grows there by its own formula.
  dense    randn x, randn / sqrt(D) W, randn b: the projections only."""
import functools
from types import SimpleNamespace

import torch

import sgemm_refs as R

F64, F32, BF16 = R.F64, R.F32, R.BF16
U = R.U
SLOPE = 0.1
EPS_LIST = (1e-5, 1e-3)
C = dict(R.C, fold=4)     # u A_p: -hm hr, the two fmas of the folded LN_f, one to spare
bf16_ulp, rne_bf16, near_midpoint, ratio, f32 = R.bf16_ulp, R.rne_bf16, R.near_midpoint, R.ratio, R.f32
FAMILIES = ("sparse", "phase_a", "ln_rows", "low_var")


def _d(t, dev):
    return t.detach().to(dev).to(F64)


def gemm3(x, w):
    """(x W^T, sum |x||w|, the number of non-zero products) of fp64 operands."""
    return x @ w.T, x.abs() @ w.abs().T, (x != 0).to(F64) @ (w != 0).to(F64).T


def lrelu(z):
    return torch.where(z >= 0, z, z * SLOPE)


def row_stats(v, dv, d, eps):
    """One-pass mean / variance / rstd of the rows of v with their error bounds (module docstring)."""
    m = lambda t: t.mean(-1, keepdim=True)
    mean, msq = m(v), m(v * v)
    var = (msq - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    am = (d + 2) * U * m(v.abs())                                            # the arithmetic of the mean
    dm = am + m(dv)
    dvar = (2 * m((v - mean).abs() * dv) + m(dv * dv)                        # the inputs' own errors
            + (d + 3) * U * msq + 2 * mean.abs() * am + am * am + 3 * U * msq)   # the one-pass arithmetic
    lo, hi = (var - dvar).clamp_min(0.0) + eps, var + dvar + eps
    rlo = 1.0 / torch.sqrt(lo)
    dr = torch.maximum(rlo - rstd, rstd - 1.0 / torch.sqrt(hi)) + (3 + C["sqrt"] + C["div"]) * U * rlo
    return SimpleNamespace(mean=mean, var=var, rstd=rstd, dm=dm, dr=dr, rmax=rstd + dr)


def ln_out(v, dv, st, g, be):
    """(y, dy) of y = (v - mean) rstd g + be evaluated in f32 from the statistics st."""
    y = (v - st.mean) * st.rstd * g + be
    dy = (g.abs() * (st.rmax * (dv + st.dm) + (v - st.mean).abs() * st.dr)
          + C["ln"] * U * (g.abs() * st.rmax * (v.abs() + st.mean.abs()) + be.abs()))
    return y, dy


def split_vec(vec, D, dev):
    """(b1, b2', c1, g2, be2) of the ffn_vec table."""
    v = _d(vec, dev)
    return v[:4 * D], v[4 * D:5 * D], v[5 * D:6 * D], v[6 * D:7 * D], v[7 * D:8 * D]


def tail_ref(att, x, w_o, w1, w2g, b_o, g1, be1, vec, eps, pre=True, rounding=True, carry_d=True):
    """out, bound, x1_flag, h_flag (+ the intermediate quantities the CPU test looks at).  pre = False:
    x is x1 itself (att, w_o, b_o, g1, be1 unused, may be None).  rounding = False: neither bf16
    rounding nor any flag — the plain formula of test_tail32_kernel.  carry_d = False: a flagged
    element's allowance is one ulp without its pre-rounding error — too small a bound, there only
    for the CPU test that shows it to be."""
    cd = 1.0 if carry_d else 0.0
    dev = (att if pre else x).device
    D = x.shape[1]
    b1, b2, c1, g2, be2 = split_vec(vec, D, dev)
    o = SimpleNamespace()
    if pre:
        z, A, Kn = gemm3(_d(att, dev), _d(w_o, dev))
        bo = _d(b_o, dev)
        v1 = z + bo + _d(x, dev)
        dv1 = (Kn + C["acc"]) * U * (A + bo.abs()) + U * v1.abs()
        s1 = row_stats(v1, dv1, D // 2 + 1, eps)
        y1, dy1 = ln_out(v1, dv1, s1, _d(g1, dev), _d(be1, dev))
        o.var1, o.y1, o.dy1 = s1.var, y1, dy1
        if rounding:
            x1 = rne_bf16(y1)
            o.x1_flag = near_midpoint(y1, dy1)
            e1 = o.x1_flag.to(F64) * (bf16_ulp(y1.abs() + dy1) + cd * dy1)
        else:
            x1, o.x1_flag, e1 = y1, torch.zeros_like(y1, dtype=torch.bool), torch.zeros_like(y1)
    else:
        x1 = _d(x, dev)
        o.x1_flag, e1 = torch.zeros_like(x1, dtype=torch.bool), torch.zeros_like(x1)
    o.x1 = x1
    w1d = _d(w1, dev)
    z1, A1, K1 = gemm3(x1, w1d)
    z1 = z1 + b1
    dz1 = (K1 + C["acc"]) * U * (A1 + b1.abs()) + e1 @ w1d.abs().T
    a = lrelu(z1)
    da = dz1 + 2 * U * a.abs()
    sf = row_stats(a, da, 2 * D + 1, eps)
    o.varf, o.hm, o.hr = sf.var, sf.mean, sf.rstd
    if rounding:
        h = rne_bf16(a)
        o.h_flag = near_midpoint(a, da)
        eh = o.h_flag.to(F64) * (bf16_ulp(a.abs() + da) + cd * da)
    else:
        h, o.h_flag, eh = a, torch.zeros_like(a, dtype=torch.bool), torch.zeros_like(a)
    o.a, o.h = a, h
    w2d = _d(w2g, dev)
    s, A2, K2 = gemm3(h, w2d)
    fl = eh @ w2d.abs().T
    ds = (K2 + C["acc"]) * U * A2 + fl
    p = sf.rstd * (s - sf.mean * c1) + b2
    mag = s.abs() + (sf.mean * c1).abs()
    dp = sf.rmax * (ds + c1.abs() * sf.dm) + (s - sf.mean * c1).abs() * sf.dr + C["fold"] * U * (sf.rmax * mag + b2.abs())
    uu = lrelu(p)
    v2 = x1 + uu
    dv2 = dp + 2 * U * uu.abs() + U * v2.abs() + e1
    s2 = row_stats(v2, dv2, D // 2 + 1, eps)
    o.var2 = s2.var
    o.out, dout = ln_out(v2, dv2, s2, g2, be2)
    o.half_ulp = bf16_ulp(o.out) / 2
    o.bound = o.half_ulp + dout
    o.flag_term = g2.abs() * s2.rmax * (sf.rmax * fl + e1)
    # outputs a flagged element feeds directly (its own residual, a non-zero w2g entry); what a flagged
    # element does to the row statistics is inside dout
    o.fed_by_flag = (fl > 0) | o.x1_flag
    o.dout = dout
    return o


def proj_ref(x, w, b):
    """out, bound of x W^T + b rounded once to bf16."""
    dev = x.device
    z, A, Kn = gemm3(_d(x, dev), _d(w, dev))
    bd = _d(b, dev)
    ref = z + bd
    return SimpleNamespace(out=ref, bound=bf16_ulp(ref) / 2 + (Kn + C["acc"]) * U * (A + bd.abs()))


# -------------------------------------------------------------------- shapes --
DS = (128, 256, 384)
NCH = {128: 8, 256: 16, 384: 24}                     # 64-unit hidden chunks: rot = blockIdx % NCH
M_SMALL = (1, 31, 32, 33, 127, 128, 129)             # one row; both sides of a wave's / token group's 32 rows
#                                                      and of the 128-row workgroup; a one-row second tile
M_SPLIT = 257 * 128 + 32 * 3 + 5                     # > 256 tiles + 3 tiles + 5 rows: with tail_split = 64 the
#                                                      remainder runs as 32-row (G = 1) workgroups, the last
#                                                      ragged with 5 rows; with tail_split = 0 as 128-row tiles
SPLITS = (64, 0)
SPECIAL_ROWS = (2, 37, 70)                           # ln_rows: constant, one non-zero, mean = 64 std
SPLIT_ROWS = (M_SPLIT - 3, M_SPLIT - 229 + 75, M_SPLIT - 229 + 8)   # the same three in M_SPLIT's last 229 rows: the
#                                                      constant row in the ragged 5-row workgroup, the others
#                                                      in the third and the first of the eight 32-row workgroups


def rot_m(D):
    """128 NCH + 1: every chunk rotation of the stream plus a one-row tile (3073 at D = 384)."""
    return 128 * NCH[D] + 1


def tail_m(D):
    """tail_kernel<D, PRE>: 128-row workgroups, a wave owns 32 rows."""
    return M_SMALL + (rot_m(D),)


def proj_m(D, NC, wide=False):
    """tail_kernel<D, false, NC>: rot = blockIdx % NC, so 128 NC + 1 reaches every rotation (at NC = 1
    that is M_SMALL's 129).  wide (projw_kernel): and 160, a tile and one token group of the next."""
    return tuple(dict.fromkeys(M_SMALL + ((160,) if wide else ()) + (128 * NC + 1,)))


WIDE_M = M_SMALL + (160,)                            # + a tile and one token group of the next
MMAX = {128: rot_m(128), 256: rot_m(256), 384: M_SPLIT}


# -------------------------------------------------------------------- inputs --
_gen, _bf = R._gen, R._bf


def frag_cols(kind, s):
    """The 16 weight columns of k16 step s: W_o / W1 in the B fragments' feature order (mfma32.h
    in_feat: 32 (s / 2) + 8 (s % 2) + {0 .. 7, 16 .. 23}); W2g ('w2') 16 consecutive hidden units."""
    if kind == "w2":
        return list(range(16 * s, 16 * s + 16))
    base = 32 * (s >> 1) + 8 * (s & 1)
    return [base + j for j in range(8)] + [base + 16 + j for j in range(8)]


def frag_index(kind, cols):
    """column -> k16 step."""
    idx = torch.empty(cols, dtype=torch.long)
    for s in range(cols // 16):
        idx[frag_cols(kind, s)] = s
    return idx


def fragments_covered(w, kind):
    """True where every (32-row tile, k16 step) fragment of w holds a non-zero."""
    rows, cols = w.shape
    nz = (w.float() != 0).view(rows // 32, 32, cols).any(1)                   # [tiles, cols]
    per = torch.zeros(rows // 32, cols // 16).index_add_(1, frag_index(kind, cols), nz.float())
    return bool((per > 0).all())


def sparse_w(rows, cols, kind, seed, nnz=4, scale=1.0):
    """nnz entries per row, +-scale / 4 or +-scale / 2: row i of tile t has them in k16 steps (nnz i + j +
    5 t) mod KS, j < nnz — 32 nnz consecutive steps per tile, so every fragment holds one."""
    g = _gen(rows, cols, seed)
    KS = cols // 16
    assert 32 * nnz >= KS and nnz <= KS
    table = torch.tensor([frag_cols(kind, s) for s in range(KS)])
    r = torch.arange(rows)
    pick = torch.randint(0, 16, (rows, nnz), generator=g)
    val = (torch.randint(0, 2, (rows, nnz), generator=g) * 2 - 1).float() * (0.25 * (1 + torch.randint(0, 2, (rows, nnz), generator=g)))
    w = torch.zeros(rows, cols)
    for j in range(nnz):
        s = ((r % 32) * nnz + j + 5 * (r // 32)) % KS
        w[r, table[s, pick[:, j]]] = val[:, j] * scale
    return w.to(BF16)


def _vec(*parts):
    return torch.cat([t.float().reshape(-1) for t in parts]).contiguous()


def _finish(c):
    c.c1 = c.w2g.double().sum(1).float()                # ffn_vec: row sums of the bf16 w2g
    c.vec = _vec(c.b1, c.b2, c.c1, c.g2, c.be2)
    return c


@functools.lru_cache(maxsize=None)
def sparse(D, M):
    """Do not modify the result (cached).  The weights and every vector are drawn before the rows and
    do not depend on M; the M rows of x and att are one draw each, so another M has other rows of
    the same distribution (the GPU tests take every M as a row prefix of one case)."""
    g = _gen(D, 31)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(D=D, eps=None)
    c.w_o, c.w1, c.w2g = sparse_w(D, D, "w", 32), sparse_w(4 * D, D, "w", 33), sparse_w(D, 4 * D, "w2", 34)
    c.b_o = torch.randint(-8, 9, (D,), generator=g).float() / 32
    c.g1, c.be1 = _bf(1 + 0.2 * rn(D)).float(), _bf(2 + 0.1 * rn(D)).float()
    c.b1, c.b2 = rn(4 * D), rn(D)                       # f32, not bf16-exact (module docstring)
    c.g2, c.be2 = _bf(1 + 0.2 * rn(D)).float(), _bf(0.1 * rn(D)).float()
    c.x, c.att = _bf(rn(M, D)), _bf(0.5 * rn(M, D))
    c.x1 = c.x                                           # the input of the FFN-only entry
    return _finish(c)


@functools.lru_cache(maxsize=None)
def phase_a(D, M):
    c = SimpleNamespace(**vars(sparse(D, M)))
    c.w1 = torch.zeros_like(c.w1)
    return _finish(c)


@functools.lru_cache(maxsize=None)
def ln_rows(D, M):
    c = SimpleNamespace(**vars(sparse(D, M)))
    g = _gen(D, 35)
    x, att = c.x.clone().float(), c.att.clone()
    j = torch.where(torch.randperm(D, generator=g) < D // 2, 2.0, -2.0) / 32
    e5 = torch.zeros(D)
    e5[5] = 2.0
    rows = [torch.ones(D), e5, 4 + j]
    x1 = x.clone()
    where = [(r, v) for r, v in zip(SPECIAL_ROWS + SPLIT_ROWS, rows + rows) if r < M]
    for r, v in where:
        att[r] = 0
        x[r] = v - c.b_o
        x1[r] = v
    c.x, c.att, c.x1 = x.to(BF16), att, x1.to(BF16)
    assert all(torch.equal(c.x[r].float() + c.b_o, v) for r, v in where)
    return _finish(c)


def delta_of(eps):
    return {1e-5: 2.0 ** -9, 1e-3: 2.0 ** -6}[eps]


@functools.lru_cache(maxsize=None)
def low_var(D, M, eps):
    g = _gen(D, 36)
    d = delta_of(eps)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    c = SimpleNamespace(D=D, eps=eps)
    c.w_o = sparse_w(D, D, "w", 37)
    c.w1, c.w2g = sparse_w(4 * D, D, "w", 38, scale=0.25), sparse_w(D, 4 * D, "w2", 39, scale=2 * d)
    c.b_o = (4 + ri(-1, 1, D)) * d
    c.g1, c.be1 = (4 + ri(-1, 1, D)) * d / 2, (8 + ri(-1, 1, D)) * d
    c.b1, c.b2 = (8 + ri(-2, 2, 4 * D)) * d, (4 + ri(-1, 1, D)) * d
    c.g2, c.be2 = sparse(D, 1).g2, sparse(D, 1).be2
    # the rows after every vector, so that the vectors do not depend on M (as in sparse)
    c.x = ((4 + torch.arange(M)[:, None] % 5 + ri(-3, 3, M, D)) * d).to(BF16)
    c.att = (ri(-2, 2, M, D) * d).to(BF16)
    c.x1 = ((8 + ri(-3, 3, M, D)) * d).to(BF16)
    for t in (c.x, c.att, c.x1, c.w1, c.w2g):
        assert torch.equal(t.float().to(BF16), t) and float(t.float().abs()[t.float() != 0].min()) >= 2.0 ** -126
    return _finish(c)


def case(family, D, M, eps=1e-5):
    """The operands of a family with Mmax = M rows; rows(c, M) takes a prefix."""
    return low_var(D, M, eps) if family == "low_var" else {"sparse": sparse, "phase_a": phase_a, "ln_rows": ln_rows}[family](D, M)


def ref_of(c, eps, pre, dev="cpu", M=None, rounding=True, carry_d=True):
    """tail_ref on the first M rows of a case, operands moved to dev."""
    t = lambda v: v[:M].to(dev) if M is not None else v.to(dev)
    if pre:
        return tail_ref(t(c.att), t(c.x), c.w_o.to(dev), c.w1, c.w2g, c.b_o, c.g1, c.be1, c.vec, f32(eps), True, rounding,
                        carry_d)
    return tail_ref(None, t(c.x1), None, c.w1, c.w2g, None, None, None, c.vec, f32(eps), False, rounding, carry_d)


@functools.lru_cache(maxsize=None)
def dense_proj(D, NC, M):
    """W and b before the rows: they do not depend on M."""
    g = _gen(D, NC, 40)
    w, b = _bf(torch.randn(NC * D, D, generator=g) / D ** 0.5), _bf(torch.randn(NC * D, generator=g)).float()
    return SimpleNamespace(x=_bf(torch.randn(M, D, generator=g)), w=w, b=b)


@functools.lru_cache(maxsize=None)
def sparse_proj(D, NC, M):
    g = _gen(D, NC, 41)
    b = _bf(torch.randn(NC * D, generator=g)).float()
    return SimpleNamespace(x=_bf(torch.randn(M, D, generator=g)), w=sparse_w(NC * D, D, "w", 42), b=b)
