"""fp64 restatement of the dense layer snvrag_linear / snvrag_linear_ex (include/snvrag.h; csrc/gemm.hip
linear_kernel<TI, TO>, csrc/gemm_rows.hip rows_gemm_kernel<TI, TO, NW, ROWNORM>) for the kernel-level
tests, with derived per-element bounds, a restatement of the dispatch and the shape tables the tests
sweep (tests/test_dense_refs_cpu.py proves them, tests/test_gpu_dense_gemm.py runs them).  linear()
evaluates in float64 on the device of its first argument and takes the operand VALUES as given
(bf16 and f32 inputs are exact in fp64); leading dimensions are the GPU test's business.  The GELUs,
the LayerNorm bound, ratio / rne_bf16 / bf16_ulp and the exact-answer inputs are those of
tests/sgemm_refs.py (imported as S), not restated.

What the kernels compute, in their order
  acc   sum_k A[m, k] W[n, k] in f32 MFMA accumulators, K-tile after K-tile.
  rn    row-norm (ROWNORM): s, ss = the sums of the n_parts (sum, sumsq) partials of row m, mean = s /
        dim, var = max(ss / dim - mean^2, 0), rstd = 1 / sqrt(var + eps); acc <- rstd acc - rstd mean c1.
  z     acc + bias + row1[(m % period) s1] col1 + row2[(m % period) s2] col2 (period 0: m itself).
  y     act(z): GELU is gelu_bf16 (S.gelu_poly64) in the row-panel kernel with a bf16 output and the
        exact-erf gelu_erf (S.gelu_erf64) everywhere else — every f32 output, and the 128-tile kernel
        for both output types (linear_kernel calls apply_act, not apply_act_t); lrelu; sigmoid.
  v     y + resid.  Without LN this is the output; stats_out holds per column tile (sum v, sum v^2)
        of the un-rounded v, laid out [tile][M].
  LN    (row-panel, N == the tile width) y = (v - mean) rstd g + b, ln_act(y) (exact-erf GELU, lrelu
        with slope 0, sigmoid), then post_base + post_scale (y maf(post_af[m % post_af_period])) where
        post_base is given; maf(af) = min(log1p(1 / (min(af, 1 - af) + 1e-6f)), 3) (csrc/mfma32.h).

Bounds, per element, u = 2^-24, every constant in C
  z     dz = (p Kn + C.acc) u A, A = sum_k |a||w| + |bias| + |r1 c1| + |r2 c2|, Kn the non-zero products
        of the element, p = 1 for bf16 operands (a product of two bf16 numbers is exact in f32: one
        rounding per accumulated product) and 2 for f32 operands (v_mfma_f32_16x16x4_f32: the product
        is allowed a rounding of its own).  C.acc = 5: the bias add, a product and a sum per rank term
        where the compiler does not contract them.
  rn    A = rstd (sum |a||w'| + |mean||c1|) + ..., C.rn = 3 more roundings (rstd acc, (rstd mean) c1,
        their sum), plus the error of rstd and of rstd mean from the f32 sums of n_parts partials
        (n_parts roundings each on sum |s_p|, sum |ss_p|), the two divisions (C.div ulp), the product
        mean^2, the subtraction, the add of eps, sqrtf and the divide (C.sqrt, C.div ulp): dvar is
        carried through 1 / sqrt exactly (both ends of [var - dvar, var + dvar]), not to first order.
  act   gelu_bf16: S.gelu_err.  gelu_erf: 1.13 dz + dz^2 + |z| (C.erfc_as + C.erfc_eval u) / 2 + 2 u |y|
        (Abramowitz & Stegun 7.1.26's 1.5e-7 on erfc, twelve roundings of its f32 evaluation, the final
        fma and product).  lrelu: max(1, |slope|) dz + u |y|.  sigmoid: s (1 - s) dz + dz^2 + s
        (S.C.sigmoid + |z|) u.
  v     dy + u |v| where a residual is added.
  LN    S._ln_tail (one-pass bound; the kernel's two-pass variance is inside it), then the activation
        and dout = |scale| (w dy + |y| dw + dy dw) + 3 u (|base| + |scale y w|), dw = C.maf u max(w, 1).
  out   bf16: + half a bf16 ulp of the reference.  f32: nothing more.
  stats a lane adds CPL 8 values serially, then log2(RL) group_sum steps (d = stats_depth(BN)):
        ds = d u sum |v| + sum dv,  dss = (d + 1) u sum v^2 + sum (2 |v| dv + dv^2).
The bounds are never measured against a kernel.

Inputs.  Dense: randn x, randn / sqrt(K) weights rounded to the input type, no subnormals.  Exact:
S.exact_case's signed selection matrix and integers (every partial sum an integer below 2^24, the
output an integer of at most 256, or a power-of-two multiple of one under row-norm): bound 0, bit for
bit."""
import functools
import math
from types import SimpleNamespace

import torch

import sgemm_refs as S
from sgemm_refs import (BF16, F32, F64, U, bf16_ulp, gelu_erf64, gelu_err, gelu_poly64, ratio,  # noqa: F401
                        rne_bf16)

ACT_NONE, ACT_GELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3
SLOPE = 0.1
EPS = 1e-5

C = {
    "acc": 5,             # dz = (p Kn + acc) u A
    "rn": 3,              # rstd acc, (rstd mean) c1, their sum
    "div": 1, "sqrt": 1,  # f32 ulps of x / y, sqrtf
    "gelu_slope": 1.13,   # max |gelu'|
    "erfc_as": 1.5e-7,    # Abramowitz & Stegun 7.1.26, |erfc error|
    "erfc_eval": 12,      # u: rcp, five FMAs on values <= 1.5, exp2 and its argument, t q e
    "maf": 8,             # u max(w, 1): 1 - af, + 1e-6f, the reciprocal, log1pf at 2 ulp
}

MAF_EPS = S.f32(1e-6)


def _d(t, dev):
    return t.detach().to(F64).to(dev)


def spec(**kw):
    """The epilogue of one call: snvrag_epilogue_t's fields by value (resid / post_base [M, N]), stats
    (bool: stats_out wanted) and rownorm = SimpleNamespace(stats [P, M, 2], n_parts, dim, eps, c1)."""
    e = SimpleNamespace(bias=None, row1=None, s1=1, col1=None, row2=None, s2=1, col2=None, period=0, act=ACT_NONE,
                        slope=0.0, resid=None, ln_g=None, ln_b=None, ln_eps=0.0, ln_act=ACT_NONE, post_base=None,
                        post_scale=1.0, post_af=None, post_af_period=0, post_maf=0, stats=False, rownorm=None)
    for k, v in kw.items():
        assert hasattr(e, k), k
        setattr(e, k, v)
    return e


def row_index(M, period, dev="cpu"):
    m = torch.arange(M, device=dev)
    return m % period if period > 0 else m


def gelu_kind(kernel, tout):
    return "poly" if kernel == "rows" and tout == BF16 else "erf"


def act_ref(code, z, dz, slope, gelu):
    """(act(z), its error) for a z known to dz."""
    if code == ACT_NONE:
        return z, dz
    if code == ACT_GELU:
        if gelu == "poly":
            return gelu_poly64(z), gelu_err(z, dz)
        y = gelu_erf64(z)
        return y, C["gelu_slope"] * dz + dz * dz + z.abs() * (C["erfc_as"] + C["erfc_eval"] * U) / 2 + 2 * U * y.abs()
    if code == ACT_LRELU:
        y = torch.where(z >= 0, z, z * slope)
        return y, max(1.0, abs(slope)) * dz + U * y.abs()
    s = torch.sigmoid(z)
    return s, s * (1 - s) * dz + dz * dz + s * (S.C["sigmoid"] + z.abs()) * U


def maf64(af):
    """maf_w of csrc/mfma32.h in fp64, with its f32 constant."""
    m = torch.minimum(af, 1.0 - af)
    return torch.log1p(1.0 / (m + MAF_EPS)).clamp_max(3.0)


def stats_depth(bn):
    """Additions behind one lane's row sum: CPL 8 values serially, then log2(RL) group_sum steps."""
    rl = 16 if bn // 8 >= 16 else bn // 8
    return (bn // 8 // rl) * 8 + int(math.log2(rl))


def rownorm_ref(rn, M, dev="cpu"):
    """mean, rstd of the rows from the n_parts partials as the kernel forms them, with their errors."""
    st = _d(rn.stats, dev)[:rn.n_parts, :M]
    P = rn.n_parts
    s, ss = st[..., 0].sum(0), st[..., 1].sum(0)
    mean, q = s / rn.dim, ss / rn.dim
    var = (q - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + rn.eps)
    dmean = P * U * st[..., 0].abs().sum(0) / rn.dim + 2 * C["div"] * U * mean.abs()
    dq = P * U * st[..., 1].abs().sum(0) / rn.dim + 2 * C["div"] * U * q.abs()
    dvar = dq + 2 * mean.abs() * dmean + dmean * dmean + U * (2 * mean * mean + q.abs()) + U * (var + rn.eps)
    hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + rn.eps)
    lo = 1.0 / torch.sqrt(var + dvar + rn.eps)
    drstd = torch.maximum(hi - rstd, rstd - lo) + 2 * (C["sqrt"] + C["div"]) * U * hi
    rm = rstd * mean
    drm = mean.abs() * drstd + rstd * dmean + drstd * dmean + U * rm.abs()
    return SimpleNamespace(mean=mean, var=var, rstd=rstd, dmean=dmean, drstd=drstd, drm=drm)


def linear(a, w, e=None, tin=BF16, tout=BF16, kernel="rows", bn=None, g=None, M=None, gelu=None):
    """The contract of include/snvrag.h for rows [0, M) of a (g: an S.gemm of at least those rows).
    out / bound [M, N]; v / dv the value before LN; stats / stats_bound [N / bn, M, 2] where e.stats."""
    e = spec() if e is None else e
    g = S.gemm(a, w) if g is None else g
    M = a.shape[0] if M is None else M
    dev = g.z.device
    N = g.z.shape[1]
    acc, Ag, Kn = g.z[:M], g.A[:M], g.K[:M]
    p = 1 if tin == BF16 else 2
    z, A, extra, cnt = acc, Ag, 0.0, C["acc"]
    if e.rownorm is not None:
        r = rownorm_ref(e.rownorm, M, dev)
        c1 = _d(e.rownorm.c1, dev)
        z = r.rstd[:, None] * acc - (r.rstd * r.mean)[:, None] * c1
        A = r.rstd[:, None] * (Ag + r.mean.abs()[:, None] * c1.abs())
        extra = r.drstd[:, None] * (acc.abs() + (p * Kn + C["acc"]) * U * Ag) + r.drm[:, None] * c1.abs()
        cnt += C["rn"]
    if e.bias is not None:
        b = _d(e.bias, dev)
        z, A = z + b, A + b.abs()
    ri = row_index(M, e.period, dev)
    for row, s, col in ((e.row1, e.s1, e.col1), (e.row2, e.s2, e.col2)):
        if row is not None:
            t = _d(row, dev)[ri * s, None] * _d(col, dev)
            z, A = z + t, A + t.abs()
    dz = (p * Kn + cnt) * U * A + extra
    y, dy = act_ref(e.act, z, dz, e.slope, gelu or gelu_kind(kernel, tout))
    v, dv = y, dy
    if e.resid is not None:
        v = y + _d(e.resid, dev)[:M]
        dv = dy + U * v.abs()
    o = SimpleNamespace(z=z, dz=dz, v=v, dv=dv, out=v, err=dv)
    if e.ln_g is not None:
        ln = S._ln_tail(v, dv, e.ln_g, e.ln_b, e.ln_eps, half=False)
        o.out, o.err = act_ref(e.ln_act, ln.out, ln.bound, 0.0, "erf")
        if e.post_base is not None:
            base = _d(e.post_base, dev)[:M]
            wgt, dw = torch.ones(M, 1, dtype=F64, device=dev), torch.zeros(M, 1, dtype=F64, device=dev)
            if e.post_maf:
                wgt = maf64(_d(e.post_af, dev)[row_index(M, e.post_af_period, dev)])[:, None]
                dw = C["maf"] * U * wgt.clamp_min(1.0)
            sc = abs(e.post_scale)
            out = base + e.post_scale * (o.out * wgt)
            o.err = sc * (wgt * o.err + o.out.abs() * dw + o.err * dw) + 3 * U * (base.abs() + sc * (o.out * wgt).abs())
            o.out = out
    o.bound = o.err + (bf16_ulp(o.out) / 2 if tout == BF16 else 0.0)
    if e.stats:
        T = N // bn
        vt, dvt = v.view(M, T, bn), dv.view(M, T, bn)
        d = stats_depth(bn)
        o.stats = torch.stack([vt.sum(-1).T, (vt * vt).sum(-1).T], -1)
        o.stats_bound = torch.stack([d * U * vt.abs().sum(-1).T + dvt.sum(-1).T,
                                     (d + 1) * U * (vt * vt).sum(-1).T + (2 * vt.abs() * dvt + dvt * dvt).sum(-1).T], -1)
    return o


# ------------------------------------------------------------------ dispatch --
TN = {F32: "float", BF16: "bf16"}
PAIRS = [(BF16, BF16), (BF16, F32), (F32, F32), (F32, BF16)]
NWS = (6, 4, 2, 1)
R_BM = 128


def ept(tin):
    """K elements of one 128-byte K-tile."""
    return 64 if tin == BF16 else 32


def rows_name(tin, tout, nw, rn):
    return f"rows_gemm_kernel<{TN[tin]}, {TN[tout]}, {nw}, {'true' if rn else 'false'}>"


def tile_name(tin, tout):
    return f"linear_kernel<{TN[tin]}, {TN[tout]}>"


ALL_INSTANCES = ([rows_name(ti, to, nw, rn) for ti, to in PAIRS for nw in NWS for rn in (False, True)]
                 + [tile_name(ti, to) for ti, to in PAIRS])


def rows_pick_nw(N, full=False, force=0):
    """rows_pick_nw of csrc/gemm_rows.hip: 6, 4, 2, 1 in that order; 0 = unsupported."""
    if force and not full and N % (64 * force) == 0 and force in (1, 2, 4, 6):
        return force
    for c in (6, 4, 2, 1):
        if (N == 64 * c) if full else (N % (64 * c) == 0):
            return c
    return 0


def cdiv(a, b):
    return -(-a // b)


def dispatch(tin, tout, M, N, K, ln=False, stats=False, rownorm=False, tile128=0, nw=0):
    """What snvrag_linear_ex launches: name, kernel ('rows' | 'tile'), bn (tile width), tiles_n, grid;
    ValueError where it refuses."""
    if K % 8 or N % (8 if tout == BF16 else 4):
        raise ValueError("K % 8, N % 16 bytes")
    fused = ln or stats or rownorm
    rows_ok = N % 64 == 0 and K % ept(tin) == 0 and not tile128
    if fused or rows_ok:
        c = rows_pick_nw(N, ln, nw)
        if not c or K % ept(tin):
            raise ValueError("row-panel GEMM: N % 64 (LN: N in 64, 128, 256, 384), K % 128 bytes")
        tn = N // (64 * c)
        return SimpleNamespace(name=rows_name(tin, tout, c, rownorm), kernel="rows", nw=c, bn=64 * c, tiles_n=tn,
                               grid=tn * cdiv(M, R_BM))
    tn = cdiv(N, 128)
    return SimpleNamespace(name=tile_name(tin, tout), kernel="tile", nw=0, bn=128, tiles_n=tn, grid=tn * cdiv(M, 128))


def xcd_remap(nwg, orig):
    """The workgroup a block index becomes (both kernels): blocks of one XCD take consecutive tiles."""
    q8, r8, xcd = nwg // 8, nwg % 8, orig % 8
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + orig // 8


# -------------------------------------------------------------------- shapes --
ROWS_N = {6: (384, 1152), 4: (256, 512), 2: (128, 640), 1: (64, 320)}
ROWS_K = {BF16: (64, 128, 192), F32: (32, 64, 96)}
ROWS_M = (1, 63, 64, 65, 127, 128, 129, 257)
ROWS_BIG = {6: (257, 1152), 4: (641, 512), 2: (257, 640), 1: (257, 320)}     # > 8 workgroups, not a multiple of 8
RN_PARTS = (1, 2, 5)
TILE_N = (8, 72, 136, 200)
TILE_K = {BF16: (8, 72, 136), F32: (8, 40, 72)}
TILE_M = (1, 3, 127, 128, 129, 641)
MMAX = 641 + 7
PADS = dict(lda=8, ldw=16, ldc=8, ld_resid=16, ld_post=24)


def periods(M):
    """row_period: none, 1, inside a 64-row half, at the tile's 128 rows, beyond M."""
    return (0, 1, 37, 128, M + 7)


# Epilogues of the sweeps without LN.  rank: (stride1, stride2) or None; pad: padded leading dimensions.
FORMS = (
    dict(act=ACT_NONE, bias=True, rank=None, resid=False, pad=False),
    dict(act=ACT_GELU, bias=True, rank=(1, 2), resid=True, pad=True),
    dict(act=ACT_LRELU, bias=False, rank=(2, 1), resid=False, pad=True),
    dict(act=ACT_SIGMOID, bias=True, rank=None, resid=True, pad=False),
    dict(act=ACT_GELU, bias=False, rank=(1, 1), resid=False, pad=False),
    dict(act=ACT_NONE, bias=True, rank=(2, 2), resid=True, pad=True),
)
# LN tails: ln_act, post (0 none, 1 base, 2 base with maf), post_af_period kind (0 none, 1 inside)
LN_FORMS = (
    dict(ln_act=ACT_NONE, post=0, afp=0),
    dict(ln_act=ACT_GELU, post=1, afp=0),
    dict(ln_act=ACT_NONE, post=2, afp=0),
    dict(ln_act=ACT_LRELU, post=2, afp=1),
    dict(ln_act=ACT_SIGMOID, post=0, afp=0),
)
AF_PERIOD = 29


def rows_cases(tin, nw):
    """(M, N, K, i): the row-panel sweep of one (input type, NW); i numbers the case."""
    out = [(M, N, K) for N in ROWS_N[nw] for K in ROWS_K[tin] for M in ROWS_M]
    out.append((*ROWS_BIG[nw], ROWS_K[tin][2]))
    return [(M, N, K, i) for i, (M, N, K) in enumerate(out)]


def ln_cases(tin, nw):
    return [(M, 64 * nw, K, i) for i, (M, K) in enumerate((M, K) for K in ROWS_K[tin] for M in ROWS_M)]


def tile_cases(tin):
    """The 128-tile sweep: its own shapes, then row-panel shapes (reached through gemm_tile128)."""
    out = [(M, N, K, 0) for N in TILE_N for K in TILE_K[tin] for M in TILE_M]
    out += [(M, N, ROWS_K[tin][k], 1) for k, (M, N) in enumerate(((129, 384), (257, 320), (65, 512)))]
    return [(M, N, K, t, i) for i, (M, N, K, t) in enumerate(out)]


def form_of(i, M):
    """(form, period) of case i: 6 forms against 5 periods, so every pair meets many shapes."""
    f = FORMS[i % len(FORMS)]
    return f, (periods(M)[i % 5] if f["rank"] else 0)


def all_table_instances():
    """instantiation -> number of table cases that launch it."""
    out = {}

    def add(name):
        out[name] = out.get(name, 0) + 1
    for ti, to in PAIRS:
        for nw in NWS:
            for M, N, K, _ in rows_cases(ti, nw):
                add(dispatch(ti, to, M, N, K).name)
                add(dispatch(ti, to, M, N, K, stats=True).name)
                add(dispatch(ti, to, M, N, K, rownorm=True).name)           # n_parts = RN_PARTS[i % 3]
            for M, N, K, _ in ln_cases(ti, nw):
                add(dispatch(ti, to, M, N, K, ln=True).name)
        for M, N, K, t, _ in tile_cases(ti):
            add(dispatch(ti, to, M, N, K, tile128=t).name)
    return out


# -------------------------------------------------------------------- inputs --
def _round(t, dt):
    return S._bf(t) if dt == BF16 else t.to(F32)


@functools.lru_cache(maxsize=None)
def base(tin, K, N):
    """x [MMAX, K], W [N, K] in the input type: every M of a table is a row prefix.  Do not modify."""
    g = S._gen(K, N, 31 + (tin == F32))
    c = SimpleNamespace(K=K, N=N, x=_round(torch.randn(MMAX, K, generator=g), tin),
                        w=_round(torch.randn(N, K, generator=g) / math.sqrt(K), tin))
    c.x[0, ::7] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def base_gemm(tin, K, N, dev="cpu"):
    c = base(tin, K, N)
    return S.gemm(c.x.to(dev), c.w.to(dev))


@functools.lru_cache(maxsize=None)
def vecs(tout, N):
    """The epilogue material of an (output type, N): f32 vectors, residual and post_base in the output
    type, rank scalars for stride 2, allele frequencies.  Do not modify."""
    g = S._gen(N, 37 + (tout == F32))
    v = SimpleNamespace(bias=torch.randn(N, generator=g), col1=torch.randn(N, generator=g), col2=torch.randn(N, generator=g),
                        c1=torch.randn(N, generator=g), row1=torch.rand(2 * MMAX, generator=g),
                        row2=torch.rand(2 * MMAX, generator=g) - 0.5,
                        resid=_round(torch.randn(MMAX, N, generator=g), tout),
                        post_base=_round(torch.randn(MMAX, N, generator=g), tout), post_af=torch.rand(MMAX, generator=g),
                        ln_g=torch.rand(N, generator=g) + 0.5, ln_b=torch.randn(N, generator=g))
    v.post_af[:4] = torch.tensor([0.0, 1.0, 0.5, 0.04])
    return v


def selection_w(tin, K, N):
    """S.exact_case's signed selection matrix: one non-zero product per output, so dz = 6 u A and the
    activation's own error is what the bound holds (the dense dz at K = 192 exceeds the 2.6e-5 between
    the two GELUs)."""
    return S.exact_case(K, 1, N).w.to(tin)


def rows_needed(M, period):
    return min(M, period) if period > 0 else M


def make_spec(tout, N, M, form, period, ln_form=None, stats=False):
    """The epilogue of a table case: rank vectors exactly (rows - 1) stride + 1 long."""
    v = vecs(tout, N)
    e = spec(act=form["act"], slope=SLOPE if form["act"] == ACT_LRELU else 0.0, period=period, stats=stats)
    if form["bias"]:
        e.bias = v.bias
    if form["rank"]:
        e.s1, e.s2 = form["rank"]
        n = rows_needed(M, period)
        e.row1, e.col1 = v.row1[:(n - 1) * e.s1 + 1], v.col1
        e.row2, e.col2 = v.row2[:(n - 1) * e.s2 + 1], v.col2
    if form["resid"]:
        e.resid = v.resid[:M]
    if ln_form is not None:
        e.ln_g, e.ln_b, e.ln_eps, e.ln_act = v.ln_g, v.ln_b, S.f32(EPS), ln_form["ln_act"]
        if ln_form["post"]:
            e.post_base, e.post_scale = v.post_base[:M], 0.75
        if ln_form["post"] == 2:
            e.post_maf = 1
            e.post_af_period = AF_PERIOD if ln_form["afp"] else 0
            e.post_af = v.post_af[:rows_needed(M, e.post_af_period)]
    return e


def row_partials(x, n_parts):
    """(sum, sumsq) of the rows of x over n_parts contiguous, uneven column groups, from fp64, rounded
    to f32: [n_parts, M, 2]."""
    K = x.shape[1]
    cuts = [round(K * (i / n_parts) ** 1.5) for i in range(n_parts + 1)]
    xd = x.double()
    return torch.stack([torch.stack([xd[:, a:b].sum(-1), (xd[:, a:b] ** 2).sum(-1)], -1)
                        for a, b in zip(cuts[:-1], cuts[1:])]).float()


def make_rownorm(tin, tout, K, N, M, n_parts):
    c = base(tin, K, N)
    return SimpleNamespace(stats=row_partials(c.x[:M], n_parts), n_parts=n_parts, dim=K, eps=S.f32(EPS), c1=vecs(tout, N).c1)


# ---------------------------------------------------------- exact-answer case --
def exact_case(tin, tout, K, M, N, period=0, strides=(1, 1), resid=False, rownorm=0, stats_bn=0):
    """S.exact_case in the types of the call, the rank scalars spread to their strides, an integer
    residual in [-8, 8]; rownorm = n_parts > 0: rows with mean in {0, 1, 2, -1} and rstd in {1, 1/2, 1/4}
    (eps 0, stats exact in f32), so the output is a power-of-two multiple of an integer below 256.  out,
    and stats [N / stats_bn, M, 2], are exact in f32 and out in the output type."""
    c = S.exact_case(K, M, N, period if period > 0 else (M if strides else None))
    it = F32 if tin == F32 else BF16
    e = spec(bias=c.b)
    x64, w64 = c.x.double(), c.w.double()
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    v = x64 @ w64.T
    if rownorm:
        mean = torch.tensor([0.0, 1.0, 2.0, -1.0])[torch.arange(M) % 4].double()
        k = (torch.arange(M) // 4) % 3
        rstd = 2.0 ** -k.double()
        q = 4.0 ** k.double() + mean * mean                  # ss / dim, var = 4^k
        st = torch.zeros(rownorm, M, 2, dtype=F64)
        st[0, :, 0], st[0, :, 1] = mean * K, q * K
        if rownorm > 1:                                      # the other partials cancel exactly
            st[0, :, 0] -= 64.0
            st[-1, :, 0] += 64.0
            st[0, :, 1] -= 32.0
            st[1, :, 1] += 32.0
        assert torch.equal(st[..., 0].sum(0), mean * K) and torch.equal(st[..., 1].sum(0), q * K)
        c1 = ((3 * n[0]) % 5 - 2).double()
        e.rownorm = SimpleNamespace(stats=st.float(), n_parts=rownorm, dim=K, eps=0.0, c1=c1.float())
        v = rstd[:, None] * v - (rstd * mean)[:, None] * c1
    v = v + c.b.double()
    if c.rank is not None:
        r1, r2, p, c1, c2 = c.rank
        e.s1, e.s2 = strides
        e.row1, e.row2 = torch.zeros((p - 1) * e.s1 + 1), torch.zeros((p - 1) * e.s2 + 1)
        e.row1[::e.s1], e.row2[::e.s2] = r1, r2
        e.col1, e.col2, e.period = c1, c2, period
        ri = row_index(M, period)
        v = v + r1.double()[ri, None] * c1.double() + r2.double()[ri, None] * c2.double()
    if resid:
        r = ((3 * m + 5 * n) % 17 - 8).double()
        e.resid = r.to(tout)
        v = v + r
    out = v.to(tout)
    assert torch.equal(out.double(), v), "exact case: the output is not representable"
    o = SimpleNamespace(x=c.x.to(it), w=c.w.to(it), e=e, out=out, col=c.col)
    if stats_bn:
        e.stats = True
        vt = v.view(M, N // stats_bn, stats_bn)
        o.stats = torch.stack([vt.sum(-1).T, (vt * vt).sum(-1).T], -1)
        assert float(o.stats.abs().max()) < 2.0 ** 24 and float(vt.abs().sum(-1).max()) < 2.0 ** 24
        o.stats = o.stats.float()
    return o
