"""fp64 restatements of the stream-GEMM family (csrc/sgemm.hip: sg_kernel's ACT / LN / HEAD2 epilogues
and its concatenated-input form, mlp_kernel and its AF-gate prologue) for the kernel-level tests,
with derived per-element bounds, a restatement of the dispatch and the shape tables the tests sweep
(tests/test_sgemm_refs_cpu.py proves them, tests/test_gpu_stream_gemm.py runs them).  Every function
evaluates in float64 on the device of its first argument and takes the operand VALUES as given (the
bf16 inputs are exact in fp64).

Roundings the references model
  CAT   x2 g2 is a product of two bf16 values, exact in f32: its bf16 rounding is definite and the
        reference applies it; no allowance.
  MLP   the hidden h = bf16(gelu(z1)) and, for AFG, the input x = bf16(CrossAFInteraction) are
        rounded inside the kernel.  The reference rounds its fp64 value and FLAGS the elements whose
        fp64 value lies within the element's own pre-rounding error of a bf16 rounding midpoint:
        only those may come out one bf16 ulp away; an unflagged element is the same bf16 number in
        the kernel and here, so its pre-rounding error does not reach the second GEMM at all.

GELU  gelu_poly64 restates gelu_bf16 (csrc/common.h) with its three coefficients and its clamp, an
exact exp and an exact division: the ACT / GELU epilogue, the HEAD2 hidden and the MLP hidden.
gelu_erf64 is the exact-erf GELU (F.gelu): the AFG prologue, whose gelu_erf common.h states to within
4.2e-7.  |gelu_poly64 - gelu_erf64| <= 2.6e-5 (common.h) is pinned by the CPU test.

Bounds, per element, u = 2^-24, every constant in C
  z     the pre-activation x W^T + b + r1 c1 + r2 c2:  dz = (Kn + C.acc) u A,  A = sum_k |x_k||w_k| +
        |b| + |r1 c1| + |r2 c2| and Kn the number of non-zero products of the element (adding an
        exact zero to an f32 accumulator is exact): Kn roundings of the MFMA accumulation, two of
        the rank FMAs, one of the bias add, one to spare for second-order terms.
  gelu  gelu_bf16 in f32 around gelu_poly64(z):  |g'(z)| dz + dz^2 (propagation) + |z| s ((1 - s)
        (C.poly u |p| + 2 u C.exp2) + 2 u (C.rcp + 1)) + u |y|,  s the sigmoid factor, p its exponent:
        the polynomial's five f32 operations move the exponent by C.poly u |p|, v_exp_f32 and
        v_rcp_f32 are C.exp2 and C.rcp ulps (1 ulp = 2 u relative), one rounding for 1 + e and one
        for the final product.
  bf16 output: ulp_bf16(ref) / 2 + the error of the un-rounded value.
  LN    v = act(z) + x with dv; one-pass statistics as the kernel takes them (a lane adds D / 2
        values serially, one shuffle: d = D / 2 + 1):  dmean = (d + 2) u mean|v| + mean(dv);
        dvar = (d + 3) u mean(v^2) + 2 mean(|v| dv) + 2 |mean| dmean + 3 u mean^2;  drstd = rstd
        (dvar / (2 (var + eps)) + 5 u) (the add of eps, sqrtf and the divide at C.sqrt / C.div ulp);
        y: |g| (rstd (dv + dmean) + |v - mean| drstd) + C.ln u (|g| rstd (|v| + |mean|) + |be|).
  HEAD2 logits: sum_n |w_out[j, n]| dh_n + (N / 2 + 3) u (sum |h||w_out| + |b_out|) (a lane's N / 2
        serial FMAs, the shuffle, the bias).  probs: p (1 - p) (dl0 + dl1) + p (C.softmax + 2 gap) u,
        gap = |l0 - l1|: the subtraction of the maximum and __expf's multiply by log2 e move the
        exponent by u gap each, then exp2, the sum, the divide and the product; + 2^-126, below which an
        f32 result may underflow.
        These f32 outputs have no rounding of their own to hide behind, and the worst-case sum dz,
        carried through 4 D hidden units, is all there is: the kernels reach 0.002 - 0.005 of it, so
        the HEAD2 bound is about 200 times the observed error.  It catches the gross faults of the
        CPU test (a dropped k-step, a shifted bias or w_out), not subtle ones; 0.005 is no margin.
  MLP   y2 = h W2^T + b2:  dy2 = sum_j |w2[n, j]| [flagged_j] ulp_bf16(h_j) + (4 D + C.acc) u
        (sum |w2||h| + |b2|), carried through the sigmoid (s (1 - s) dy2 + dy2^2 + s (C.sigmoid +
        |y2|) u) or the LN above.
  AFG   dx of the prologue, term by term in afgate_err: 3 u per affine map, C.gelu_erf for each
        gelu_erf, C.split for the split-bf16 gate GEMV (hi lo + lo hi kept, lo lo and the rounding
        of lo dropped: 3 2^-18 of sum |w||h|), the LayerNorm from the weight-column moments with
        dvar = C.moments u (the sum of the magnitudes of the closed form's six terms).  A flagged
        input moves z1 by sum_k |w1[j, k]| [flagged_k] ulp_bf16(x_k).
The bounds are never measured against a kernel.

Inputs.  The scale of the existing tests (randn x, randn / sqrt(K) weights), rounded to bf16, no
subnormals.  The MLP and AFG cases take a W1 with eight entries +-1/4 or +-1/2 per row (the same
output scale): with a dense W1 the worst-case dz (K = 384) flags most of the hidden and the flagged
allowance would exceed the output's half ulp, which the CPU test forbids; with Kn = 8 it stays below
a tenth of it."""
import functools
import math
from types import SimpleNamespace

import torch

import frontend_refs as FR

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
EPS = 1e-5
SLOPE = 0.1
RES_SCALE = 0.37

C = {
    "acc": 4,            # dz = (Kn + acc) u A
    "rcp": 1, "exp2": 1, "div": 1, "sqrt": 1,      # f32 ulps of v_rcp_f32, v_exp_f32, 1.0f / x, sqrtf
    "poly": 6,           # u |p|: gelu_bf16's polynomial, five f32 operations and the coefficients' rounding
    "gelu_fit": 2.6e-5,  # common.h: max |gelu_bf16 - exact-erf GELU| over R
    "gelu_erf": 4.2e-7,  # common.h: max |gelu_erf - exact-erf GELU| over R
    "ln": 4,             # u A_y: the subtraction, the two products and the fma of the LN output
    "softmax": 10,       # u p: 2 exp2 + 2 div ulps (2 u each), the sum, the product
    "sigmoid": 8,        # u s: __expf's exp2, 1 + e, v_rcp_f32
    "split": 3 * 2.0 ** -18,   # the AFG gate GEMV in split bf16
    "moments": 8,        # u sum |terms| of the AFG closed-form variance (f32 moments, six terms)
}

# gelu_bf16's coefficients as the f32 numbers of csrc/common.h: p(x) = x (A0 + A1 x^2 + A2 x^4)
_f32 = lambda v: float(torch.tensor(v, dtype=F32))
GA0, GA1, GA2 = _f32(-1.59501577), _f32(-7.40112920e-2), _f32(7.03033577e-4)


def f32(x) -> float:
    return _f32(x)


def _d(t):
    return t.detach().to(F64)


bf16_ulp = FR.bf16_ulp


def rne_bf16(t):
    """The bf16 rounding of an fp64 tensor (through f32, as the kernels store), as fp64."""
    return t.to(F32).to(BF16).to(F64)


def ratio(got, ref, bound):
    """max |got - ref| / bound; a difference where the bound is 0, or a NaN, gives inf."""
    d = (got.detach().cpu().to(F64) - ref.cpu()).abs()
    r = torch.where(d > 0, d / bound.cpu(), torch.zeros_like(d))
    return float("inf") if torch.isnan(d).any() else float(r.max()) if r.numel() else 0.0


def near_midpoint(v, dv):
    """Elements of the fp64 v within dv of a bf16 rounding midpoint (or with dv above a quarter of
    the spacing, where the next binade's midpoints come into reach): their bf16 rounding is not
    decided by v alone."""
    ulp = bf16_ulp(v)
    safe = torch.where(ulp > 0, ulp, torch.ones_like(ulp))
    t = v.abs() / safe
    dist = (t - torch.floor(t) - 0.5).abs() * safe
    return (ulp > 0) & ((dist <= dv) | (dv >= ulp / 4))


# ---------------------------------------------------------------------- GELU --
def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _poly(x):
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    return xc, xc * (x2 * (x2 * GA2 + GA1) + GA0)


def gelu_poly64(x):
    """gelu_bf16 of csrc/common.h in fp64: x / (1 + exp(p(clamp(x, -8, 8))))."""
    return x / (1.0 + torch.exp(_poly(x)[1]))


def gelu_err(z, dz):
    """The error of gelu_bf16 evaluated in f32 at z + e, |e| <= dz, around gelu_poly64(z)."""
    xc, p = _poly(z)
    s = 1.0 / (1.0 + torch.exp(p))
    x2 = xc * xc
    dp = torch.where(z.abs() <= 8.0, GA0 + 3 * GA1 * x2 + 5 * GA2 * x2 * x2, torch.zeros_like(z))
    slope = s + z.abs() * s * (1 - s) * dp.abs()
    ev = z.abs() * s * ((1 - s) * (C["poly"] * U * p.abs() + 2 * U * C["exp2"]) + 2 * U * (C["rcp"] + 1))
    return slope * dz + dz * dz + ev + U * (z * s).abs()


# ------------------------------------------------------------- the operations --
def gemm(x, w):
    """(x W^T, sum |x||w|, the number of non-zero products) — shared by the cases of a table row."""
    x = _d(x)
    w = _d(w).to(x.device)
    return SimpleNamespace(z=x @ w.T, A=x.abs() @ w.abs().T, K=(x != 0).to(F64) @ (w != 0).to(F64).T)


def pre(x, w, b, rank=None, g=None, zx=None):
    """z, dz of the pre-activation.  rank = (r1, r2, period, c1, c2); g a gemm() of at least the
    rows of x; zx an extra |error| of z (a flagged input)."""
    M = x.shape[0]
    g = gemm(x, w) if g is None else g
    b = _d(b).to(g.z.device)
    z, A = g.z[:M] + b, g.A[:M] + b.abs()
    if rank is not None:
        r1, r2, period, c1, c2 = rank
        ri = torch.arange(M, device=z.device) % period
        t1 = _d(r1).to(z.device)[ri, None] * _d(c1).to(z.device)
        t2 = _d(r2).to(z.device)[ri, None] * _d(c2).to(z.device)
        z, A = z + t1 + t2, A + t1.abs() + t2.abs()
    dz = (g.K[:M] + C["acc"]) * U * A
    return SimpleNamespace(z=z, A=A, dz=dz if zx is None else dz + zx)


def act(x, w, b, act="none", rank=None, g=None):
    """ACT: act(x W^T + b + r1[m % period] c1 + r2[m % period] c2), bf16 output."""
    p = pre(x, w, b, rank, g)
    y, dy = (gelu_poly64(p.z), gelu_err(p.z, p.dz)) if act == "gelu" else (p.z, p.dz)
    return SimpleNamespace(out=y, bound=bf16_ulp(y) / 2 + dy, z=p.z, dz=p.dz)


def _ln_tail(v, dv, g, be, eps, half=True):
    """LayerNorm of the un-rounded v (error dv); half: the output is rounded to bf16."""
    D = v.shape[1]
    d = D // 2 + 1
    g, be = _d(g).to(v.device), _d(be).to(v.device)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (v - mean) * rstd * g + be
    dm = (d + 2) * U * v.abs().mean(-1, keepdim=True) + dv.mean(-1, keepdim=True)
    dvar = ((d + 3) * U * (v * v).mean(-1, keepdim=True) + 2 * (v.abs() * dv).mean(-1, keepdim=True)
            + 2 * mean.abs() * dm + 3 * U * mean * mean)
    dr = rstd * (0.5 * dvar / (var + eps) + (3 + C["sqrt"] + C["div"]) * U)
    Ay = g.abs() * rstd * (v.abs() + mean.abs()) + be.abs()
    by = (bf16_ulp(y) / 2 if half else 0.0) + g.abs() * (rstd * (dv + dm) + (v - mean).abs() * dr) + C["ln"] * U * Ay
    return SimpleNamespace(out=y, bound=by, mean=mean, var=var, rstd=rstd)


def ln(x, w, b, rank, g, be, slope, eps, gm=None, mut=None):
    """LN: LayerNorm(lrelu(z) + x) over the D = N features of a row.  mut (the CPU test's faults):
    'no_resid' leaves the residual out, 'round_first' adds it after a bf16 rounding of lrelu(z)."""
    p = pre(x, w, b, rank, gm)
    a = torch.where(p.z >= 0, p.z, p.z * slope)
    da = max(1.0, abs(slope)) * p.dz + U * a.abs()
    xx = _d(x).to(a.device)
    if mut == "no_resid":
        xx = torch.zeros_like(xx)
    if mut == "round_first":
        a = rne_bf16(a)
    v = a + xx
    return _ln_tail(v, da + U * v.abs(), g, be, eps)


def head2(x, w, b, w_out, b_out, g=None):
    """HEAD2: (logits, probs) = softmax(gelu(x W^T + b) w_out^T + b_out), f32 outputs, the hidden
    never rounded to bf16."""
    p = pre(x, w, b, None, g)
    h, dh = gelu_poly64(p.z), gelu_err(p.z, p.dz)
    wo, bo = _d(w_out).to(h.device), _d(b_out).to(h.device)
    logits = h @ wo.T + bo
    Al = h.abs() @ wo.abs().T + bo.abs()
    bl = dh @ wo.abs().T + (w.shape[0] // 2 + 3) * U * Al
    probs = torch.softmax(logits, -1)
    gap = (logits[:, :1] - logits[:, 1:]).abs()
    bp = probs * probs.flip(-1) * bl.sum(-1, keepdim=True) + probs * (C["softmax"] + 2 * gap) * U + 2.0 ** -126
    return SimpleNamespace(logits=logits, probs=probs, bound_logits=bl, bound_probs=bp)


def cat_input(q, x2, g2, period2, swap=False):
    """[q | bf16(x2 g2[m % period2])] as fp64 values."""
    M = q.shape[0]
    ri = torch.arange(M, device=q.device) % period2
    prod = rne_bf16(_d(x2) * _d(g2)[ri])
    return torch.cat([prod, _d(q)] if swap else [_d(q), prod], -1)


def cat(q, x2, g2, period2, w, b):
    """CAT: gelu([q | bf16(x2 g2[m % period2])] W^T + b)."""
    return act(cat_input(q, x2, g2, period2), w, b, "gelu")


def mlp(x, w1, w2, parts, epi2, rank=None, g=None, x_flag=None):
    """MLP: EPI2(bf16(gelu(x W1^T + b1 [+ rank])) W2^T + b2), EPI2 0 = sigmoid, 1 = LayerNorm;
    parts = dict(b1, b2[, g, be, eps]); x_flag [M, D]: ulp_bf16(x) where the (AFG) input is flagged,
    else 0."""
    w1a = _d(w1).abs()
    zx = None if x_flag is None else x_flag @ w1a.to(x_flag.device).T
    p = pre(x, w1, parts["b1"], rank, g, zx)
    h64, dh = gelu_poly64(p.z), gelu_err(p.z, p.dz)
    h = rne_bf16(h64)
    flagged = near_midpoint(h64, dh)
    w2d = _d(w2).to(h.device)
    b2 = _d(parts["b2"]).to(h.device)
    y2 = h @ w2d.T + b2
    A2 = h.abs() @ w2d.abs().T + b2.abs()
    fl = (flagged.to(F64) * bf16_ulp(h64.abs() + dh)) @ w2d.abs().T
    dy2 = fl + (w2.shape[1] + C["acc"]) * U * A2
    if epi2 == 0:
        s = torch.sigmoid(y2)
        sl = s * (1 - s)
        o = SimpleNamespace(out=s, bound=bf16_ulp(s) / 2 + sl * dy2 + dy2 * dy2 + s * (C["sigmoid"] + y2.abs()) * U,
                            flag_term=sl * fl)
    else:
        o = _ln_tail(y2, dy2 + U * y2.abs(), parts["g"], parts["be"], parts["eps"])
        o.flag_term = _d(parts["g"]).to(h.device).abs() * o.rstd * fl
    o.half_ulp = bf16_ulp(o.out) / 2
    o.flag_share = float(flagged.to(F64).mean())
    return o


def afgate_err(af, afp, ag, rs):
    """The f32 error of the AFG prologue's x = af + rs gate enc around FR.af_gate (module docstring)."""
    g1w, g1b, g2w, g2b, jw, jb, lw, lb = [FR._t(t, F64) for t in ag]
    a0, a1 = FR._t(af, F64)[:, None], FR._t(afp, F64)[:, None]
    GP = 1.13                                              # max |gelu'|
    A1 = (g1w[:, 0] * a0).abs() + (g1w[:, 1] * a1).abs() + g1b.abs()
    h1 = gelu_erf64(g1w[:, 0] * a0 + g1w[:, 1] * a1 + g1b)
    dh1 = GP * 3 * U * A1 + C["gelu_erf"]
    gg = h1 @ g2w.T + g2b
    dg = dh1 @ g2w.abs().T + (C["split"] + (96 + C["acc"]) * U) * (h1.abs() @ g2w.abs().T) + U * (gg.abs() + g2b.abs())
    gt = torch.sigmoid(gg)
    dgt = gt * (1 - gt) * dg + gt * (C["sigmoid"] + gg.abs()) * U
    enc = jw[:, 0] * a0 + jw[:, 1] * a1 + jb
    denc = 3 * U * ((jw[:, 0] * a0).abs() + (jw[:, 1] * a1).abs() + jb.abs())
    cols = [jw[:, 0], jw[:, 1], jb]
    mu = [c.mean() for c in cols]
    cc = [c - m for c, m in zip(cols, mu)]
    S = lambda i, j: (cc[i] * cc[j]).mean()
    mean = enc.mean(-1, keepdim=True)
    var = ((enc - mean) ** 2).mean(-1, keepdim=True)
    dmean = 4 * U * ((mu[0] * a0).abs() + (mu[1] * a1).abs() + mu[2].abs())
    T = (a0 * a0 * S(0, 0) + a1 * a1 * S(1, 1) + 2 * ((a0 * a1 * S(0, 1)).abs() + (a0 * S(0, 2)).abs() + (a1 * S(1, 2)).abs())
         + S(2, 2))
    eps = f32(1e-5)
    rstd = 1.0 / torch.sqrt(var + eps)
    drstd = rstd * (0.5 * (C["moments"] * U * T + 2 * U * eps) / (var + eps) + (3 + C["sqrt"] + C["div"]) * U)
    lo = (enc - mean) * rstd * lw + lb
    dlo = lw.abs() * (rstd * (denc + dmean) + (enc - mean).abs() * drstd) + C["ln"] * U * (
        lw.abs() * rstd * (enc.abs() + mean.abs()) + lb.abs())
    e = gelu_erf64(lo)
    de = GP * dlo + C["gelu_erf"]
    return abs(rs) * (gt * de + e.abs() * dgt) + 3 * U * (a0.abs() + (rs * gt * e).abs())


def afgate_mlp(af, afp, ag, rs, w1, w2, b1, b2, dev="cpu"):
    """AFG: sigmoid(bf16(gelu(bf16(CrossAFInteraction(af, af_p)) W1^T + b1)) W2^T + b2)."""
    v = FR.af_gate(af, afp, ag, rs)
    dv = afgate_err(af, afp, ag, rs)
    flag = near_midpoint(v, dv)
    xf = (flag.to(F64) * bf16_ulp(v.abs() + dv)).to(dev)
    o = mlp(rne_bf16(v).to(dev), w1, w2, dict(b1=b1, b2=b2), 0, None, None, xf)
    o.x_flag_share = float(flag.to(F64).mean())
    return o


# ------------------------------------------------------------------ dispatch --
ROWS4, ROWS8 = 128, 256
_EPI = {"act": "SG_ACT", "head2": "SG_HEAD2", "ln": "SG_LN"}
_ACT = {"none": "NONE", "gelu": "GELU", "lrelu": "LRELU"}


def sg_name(D, epi, act, rank, waves=4, cat=False):
    return f"sg_kernel<{D}, {_EPI[epi]}, {_ACT[act]}, {'true' if rank else 'false'}, {waves}{', CAT' if cat else ''}>"


def mlp_name(rank, epi2, afg=False):
    return f"mlp_kernel<384, {'true' if rank else 'false'}, {epi2}{', AFG' if afg else ''}>"


def dispatch(D, epi, act, rank, waves4=False, cat=False):
    """(instantiation, rows per workgroup) that sg_dispatch / snvrag_sgemm_forward /
    snvrag_sgemm_cat_forward launch; ValueError where they refuse."""
    if cat:
        if D != 768:
            raise ValueError("the concatenated input needs D / 2 = 384")
        return sg_name(768, "act", "gelu", False, 4, True), ROWS4
    if D == 768:
        if epi != "act" or act != "gelu" or rank:
            raise ValueError("K = 768 supports the GELU activation epilogue only")
        return sg_name(768, "act", "gelu", False), ROWS4
    if D not in (128, 256, 384):
        raise ValueError("D")
    if epi == "head2":
        if act != "gelu" or rank:
            raise ValueError("head epilogue: GELU, no rank terms")
        return sg_name(D, "head2", "gelu", False), ROWS4
    if epi == "ln":
        if act != "lrelu":
            raise ValueError("LayerNorm epilogue supports LeakyReLU only")
        return sg_name(D, "ln", "lrelu", rank), ROWS4
    if act not in ("none", "gelu"):
        raise ValueError("activation epilogue supports none / GELU")
    if D == 384 and not waves4 and not rank:
        return sg_name(D, "act", act, False, 8), ROWS8
    return sg_name(D, "act", act, rank), ROWS4


SG_INSTANCES = ([sg_name(D, "head2", "gelu", False) for D in (128, 256, 384)]
                + [sg_name(D, "ln", "lrelu", r) for D in (128, 256, 384) for r in (True, False)]
                + [sg_name(D, "act", a, r) for D in (128, 256, 384) for a in ("none", "gelu") for r in (True, False)]
                + [sg_name(384, "act", a, False, 8) for a in ("none", "gelu")]
                + [sg_name(768, "act", "gelu", False), sg_name(768, "act", "gelu", False, 4, True)])
MLP_INSTANCES = [mlp_name(r, e) for r in (False, True) for e in (0, 1)] + [mlp_name(False, 0, True)]
ALL_INSTANCES = SG_INSTANCES + MLP_INSTANCES


# -------------------------------------------------------------------- shapes --
DS = (128, 256, 384)
AF_PAIRS = [(0.0, 1e-4), (1.0, 0.5), (1e-4, 1e-4), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (1e-4, 1.0), (0.3, 0.0)]


def act_rows(rows):
    return (1, 31, 33, rows - 1, rows, rows + 1, rows + 33, 3 * rows + 1)


def act_n(D):
    return (64, 128, 192, 320) + ((1152,) if D == 384 else ())


def periods(M, rows):
    return (1, 33, rows, M, M + 7)


def act_forms():
    """(D, act, rank, waves4) of every ACT instantiation at D <= 384."""
    out = [(D, a, r, False) for D in DS for a in ("none", "gelu") for r in (False, True)]
    return out + [(384, a, False, True) for a in ("none", "gelu")]


def act_cases(D, a, rank, waves4):
    """(M, N, period or None)."""
    rows = dispatch(D, "act", a, rank, waves4)[1]
    return [(M, N, p) for N in act_n(D) for M in act_rows(rows) for p in (periods(M, rows) if rank else (None,))]


K768_M = (1, 127, 128, 129, 385)
K768_N = (64, 192, 1536)


def cat_periods(M):
    return (1, 33, 128, M, M + 5)


LN_M = (1, 127, 128, 129, 257)


def ln_cases(D, rank):
    return [(M, p) for M in LN_M for p in (periods(M, ROWS4) if rank else (None,))]


def head_rows(D):
    return (1, 127, 128, 129, (4 * D // 64) * 128 + 1)


MLP_M = (1, 127, 128, 129, 24 * 128 + 1)


def mlp_cases(rank):
    return [(M, p) for M in MLP_M for p in (periods(M, ROWS4) if rank else (None,))]


def all_table_instances():
    """instantiation -> number of table cases that launch it."""
    out = {}

    def add(name, n):
        out[name] = out.get(name, 0) + n
    for D, a, r, w4 in act_forms():
        add(dispatch(D, "act", a, r, w4)[0], len(act_cases(D, a, r, w4)))
    for M in K768_M:
        for _ in K768_N:
            add(dispatch(768, "act", "gelu", False)[0], 1)
            add(dispatch(768, "act", "gelu", False, cat=True)[0], len(cat_periods(M)))
    for D in DS:
        for r in (False, True):
            add(dispatch(D, "ln", "lrelu", r)[0], len(ln_cases(D, r)))
        add(dispatch(D, "head2", "gelu", False)[0], 2 * len(head_rows(D)))
    for r in (False, True):
        for e in (0, 1):
            add(mlp_name(r, e), len(mlp_cases(r)))
    add(mlp_name(False, 0, True), len(MLP_M) + 2)
    return out


# -------------------------------------------------------------------- inputs --
def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * 1000003 ** i for i, s in enumerate(seed)) % (2 ** 63 - 1))
    return g


def _bf(t):
    """Round to bf16 and flush what would be a bf16 subnormal."""
    t = t.to(BF16)
    return torch.where(t.float().abs() < 2.0 ** -126, torch.zeros_like(t), t)


def _vecs(g, *n):
    """f32 vectors with bf16-exact values."""
    return [_bf(torch.randn(k, generator=g)).float() for k in n]


@functools.lru_cache(maxsize=None)
def base(D, N, Mmax):
    """x [Mmax, D], W [N, D], bias and rank columns of a (D, N): every M of the table is a row
    prefix.  Do not modify."""
    g = _gen(D, N, 1)
    c = SimpleNamespace(D=D, N=N, x=_bf(torch.randn(Mmax, D, generator=g)), w=_bf(torch.randn(N, D, generator=g) / math.sqrt(D)))
    c.x[0, ::7] = 0.0
    c.b, c.c1, c.c2 = _vecs(g, N, N, N)
    return c


@functools.lru_cache(maxsize=None)
def base_gemm(D, N, Mmax, dev="cpu"):
    c = base(D, N, Mmax)
    return gemm(c.x.to(dev), c.w.to(dev))


def rank_scalars(M, period, seed=0):
    """r1, r2 of exactly `period` elements in [0, 1), bf16-exact."""
    g = _gen(M, period, seed, 2)
    return _bf(torch.rand(period, generator=g)).float(), _bf(torch.rand(period, generator=g)).float()


def ln_vecs(D):
    g = _gen(D, 3)
    return _bf(torch.rand(D, generator=g) + 0.5).float(), _bf(torch.randn(D, generator=g)).float()


def low_variance_case(D, M):
    """W = 0 and a constant bias; x[m, :] = (8 + m % 9 + k) 2^-8, k in -3 .. 3: v = lrelu(b) + x has a
    row variance of about 4 2^-16 = 6e-5 around a mean of 2^-5, so eps = 1e-5 is a sixth of the
    denominator, eps x 10 halves rstd, and the one-pass E[v^2] - mean^2 loses nothing that matters."""
    g = _gen(D, M, 4)
    k = torch.randint(-3, 4, (M, D), generator=g)
    x = ((8 + torch.arange(M)[:, None] % 9 + k).float() * 2.0 ** -8).to(BF16)
    gm, be = ln_vecs(D)
    return SimpleNamespace(x=x, w=torch.zeros(D, D, dtype=BF16), b=torch.full((D,), -2.0 ** -4), g=gm, be=be)


def head_vecs(D, scale=1.0):
    N = 4 * D
    g = _gen(D, 5)
    w_out = _bf(torch.randn(2, N, generator=g) / math.sqrt(N) * scale).float()
    return w_out, _bf(torch.randn(2, generator=g)).float()


def sparse_w1(D=384, H=1536, nnz=8, seed=6):
    """Eight entries per row, +-1/4 or +-1/2, at distinct columns."""
    g = _gen(D, H, seed)
    w = torch.zeros(H, D)
    cols = torch.rand(H, D, generator=g).argsort(-1)[:, :nnz]
    vals = (torch.randint(0, 2, (H, nnz), generator=g) * 2 - 1).float() * (0.25 * (1 + torch.randint(0, 2, (H, nnz), generator=g)))
    w.scatter_(1, cols, vals)
    return w.to(BF16)


@functools.lru_cache(maxsize=None)
def mlp_base(Mmax=MLP_M[-1]):
    D, H = 384, 1536
    g = _gen(D, H, 7)
    c = SimpleNamespace(D=D, H=H, x=_bf(torch.randn(Mmax, D, generator=g)), w1=sparse_w1(D, H),
                        w2=_bf(torch.randn(D, H, generator=g) / math.sqrt(H)))
    c.b1, c.c1, c.c2 = _vecs(g, H, H, H)
    c.b2 = _bf(0.1 * torch.randn(D, generator=g)).float()
    c.g, c.be = ln_vecs(D)
    return c


@functools.lru_cache(maxsize=None)
def mlp_gemm(dev="cpu"):
    c = mlp_base()
    return gemm(c.x.to(dev), c.w1.to(dev))


def mlp_parts(c, epi2):
    p = dict(b1=c.b1, b2=c.b2)
    if epi2 == 1:
        p.update(g=c.g, be=c.be, eps=f32(EPS))
    return p


def afgate_weights(seed=8, conditioning=False):
    """The scale of test_mlp_afgate_vs_fp32_and_two_launch_path; conditioning: the joint encoder of
    test_af_gate_layernorm_conditioning, which nearly cancels at af = 0.3."""
    g = _gen(seed)
    D = 384
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    w = [rn(32, 2, sc=0.8), rn(32, sc=0.1), rn(D, 32, sc=0.25), rn(D, sc=0.1), rn(D, 2, sc=0.7), rn(D, sc=0.1),
         1 + rn(D, sc=0.1), rn(D, sc=0.1)]
    if conditioning:
        w[4][:, 1] = 0.0
        w[5] = -0.3 * w[4][:, 0] + 1e-3 * torch.randn(D, generator=g)
    return w


def afgate_inputs(M, kind="rand"):
    """af, af_p in [0, 1): 'rand' starts with AF_PAIRS; 'pairs' is AF_PAIRS alone; 'cond' puts af = 0.3
    on the even rows and af in [0.45, 1) on the odd ones."""
    g = _gen(M, 9)
    af, afp = torch.rand(M, generator=g), torch.rand(M, generator=g)
    if kind == "cond":
        af = 0.45 + 0.55 * af                               # the ordinary rows keep clear of the cancellation
        af[::2] = 0.3
    else:
        n = min(M, len(AF_PAIRS))
        af[:n] = torch.tensor([a for a, _ in AF_PAIRS])[:n]
        afp[:n] = torch.tensor([b for _, b in AF_PAIRS])[:n]
    return af, afp


AFG_EXTRA = (("pairs", len(AF_PAIRS)), ("cond", 130))


# ---------------------------------------------------------- exact-answer case --
def exact_case(D, M, N, rank_period=None):
    """W a signed selection matrix (row n: (-1)^(n / 3) at column (7 n + 3) % D), x[m, k] = ((131 m +
    17 k) % 401) - 200, integer bias in [-8, 8], c1, c2 in [-4, 4], r1, r2 in [0, 3]: |out| <= 232,
    every product and sum an integer below 256, exact in f32 and in bf16."""
    m, k, n = torch.arange(M)[:, None], torch.arange(D)[None, :], torch.arange(N)
    x = ((131 * m + 17 * k) % 401 - 200).to(F64)
    col = (7 * n + 3) % D
    sgn = (1 - 2 * ((n // 3) % 2)).to(F64)
    w = torch.zeros(N, D, dtype=F64)
    w[n, col] = sgn
    b = ((5 * n) % 17 - 8).to(F64)
    out = x[:, col] * sgn + b
    c = SimpleNamespace(x=x.to(BF16), w=w.to(BF16), b=b.float(), col=col, rank=None)
    if rank_period is not None:
        i = torch.arange(rank_period)
        r1, r2 = (i % 4).to(F64), ((i // 4 + 1) % 4).to(F64)
        c1, c2 = ((3 * n) % 9 - 4).to(F64), ((7 * n) % 9 - 4).to(F64)
        ri = torch.arange(M) % rank_period
        out = out + r1[ri, None] * c1 + r2[ri, None] * c2
        c.rank = (r1.float(), r2.float(), rank_period, c1.float(), c2.float())
    assert float(out.abs().max()) <= 256 and torch.equal(c.x.to(F64), x)
    c.out = out.to(BF16)
    assert torch.equal(c.out.to(F64), out)
    return c


def gelu_domain_input():
    """Every normal bf16 value with |x| <= 16, both signs, padded with zeros to whole rows of 128."""
    bits = torch.arange(0x0080, 0x4180 + 1, dtype=torch.int32)             # 2^-126 .. 16.0
    v = torch.cat([bits, bits + 0x8000]).to(torch.int16).view(BF16)
    assert float(v.float().abs().max()) == 16.0 and float(v.float().abs().min()) == 2.0 ** -126
    pad = (-v.numel()) % 128
    return torch.cat([v, torch.zeros(pad, dtype=BF16)]).view(-1, 128)
