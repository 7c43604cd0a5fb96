"""float64 references, CPU emulations, elementwise bounds and exact-answer input builders for the
attention kernels (csrc/attention.hip, csrc/attention_train.hip).  CPU only (torch / numpy);
tests/test_attn_refs_cpu.py ties every piece down without a GPU, tests/test_gpu_attention.py runs
the kernels against it.

Layout everywhere: qkv [nseq * L, 3 D] = [Q | K | V], D = H * dh, head h in columns h * dh ..;
out / dout [nseq * L, D]; lse [nseq, H, L] in the log2 domain: lse_q = log2 sum_k exp2(c s_qk),
c = scale * log2(e), s = Q K^T.  ``keep`` is the bool mask of attn_helpers.keep_mask
[nseq, H, L(q), L(k)]; kept probabilities are scaled by 1 / (1 - p) (P~ = P o keep / (1 - p)).

ref_fwd / ref_bwd are the plain formulas in fp64.  ref_bwd takes ``out`` and ``lse`` as inputs, as
the kernels do, so D = sum_d dO O uses the bf16 ``out`` the kernel is given.

emu_fwd / emu_bwd evaluate the same formulas but round where the kernels round (f32r = to f32,
bf16r = to bf16, both round-to-nearest-even):

  forward, dh = 32 ring kernel attn32_dma (paths "dma32_pre", "dma32", "train32"):
    * "dma32" only: Q <- bf16r(Q * c) when loaded (attention.hip:507-510); "dma32_pre" takes Q as
      stored (the caller's scale is 1 / log2 e, c = 1); "train32" keeps Q unscaled and multiplies
      the shifted score by c in f32 (attention.hip:322);
    * the shift m_q is the exact maximum of the first 64 keys (a32::tile FIRST, :284-297);
    * P^ = bf16r(exp2(.)) (:322-324); the SAME P^ feeds the PV product and, through the ones-MFMA,
      the row sum (:359-363), so one bf16 rounding of P is on the path: n_p = 1;
    * dropout clears dropped P^ bit patterns (drop_pair_apply, :336-343: no second rounding) and
      scales O by the f32 1 / (1 - p) once (drop_scale_o, :369-375): still n_p = 1;
    * a wave (32 queries) in which any l or O is not finite recomputes with the exact online max
      (attn32_online, :392-455): P^ = bf16r(exp2(c s - max)) feeds the row sum, the PV operand is
      bf16r(p * keep / (1 - p)) (one rounding);
    * f32 accumulation, out = bf16r(O * (1 / l)) (:665-675), lse = c m + log2 l in f32 (:667).
  forward, generic bf16 kernel attn_fwd_bf16 (path "generic": dh 16 / 48 / 64 inference and the
  dh = 64 training forward), 64-key tiles with the online max:
    * p = exp2(c s - m) in f32 enters the row sum unrounded (:146-147, :156-157), the PV operand
      is bf16r(p) or bf16r(p * keep / (1 - p)) (:148, :158): n_p = 1;
    * f32 accumulation with the alpha rescale per tile, out = bf16r(O * (1 / l)) (:186-195).
  forward, "f32": attn_fwd_f32 in plain f32, f32 output.
  backward (attn_bwd_dq / attn_bwd_dkv and the dh = 32 ring kernels; the same element math):
    * P = exp2(c s - lse) in f32 from the lse it is given (attention_train.hip:192, :324, :489,
      :612); D_q = sum_d dO O in f32 from the bf16 ``out`` it is given (:129-135, :562-566) -- an
      input of ref_bwd as well, so it adds no rounding against that reference;
    * dQ: dS = bf16r(P (dP m - D)) (:196, :614), dQ = bf16r(scale * sum_k dS K) (:217, :654):
      one bf16 rounding on the path, n_r = 1;
    * dV: P~ = bf16r(P m) (:329, :492), dV = bf16r(sum_q P~ dO) (:354, :535): n_r = 1;
    * dK: dS = bf16r(P m dP - P D) (:330, :493), dK = bf16r(scale * sum_q dS Q) (:354, :535):
      n_r = 1;   (m = keep / (1 - p) in f32, 1 without dropout.)

Elementwise bounds (derived from those rounding points, calibrated against the emulation in
test_attn_refs_cpu.py, never against a kernel):
  forward, output (q, d) with W = sum_k P_qk |v~_qkd - ref_qd|, v~ = keep v / (1 - p) (= v
  without dropout):
      bound = ulp_bf16(ref) / 2 + n_p u W + 2 delta_q W + 1e-5 (1 + |ref|),   u = 2^-8
    - u is the unit roundoff of bf16: 8 significant bits, so the spacing at x in [2^e, 2^(e+1)) is
      2^(e-7) and a rounding moves x by at most 2^(e-8) <= 2^-8 |x|  (2^-9 |x| holds only at the
      top of a binade).
    - out = sum P^ v~ / sum P^ with P^ = P (1 + e_k), |e_k| <= u per bf16 rounding: to first
      order the error is sum_k P e_k (v~ - ref), at most n_p u W;
    - delta_q = u scale max_k sum_d |q_d k_d| bounds the change of a (natural-log) score from
      rounding Q * c to bf16 ("dma32" only, 0 elsewhere); every P moves by at most
      exp(+-delta) - 1 ~ delta, numerator and denominator both: 2 delta_q W;
    - 1e-5 (1 + |ref|) is the project's f32 bar (accumulation order, exp2, the reciprocal);
    - an f32 output ("f32") has no bf16 terms: 1e-5 (1 + W).
  backward, each of dQ, dK, dV:  bound = ulp_bf16(ref) / 2 + n_r u A + 1e-5 (1 + F), n_r = 1
  (above), A the reference's own sum with every term replaced by its absolute value:
      A_dQ = scale sum_k |dS| |K|,  A_dK = scale sum_q |dS| |Q|,  A_dV = sum_q P~ |dO|,
  and F the project's f32 bar on the same sum with dS opened up too (dS = P (dP m - D) is a
  difference of two f32 dot products, each of which carries its own f32 error however small their
  difference is -- at L = 1 the difference is exactly 0 and u A with it):
      |dS| -> P (sum_d |dO| |V| m + sum_d |dO| |O|);   F_dV = A_dV.

Builders (each asserts its preconditions in fp64 on the final, exactly representable values):
onehot_case, uniform_case (+ uniform_dout, the backward twin) and dropout counts; see there."""
import math

import numpy as np
import torch

import attn_helpers as AH

F64 = torch.float64
LOG2E = math.log2(math.e)
PRESCALED = 1.0 / LOG2E                  # the scale that declares Q pre-scaled by log2(e) / sqrt(dh)
KT = 64                                  # keys per tile, every kernel
U_BF16 = 2.0 ** -8                       # unit roundoff of bf16 (8 significant bits)
DROP_SEED = 0x1234_5678_9ABC_DEF1        # both seed halves in use

# every nfull / ntile from 0/1 to 9/10 on both sides of the ring's loop conditions; both sides of a
# 32-query wave, the 128-query workgroup and the 256-query workgroup of variant 4
L_SWEEP = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321,
           383, 384, 385, 447, 448, 449, 512, 513, 577, 1030)
L_DH64 = (1, 64, 65, 129, 257)
L_GENERIC = (1, 63, 64, 65, 129, 257)
L_RANDOM = (77, 257, 321, 1030)
L_FALLBACK = (65, 257, 321, 1030)
RANDOM_AMPS = (1.5, 0.25)                # randn * 1.5: peaky rows; * 0.25: near-uniform rows, where one key is visible
BWD_AMP = 1.0                            # the random backward inputs
BWD_DROP_SHAPES = ((65, 32), (257, 32), (1030, 32), (129, 64))   # (L, dh) of the random backward with p = 0.1


def f32r(x):
    return x.to(torch.float32).to(F64)


def bf16r(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def bf16_ulp(x):
    """Spacing of bf16 (8 significant bits) at |x|."""
    ax = torch.as_tensor(x, dtype=F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def _f32(x) -> float:
    return float(np.float32(x))


def split(qkv, nseq, L, H, dh):
    """q, k, v [nseq, H, L, dh] in fp64."""
    x = qkv.detach().cpu().to(F64).reshape(nseq, L, 3, H, dh)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    return q, k, v


def heads(x, nseq, L, H, dh):
    return x.detach().cpu().to(F64).reshape(nseq, L, H, dh).permute(0, 2, 1, 3)


def merge(x):
    n, H, L, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * L, H * dh)


def _mult(keep, p_drop, rounded=False):
    """keep / (1 - p) in fp64 (``rounded``: the kernels' f32 1.0f / (1.0f - p)); 1.0 without a mask."""
    if keep is None:
        return 1.0
    inv = _f32(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop))) if rounded else 1.0 / (1.0 - _f32(p_drop))
    return torch.as_tensor(np.asarray(keep)).to(F64) * inv


def keep_mask(nseq, H, L, p_drop, seed=DROP_SEED):
    return AH.keep_mask(seed, nseq, H, L, p_drop) if p_drop > 0 else None


# ------------------------------------------------------------------ references --
def ref_fwd(qkv, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0):
    """(out [nseq L, D], lse [nseq, H, L] (log2), P [nseq, H, L, L]) in fp64."""
    scale = dh ** -0.5 if scale is None else scale
    q, k, v = split(qkv, nseq, L, H, dh)
    s = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    m = s.amax(-1, keepdim=True)
    lse = m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))
    P = torch.exp2(s - lse)
    return merge((P * _mult(keep, p_drop)) @ v), lse.squeeze(-1), P


def _bwd_terms(qkv, dout, out, lse, nseq, L, H, dh, scale, keep, p_drop):
    scale = dh ** -0.5 if scale is None else scale
    q, k, v = split(qkv, nseq, L, H, dh)
    g, o = heads(dout, nseq, L, H, dh), heads(out, nseq, L, H, dh)
    P = torch.exp2((q @ k.transpose(-1, -2)) * (scale * LOG2E) - lse.detach().cpu().to(F64)[..., None])
    mk = _mult(keep, p_drop)
    Dq = (g * o).sum(-1, keepdim=True)
    dS = P * ((g @ v.transpose(-1, -2)) * mk - Dq)
    return scale, q, k, g, P * mk, dS


def ref_bwd(qkv, dout, out, lse, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0):
    """(dQ, dK, dV), each [nseq L, D] fp64: dV = P~^T dO, dS = P o (dO V^T o keep / (1 - p) - D),
    D = sum_d dO O, dQ = scale dS K, dK = scale dS^T Q, with P = exp2(c Q K^T - lse)."""
    scale, q, k, g, Pm, dS = _bwd_terms(qkv, dout, out, lse, nseq, L, H, dh, scale, keep, p_drop)
    return merge(scale * (dS @ k)), merge(scale * (dS.transpose(-1, -2) @ q)), merge(Pm.transpose(-1, -2) @ g)


def bwd_abs(qkv, dout, out, lse, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0):
    """((A_dQ, A_dK, A_dV), (F_dQ, F_dK, F_dV)): ref_bwd's sums with every term replaced by its
    absolute value -- A with |dS| as one term, F with dS itself opened up as well,
    |dS| -> P (sum_d |dO| |V| keep / (1 - p) + sum_d |dO| |O|), the quantity the f32 bar applies to."""
    scale, q, k, g, Pm, dS = _bwd_terms(qkv, dout, out, lse, nseq, L, H, dh, scale, keep, p_drop)
    _, _, v = split(qkv, nseq, L, H, dh)
    o = heads(out, nseq, L, H, dh)
    a = dS.abs()
    P = torch.exp2((q @ k.transpose(-1, -2)) * (scale * LOG2E) - lse.detach().cpu().to(F64)[..., None])
    f = P * ((g.abs() @ v.abs().transpose(-1, -2)) * _mult(keep, p_drop) + (g.abs() * o.abs()).sum(-1, keepdim=True))
    dv = merge(Pm.transpose(-1, -2) @ g.abs())
    return ((merge(scale * (a @ k.abs())), merge(scale * (a.transpose(-1, -2) @ q.abs())), dv),
            (merge(scale * (f @ k.abs())), merge(scale * (f.transpose(-1, -2) @ q.abs())), dv))


# ---------------------------------------------------------------------- bounds --
def fwd_bound(qkv, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0, path="dma32_pre", n_p=1):
    """(ref out, elementwise bound) of the module docstring for a forward ``path``."""
    scale = dh ** -0.5 if scale is None else scale
    ref, _, P = ref_fwd(qkv, nseq, L, H, dh, scale, keep, p_drop)
    q, k, v = split(qkv, nseq, L, H, dh)
    r = heads(ref, nseq, L, H, dh)
    mk = _mult(keep, p_drop)
    W = torch.empty_like(r)
    for d in range(dh):                                  # sum_k P_qk |v~_qkd - ref_qd|
        W[..., d] = (P * (mk * v[..., None, :, d] - r[..., :, None, d]).abs()).sum(-1)
    W = merge(W)
    if path == "f32":
        return ref, 1e-5 * (1 + W)
    delta = 0.0
    if path == "dma32":
        delta = merge((U_BF16 * scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)).expand_as(r))
    return ref, bf16_ulp(ref) / 2 + n_p * U_BF16 * W + 2 * delta * W + 1e-5 * (1 + ref.abs())


def lse_bound(ref_lse, path):
    """The f32 bar 1e-5 (1 + |ref|); the dh = 32 ring kernel sums the bf16-rounded P^ (its row sum is
    a ones-MFMA over the PV operand), l^ = l (1 + e), |e| <= u, which moves log2 l by up to u log2(e)
    more.  (Where every P^ is exact -- the uniform case -- the f32 bar alone holds.)"""
    return 1e-5 * (1 + ref_lse.abs()) + (U_BF16 * LOG2E if path in ("dma32_pre", "dma32", "train32") else 0.0)


def bwd_bound(ref, A, F, n_r=1):
    return bf16_ulp(ref) / 2 + n_r * U_BF16 * A + 1e-5 * (1 + F)


def ratio(got, ref, bound):
    """max |got - ref| / bound; NaN anywhere gives inf."""
    d = (got.detach().cpu().to(F64) - ref).abs()
    r = torch.where(d > 0, d / bound, torch.zeros_like(d))
    return float("inf") if torch.isnan(d).any() else float(r.max())


# ------------------------------------------------------------------ emulations --
FWD_PATHS = ("dma32_pre", "dma32", "train32", "generic", "f32")


def emu_fwd(qkv, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0, path="dma32_pre"):
    """(out, lse, number of 32-query waves that fell back) with the roundings of the module
    docstring; out holds bf16 values (f32 values for path "f32") in fp64."""
    scale = dh ** -0.5 if scale is None else scale
    q, k, v = split(qkv, nseq, L, H, dh)
    c = _f32(_f32(scale) * _f32(1.4426950408889634))
    kb = None if keep is None else torch.as_tensor(np.asarray(keep)).to(F64)
    dm = _mult(keep, p_drop, rounded=True)
    inv = _mult(np.ones(1), p_drop, rounded=True).item() if keep is not None else 1.0
    if path == "f32":
        q32, k32, v32 = (t.to(torch.float32) for t in (q, k, v))
        s = (q32 * np.float32(scale)) @ k32.transpose(-1, -2)
        return merge((torch.softmax(s, -1) @ v32).to(F64)), None, 0
    if path == "generic":
        sc = f32r(f32r(q @ k.transpose(-1, -2)) * c)
        m_run = torch.full(sc.shape[:-1] + (1,), -math.inf, dtype=F64)
        l = torch.zeros_like(m_run)
        o = torch.zeros_like(q)
        for t0 in range(0, L, KT):
            st = sc[..., t0:t0 + KT]
            m_new = torch.maximum(m_run, st.amax(-1, keepdim=True))
            alpha = f32r(torch.exp2(m_run - m_new))
            p = f32r(torch.exp2(st - m_new))
            pb = bf16r(p if keep is None else f32r(p * dm[..., t0:t0 + KT]))
            l = f32r(l * alpha + p.sum(-1, keepdim=True))
            o = f32r(o * alpha + pb @ v[..., t0:t0 + KT, :])
            m_run = m_new
        out = bf16r(f32r(o * f32r(1.0 / l)))
        return merge(out), f32r(m_run + torch.log2(l)).squeeze(-1), 0
    assert dh == 32 and path in ("dma32_pre", "dma32", "train32"), path
    cs = 1.0
    if path == "dma32":
        q = bf16r(f32r(q * c))
    elif path == "train32":
        cs = c
    else:
        assert abs(c - 1.0) < 1e-6, "the prescaled path needs scale = 1 / log2(e)"
    s = f32r(q @ k.transpose(-1, -2))
    m = s[..., :KT].amax(-1, keepdim=True)
    p = bf16r(torch.exp2(f32r(cs * f32r(s - m))))
    l = p.sum(-1, keepdim=True)
    pd = p if kb is None else torch.where(kb > 0, p, torch.zeros_like(p))
    o = f32r(f32r(pd @ v) * inv)
    bad = ~((l > 0) & (l < math.inf)) | ~torch.isfinite(o).all(-1, keepdim=True)
    nw = (L + 31) // 32
    badw = torch.zeros(nseq, H, nw * 32, 1, dtype=torch.bool)
    badw[:, :, :L] = bad
    badw = badw.view(nseq, H, nw, 32).any(-1)
    nfall = int(badw.sum())
    lse = f32r(cs * m + torch.log2(l))
    if nfall:
        rows = badw[..., None].expand(nseq, H, nw, 32).reshape(nseq, H, nw * 32)[:, :, :L, None]
        sc = f32r(cs * s)
        mn = sc.amax(-1, keepdim=True)
        pf = f32r(torch.exp2(sc - mn))
        pr = bf16r(pf)
        l2 = pr.sum(-1, keepdim=True)
        o2 = f32r((pr if kb is None else bf16r(f32r(pf * dm))) @ v)
        l, o = torch.where(rows, l2, l), torch.where(rows, o2, o)
        lse = torch.where(rows, f32r(mn + torch.log2(l2)), lse)
    out = bf16r(f32r(o * f32r(1.0 / l)))
    return merge(out), lse.squeeze(-1), nfall


def emu_bwd(qkv, dout, out, lse, nseq, L, H, dh, scale=None, keep=None, p_drop=0.0):
    """(dQ, dK, dV) bf16 values in fp64 with the roundings of the module docstring."""
    scale = dh ** -0.5 if scale is None else scale
    q, k, v = split(qkv, nseq, L, H, dh)
    g, o = heads(dout, nseq, L, H, dh), heads(out, nseq, L, H, dh)
    sf = _f32(scale)
    c = _f32(sf * _f32(1.4426950408889634))
    mk = _mult(keep, p_drop, rounded=True)
    p = f32r(torch.exp2(f32r(f32r(q @ k.transpose(-1, -2)) * c - f32r(lse.detach().cpu().to(F64))[..., None])))
    dp = f32r(g @ v.transpose(-1, -2))
    Dq = f32r((g * o).sum(-1, keepdim=True))
    ds_q = bf16r(p * f32r(dp * mk - Dq))                               # the dQ kernel's dS
    pm = f32r(p * mk)
    ds_k = bf16r(f32r(pm * dp - p * Dq))                               # the dK / dV kernel's dS
    dQ = bf16r(f32r(ds_q @ k) * sf)
    dK = bf16r(f32r(ds_k.transpose(-1, -2) @ q) * sf)
    dV = bf16r(f32r(bf16r(pm).transpose(-1, -2) @ g))
    return merge(dQ), merge(dK), merge(dV)


# -------------------------------------------------------------------- builders --
def random_qkv(nseq, L, H, dh, amp, seed, prescaled=False):
    """bf16 qkv of randn * amp; ``prescaled``: Q carries log2(e) / sqrt(dh) (use scale PRESCALED)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(nseq * L, 3 * H * dh, generator=g) * amp
    if prescaled:
        x[:, :H * dh] *= LOG2E / math.sqrt(dh)
    return x.to(torch.bfloat16)


def random_dout(nseq, L, H, dh, seed):
    g = torch.Generator(device="cpu").manual_seed(seed + 7919)
    return torch.randn(nseq * L, H * dh, generator=g).to(torch.bfloat16)


def _codes(n, count, seed):
    """``count`` distinct words of the length-n extended Hamming code {x: even weight, xor of the set
    positions = 0} (minimum distance 4) as a 0/1 array [count, n]: the zero word first, then the
    weight-4 words, then weight-6 words.  Every word is at distance 4 or 6 from the zero word."""
    rng = np.random.default_rng(seed)
    words = [()]
    w4 = [(a, b, c, a ^ b ^ c) for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n)
          if c < a ^ b ^ c < n]
    words += [w4[i] for i in rng.permutation(len(w4))]
    seen = set(words)
    while len(words) < count:
        five = rng.choice(n, 5, replace=False)
        sixth = int(np.bitwise_xor.reduce(five))
        w = tuple(sorted(set(int(x) for x in five) | {sixth}))
        if len(w) == 6 and sixth < n and w not in seen:
            seen.add(w)
            words.append(w)
    out = np.zeros((count, n), np.int64)
    for i, w in enumerate(words[:count]):
        out[i, list(w)] = 1
    return out


def onehot_pi(L, overshoot=False):
    """pi [L]: query i attends key pi(i).  The first queries cover all of tile 0, the first and the
    last key of every 64-key tile and key L - 1; the others walk the keys with stride 37.  With
    ``overshoot`` every 32-query wave gets a query whose key lies outside tile 0 (queries 32 w + 1
    of the waves that have none are redirected to key L - 1, at the price of their own key)."""
    cover = sorted(set(range(min(KT, L))) | {t for t in range(0, L, KT)} | {min(t + KT, L) - 1 for t in range(0, L, KT)}
                   | {L - 1})
    pi = np.array([cover[i] if i < len(cover) else (37 * i + 11) % L for i in range(L)])
    if overshoot:
        assert L > KT, "one tile: the shift is the exact maximum, nothing can overshoot"
        for w0 in range(0, L, 32):
            if not (pi[w0:w0 + 32] >= KT).any():
                pi[min(w0 + 1, L - 1)] = L - 1
    else:
        assert set(cover) <= set(pi.tolist())
    return pi


ONEHOT_AB = {16: (4.0, 4.0), 32: (4.0, 6.0), 48: (4.0, 8.0), 64: (4.0, 8.0)}    # key / query amplitudes
OVERSHOOT_B = 5.0                                                                 # query amplitude factor


def onehot_case(L, H, dh, overshoot=False, nseq=2, prescaled=False, seed=0):
    """Keys are a times distinct sign codes (minimum Hamming distance 4, key 0 the all-plus word, so
    every score is within 6 sign flips of a tile-0 score), query i is b times the code of key
    pi(i), V rows are distinct bf16-exact values in +-[1, 2) that also differ between sequences and
    heads; each (sequence, head) flips its own random subset of the dh coordinates in Q and K
    alike.  ``prescaled``: Q holds bf16(b log2(e) / sqrt(dh)) and the scale is 1 / log2(e).
    ``overshoot`` (the fallback flavour): queries whose key lies outside tile 0 are 5 times larger.

    Returns (qkv fp64 of bf16-exact values, expected out = V[pi] [nseq L, D] fp64, scale, pi).
    Asserted here, in log2 units (what the kernel's exp2 sees), on the returned values:
      * the winning score beats the runner-up by >= 30 (every query);
      * no overshoot: no score exceeds the row's tile-0 maximum by more than 100;
      * overshoot: in every 32-query wave some query exceeds it by >= 200;
      * the softmax output rounds to V[pi] exactly in bf16, and in f32 when the winner has weight 1
        in f32 (sum_k!=pi P_qk |v_k - v_pi| < 2^-26)."""
    a, b = ONEHOT_AB[dh]
    c = LOG2E / math.sqrt(dh)
    scale = PRESCALED if prescaled else 1.0 / math.sqrt(dh)
    b_big = b * OVERSHOOT_B
    if prescaled:
        b, b_big = (float(torch.tensor(x * c).to(torch.bfloat16)) for x in (b, b_big))
    pi = onehot_pi(L, overshoot)
    sign = torch.from_numpy(1 - 2 * _codes(dh, L, seed + 1000 * dh)).to(F64)               # [L, dh]
    rng = np.random.default_rng(seed + 1)
    flip = torch.from_numpy(1 - 2 * rng.integers(0, 2, (nseq, H, 1, dh))).to(F64)
    bq = torch.full((L, 1), b, dtype=F64)
    if overshoot:
        bq[torch.from_numpy(pi >= KT)] = b_big
    kk = torch.arange(L)[:, None]
    dd = torch.arange(dh)[None, :]
    v = torch.empty(nseq, H, L, dh, dtype=F64)
    for s in range(nseq):
        for h in range(H):
            mant = torch.where(dd % 2 == 0, kk + 3 * dd, 11 * (kk // 128) + kk + 5 * dd) + 29 * h + 61 * s
            v[s, h] = (1 + (mant % 128).to(F64) / 128) * (1 - 2 * ((kk + dd) % 2)).to(F64)
            assert len({tuple(r) for r in v[s, h].tolist()}) == L, "V rows must be distinct"
    q = (bq * sign[pi])[None, None] * flip
    k = (a * sign)[None, None] * flip
    qkv = torch.cat([merge(q), merge(k), merge(v)], 1)
    assert torch.equal(bf16r(qkv), qkv), "values must be bf16-exact"
    expect = merge(v[:, :, pi])
    # preconditions, fp64, on the final values
    s2 = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    win = s2.gather(-1, torch.from_numpy(pi).expand(nseq, H, L)[..., None])
    rest = s2.scatter(-1, torch.from_numpy(pi).expand(nseq, H, L)[..., None], -math.inf)
    assert rest.shape[-1] == 1 or float((win - rest.amax(-1, keepdim=True)).min()) >= 30.0, "gap below 30"
    over = (s2.amax(-1) - s2[..., :KT].amax(-1))                                          # [nseq, H, L]
    if overshoot:
        pad = torch.full((nseq, H, (-L) % 32), -math.inf, dtype=F64)
        assert bool((torch.cat([over, pad], -1).view(nseq, H, -1, 32).amax(-1) >= 200.0).all()), "no overshoot in a wave"
    else:
        assert float(over.max()) <= 100.0, "a score overshoots the tile-0 maximum by more than 100"
    ref, _, P = ref_fwd(qkv, nseq, L, H, dh, scale)
    assert torch.equal(bf16r(ref), expect), "the exact softmax does not round to V[pi]"
    dev = torch.stack([(P * (v[..., None, :, d] - v[:, :, pi][..., :, None, d]).abs()).sum(-1) for d in range(dh)], -1)
    assert float(dev.max()) < 2.0 ** -26, "the runners-up are visible in f32"
    return qkv, expect, scale, pi


def class_counts(L, dh):
    """counts[d] = number of r < L with r % dh == d."""
    return torch.bincount(torch.arange(L) % dh, minlength=dh).to(F64)


def uniform_case(L, H, dh, nseq=2, seed=0):
    """Q = 0, K random, V[k, d] = 1 if k % dh == d else 0: P = 1 / L exactly and out[q, d] L is the
    number of keys in residue class d (<= ceil(L / dh) <= 65 for L <= 1030, dh >= 16).  Adjacent
    counts differ by >= 1 / 65 relative, far above the 2^-8 of the bf16 roundings on the way, so
    round(out L) must equal the count: one missing or extra key anywhere fails.
    Returns (qkv bf16, counts [dh] fp64)."""
    qkv = random_qkv(nseq, L, H, dh, 1.5, seed + 31 * L + dh).to(F64).view(nseq * L, 3, H, dh)
    qkv[:, 0] = 0
    qkv[:, 2] = (torch.arange(L).repeat(nseq)[:, None, None] % dh == torch.arange(dh)[None, None, :]).to(F64)
    cnt = class_counts(L, dh)
    assert float(cnt.max()) <= 65 and 65 * 2.0 ** -7 < 1.0       # the decode margin: 65 (1 + 2^-7) rounds to 65
    return qkv.view(nseq * L, 3 * H * dh).to(torch.bfloat16), cnt


def uniform_dout(L, H, dh, nseq=2):
    """The backward twin: dout[q, d] = 1 if q % dh == d.  dV[k, d] L is the number of queries in class
    d and dK is exactly 0 (Q = 0)."""
    one = (torch.arange(L).repeat(nseq)[:, None, None] % dh == torch.arange(dh)[None, None, :])
    return one.expand(nseq * L, H, dh).reshape(nseq * L, H * dh).to(torch.bfloat16)


def kept_counts(keep, L, H, dh, over="k"):
    """dropout_count_case: counts of kept pairs per residue class as [nseq L, D] fp64.
    over="k": row q, column (h, d) = #{k: keep[q, k], k % dh == d}   (the forward's out L (1 - p));
    over="q": row k, column (h, d) = #{q: keep[q, k], q % dh == d}   (the backward's dV L (1 - p))."""
    kp = torch.as_tensor(np.asarray(keep)).to(F64)                    # [nseq, H, L(q), L(k)]
    cls = (torch.arange(L)[:, None] % dh == torch.arange(dh)[None, :]).to(F64)  # [L, dh]
    return merge(kp @ cls if over == "k" else kp.transpose(-1, -2) @ cls)


def decode_counts(x, factor):
    """round(x * factor) of a kernel or emulation output."""
    return torch.round(x.detach().cpu().to(F64) * factor)
