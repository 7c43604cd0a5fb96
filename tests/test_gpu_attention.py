"""The attention kernels (csrc/attention.hip: attn32_dma in its six attn_variant forms and both Q
paths, attn_fwd_bf16, attn_fwd_f32; csrc/attention_train.hip: attn_bwd_dq / attn_bwd_dkv and the
dh = 32 ring kernels) on inputs whose answer is exact, at every tile edge, and on random inputs
against the fp64 references of tests/attn_refs.py within its derived elementwise bounds
(test_attn_refs_cpu.py proves the references, the bounds and the builders on the CPU).

Exact-answer inputs (attn_refs.py):
  uniform   Q = 0, V[k, d] = [k % dh == d]: round(out L) is the number of keys in class d; one
            missing or extra key anywhere changes it.  Backward twin: round(dV L) counts queries,
            dK == 0.  lse == log2(L).
  one-hot   query i matches key pi(i) alone (next score >= 30 log2 units lower): out == V[pi(i)] bit
            for bit; pi covers tile 0, both ends of every 64-key tile and key L - 1.  No-fallback
            flavour: the fixed shift holds (attention_fallbacks() == 0); fallback flavour: in every
            wave a score exceeds the tile-0 maximum by >= 200, the wave must take the exact path.
  dropout   the uniform case with p in {0.1, 0.5}: round(out L (1 - p)) is the number of kept keys
            of class d for that query by attn_helpers.keep_mask -- the mask's (q, k) indexing
            decoded pair by pair; the same for dV over queries.
Random inputs: |out - ref| <= ulp_bf16(ref) / 2 + u W + 2 delta_q W + 1e-5 (1 + |ref|), u = 2^-8,
W = sum_k P |v - ref|; gradients: ulp_bf16(ref) / 2 + u A + 1e-5 (1 + F) (attn_refs.py derives both, one bf16
rounding of P or dS on every path).  max err / bound is printed per case.

L_SWEEP = 1, 15..17, 31..33, 63..65, 96, 97, 127..129, 191..193, 255..257, 319..321, 383..385,
447..449, 512, 513, 577, 1030: nfull / ntile of the 4-slot ring from 0/1 to 9/10 and 16/17 --
L <= 64 one (ragged) tile; 65..255 the tail loop alone with 2, 3, 4 tiles (wait(min(2, ..)) taking
0, 1, 2); 256 / 257 the first trip of the unrolled loop (nfull = 4) without and with a tail; 320 /
321 variant 3's ring3 branch (nfull >= 5) and its hand-back block, 384..513 the hand-back followed
by 1..3 more tiles, 512 / 513 two trips of the plain loop, 577 nine full tiles + 1 key; tails of 1,
15, 16, 17, 31, 32, 33 and 63 keys (the 1 / 2 / 4 MFMA-group tail bodies); both sides of a 32-query
wave, of the 128-query workgroup and of variant 4's 256-query workgroup.  The backward rings loop
over ntile with the same conditions.

Every input is a prefix view of NaN-padded storage (an over-read past the tensor shows up as
NaN), every output lives in sentinel-filled storage with guard columns and one guard row that must
be unchanged afterwards; the kernels are called through the C ABI so that leading dimensions
differ from the widths."""
import math

import pytest
import torch

import attn_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -776.0                      # bf16-exact sentinel
PAD = 4096                         # NaN elements behind every input
BF16_MAX = 3.3895313892515355e38
NSEQ, H = 2, 2


def K():
    from src import kernels
    return kernels


def N():
    from src import native
    return native


# ------------------------------------------------------------- guarded calls --
def _in(t, ld=None, pad=PAD):
    """Device storage holding the 2-D ``t`` with row stride ``ld``: NaN in the gap columns and in
    ``pad`` elements behind the last row; pad = 0: the storage ends at the last element."""
    rows, cols = t.shape
    ld = ld or cols
    buf = torch.full((rows * ld + pad,), float("nan"), dtype=t.dtype)
    buf[:rows * ld].view(rows, ld)[:, :cols] = t
    return torch.cat([buf[:(rows - 1) * ld + cols], buf[rows * ld:]]).to(DEV)


def _outbuf(rows, ld, dtype):
    return torch.full(((rows + 1) * ld,), SENT, dtype=dtype, device=DEV)


def _take(buf, rows, cols, ld, what):
    v = buf.view(rows + 1, ld).cpu()
    res = v[:rows, :cols].clone()
    v[:rows, :cols] = SENT
    assert bool((v == SENT).all()), f"{what}: wrote outside its {rows} x {cols} block (ld {ld})"
    return res


def attn(x, nseq, L, Hh, dh, scale=None, ld_qkv=None, ld_out=None, pad=PAD):
    D, n = Hh * dh, N()
    ld_out = ld_out or D + 8
    xin, ob = _in(x, ld_qkv, pad), _outbuf(nseq * L, ld_out, x.dtype)
    n.check(n.lib().snvrag_attention(n.dtype_code(x.dtype), nseq, L, Hh, dh, n.ptr(xin), ld_qkv or 3 * D, n.ptr(ob),
                                     ld_out, dh ** -0.5 if scale is None else scale, n.stream_ptr()), "attention")
    torch.cuda.synchronize()
    return _take(ob, nseq * L, D, ld_out, "attention out")


def train_fwd(x, nseq, L, Hh, dh, p=0.0, seed=R.DROP_SEED, ld_qkv=None, ld_out=None, pad=PAD):
    D, n = Hh * dh, N()
    ld_out = ld_out or D + 8
    xin, ob = _in(x, ld_qkv, pad), _outbuf(nseq * L, ld_out, BF16)
    lb = torch.full((nseq * Hh * L + L,), SENT, dtype=F32, device=DEV)
    n.check(n.lib().snvrag_attention_train_fwd(nseq, L, Hh, dh, n.ptr(xin), ld_qkv or 3 * D, n.ptr(ob), ld_out,
                                               n.ptr(lb), dh ** -0.5, p, seed, n.stream_ptr()), "attention_train_fwd")
    torch.cuda.synchronize()
    lse = lb.cpu()
    assert bool((lse[nseq * Hh * L:] == SENT).all()), "lse: wrote past its end"
    return _take(ob, nseq * L, D, ld_out, "train out"), lse[:nseq * Hh * L].view(nseq, Hh, L).clone()


def bwd(x, dout, out, lse, nseq, L, Hh, dh, p=0.0, seed=R.DROP_SEED, ld_qkv=None, ld_out=None, ld_dout=None,
        ld_dqkv=None, pad=PAD):
    D, n = Hh * dh, N()
    ld_dqkv = ld_dqkv or 3 * D + 8
    xin, oin, gin = _in(x, ld_qkv, pad), _in(out.to(BF16), ld_out, pad), _in(dout, ld_dout, pad)
    lin = _in(lse.to(F32).reshape(1, -1), None, pad)
    ws = torch.full((nseq * Hh * L + 64,), float("nan"), dtype=F32, device=DEV)
    gb = _outbuf(nseq * L, ld_dqkv, BF16)
    n.check(n.lib().snvrag_attention_bwd(nseq, L, Hh, dh, n.ptr(xin), ld_qkv or 3 * D, n.ptr(oin), ld_out or D,
                                         n.ptr(gin), ld_dout or D, n.ptr(lin), n.ptr(ws), n.ptr(gb), ld_dqkv,
                                         dh ** -0.5, p, seed, n.stream_ptr()), "attention_bwd")
    torch.cuda.synchronize()
    g = _take(gb, nseq * L, 3 * D, ld_dqkv, "dqkv")
    return g[:, :D], g[:, D:2 * D], g[:, 2 * D:]


def _counts(cnt, rows, Hh):
    return cnt.repeat(Hh).expand(rows, cnt.numel() * Hh)


def _check(got, ref, bound, what):
    r = R.ratio(got, ref, bound)
    print(f"{what}: max err/bound {r:.3f}")
    assert r <= 1.0, what
    return r


# ------------------------------------------------ a. inference, dh = 32, bf16 --
def _dh32_paths():
    """(name, prescaled, attn_variant): the prescaled kernel in its six variants, then attn32_dma<false>."""
    return [(f"pre/v{v}", True, v) for v in range(6)] + [("unscaled", False, 0)]


def _dh32_params():
    return [pytest.param(L, name, pre, var, id=f"{L}-{name}") for L in R.L_SWEEP for name, pre, var in _dh32_paths()]


@pytest.mark.parametrize("L,name,pre,var", _dh32_params())
def test_inference_dh32_exact(L, name, pre, var):
    dh, rows = 32, NSEQ * L
    uq, cnt = R.uniform_case(L, H, dh, NSEQ)
    scale = R.PRESCALED if pre else None
    K().attention_fallbacks(True)
    with K().option("attn_variant", var):
        out = attn(uq, NSEQ, L, H, dh, scale)
        oq, expect, oscale, _ = R.onehot_case(L, H, dh, False, NSEQ, prescaled=pre)
        hot = attn(oq.to(BF16), NSEQ, L, H, dh, oscale)
    bad = (R.decode_counts(out, L) != _counts(cnt, rows, H)).any(1).nonzero().flatten().tolist()
    assert not bad, f"uniform: rows {bad[:8]} decode to {R.decode_counts(out, L)[bad[0]][:4].tolist()}, want {cnt[:4].tolist()}"
    assert torch.equal(hot.to(F64), expect), "one-hot"
    if pre and var:
        assert torch.equal(out, attn(uq, NSEQ, L, H, dh, scale)), f"variant {var} differs from variant 0"
    assert K().attention_fallbacks(True) == 0


@pytest.mark.parametrize("L", R.L_FALLBACK)
def test_inference_dh32_fallback_exact(L):
    dh = 32
    cases = {pre: R.onehot_case(L, H, dh, True, NSEQ, prescaled=pre) for pre in (True, False)}
    for name, pre, var in _dh32_paths():
        oq, expect, scale, _ = cases[pre]
        K().attention_fallbacks(True)
        with K().option("attn_variant", var):
            out = attn(oq.to(BF16), NSEQ, L, H, dh, scale)
        assert torch.equal(out.to(F64), expect), name
        assert K().attention_fallbacks(True) > 0, name


# ------------------------------------------------- b. generic and f32 kernels --
@pytest.mark.parametrize("L", R.L_GENERIC)
@pytest.mark.parametrize("dh,dt", [(16, BF16), (48, BF16), (64, BF16), (16, F32), (32, F32), (48, F32), (64, F32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_generic_and_f32_exact(dh, dt, L):
    rows = NSEQ * L
    uq, cnt = R.uniform_case(L, H, dh, NSEQ)
    out = attn(uq.to(dt), NSEQ, L, H, dh)
    assert torch.equal(R.decode_counts(out, L), _counts(cnt, rows, H)), "uniform"
    for over in ((False, True) if L > R.KT else (False,)):
        oq, expect, scale, _ = R.onehot_case(L, H, dh, over, NSEQ)
        out = attn(oq.to(dt), NSEQ, L, H, dh, scale)
        assert torch.equal(out.to(F64), expect), ("one-hot", over)


# ----------------------------------------------------- c. training forward --
TRAIN_SHAPES = [(32, L) for L in R.L_SWEEP] + [(64, L) for L in R.L_DH64]
LSE_F32 = 3.5 * 2.0 ** -23           # f32 rounding + the 3-ulp log2 of the device math library, per unit of |lse|


@pytest.mark.parametrize("dh,L", TRAIN_SHAPES)
def test_train_fwd_exact(dh, L):
    rows = NSEQ * L
    uq, cnt = R.uniform_case(L, H, dh, NSEQ)
    K().attention_fallbacks(True)
    out, lse = train_fwd(uq, NSEQ, L, H, dh)
    assert torch.equal(R.decode_counts(out, L), _counts(cnt, rows, H)), "uniform"
    assert float((lse.to(F64) - math.log2(L)).abs().max()) <= LSE_F32 * max(1.0, math.log2(L)), "uniform lse"
    for p in (0.1, 0.5):
        keep = R.keep_mask(NSEQ, H, L, p)
        out, lse = train_fwd(uq, NSEQ, L, H, dh, p)
        assert torch.equal(R.decode_counts(out, L * (1 - p)), R.kept_counts(keep, L, H, dh, "k")), ("dropout", p)
        assert float((lse.to(F64) - math.log2(L)).abs().max()) <= LSE_F32 * max(1.0, math.log2(L)), ("dropout lse", p)
    assert K().attention_fallbacks(True) == 0
    for over in ((False, True) if L > R.KT else (False,)):
        oq, expect, scale, _ = R.onehot_case(L, H, dh, over, NSEQ)
        out, lse = train_fwd(oq.to(BF16), NSEQ, L, H, dh)
        assert torch.equal(out.to(F64), expect), ("one-hot", over)
        rlse = R.ref_fwd(oq, NSEQ, L, H, dh)[1]
        _check(lse, rlse, 1e-5 * (1 + rlse.abs()), f"train fwd one-hot lse dh={dh} L={L} overshoot={over}")
        nf = K().attention_fallbacks(True)
        assert nf == 0 if not over or dh != 32 else nf > 0, (over, nf)


# -------------------------------- d. backward, isolated from the forward kernel --
@pytest.mark.parametrize("dh,L", TRAIN_SHAPES)
def test_bwd_isolated_exact(dh, L):
    """out (bf16) and lse (f32) come from ref_fwd, not from the forward kernel."""
    rows = NSEQ * L
    uq, cnt = R.uniform_case(L, H, dh, NSEQ)
    dout = R.uniform_dout(L, H, dh, NSEQ)
    for p in (0.0, 0.1, 0.5):
        keep = R.keep_mask(NSEQ, H, L, p)
        rout, rlse, _ = R.ref_fwd(uq, NSEQ, L, H, dh, None, keep, p)
        args = (uq, dout, rout.to(BF16), rlse.to(F32), NSEQ, L, H, dh)
        dq, dk, dv = bwd(*args, p=p)
        want = _counts(cnt, rows, H) if p == 0 else R.kept_counts(keep, L, H, dh, "q")
        assert torch.equal(R.decode_counts(dv, L * (1 - p)), want), ("dV counts", p)
        assert not dk.any(), ("dK must be 0", p)
        rq = R.ref_bwd(*args, None, keep, p)[0]
        ab = R.bwd_abs(*args, None, keep, p)
        _check(dq, rq, R.bwd_bound(rq, ab[0][0], ab[1][0]), f"bwd uniform dQ dh={dh} L={L} p={p}")


def _bwd_random(dh, L, p, chained=False):
    qkv, dout = R.random_qkv(NSEQ, L, H, dh, R.BWD_AMP, 3 * L + dh), R.random_dout(NSEQ, L, H, dh, L)
    keep = R.keep_mask(NSEQ, H, L, p)
    rout, rlse, P = R.ref_fwd(qkv, NSEQ, L, H, dh, None, keep, p)
    if not chained:
        args = (qkv, dout, rout.to(BF16), rlse.to(F32), NSEQ, L, H, dh)
        got = bwd(*args, p=p)
        refs, As = R.ref_bwd(*args, None, keep, p), R.bwd_abs(*args, None, keep, p)
        rs = [R.ratio(g, r, R.bwd_bound(r, a, f)) for g, r, a, f in zip(got, refs, *As)]
        print(f"bwd dh={dh} L={L} p={p}: max err/bound dQ {rs[0]:.3f} dK {rs[1]:.3f} dV {rs[2]:.3f}")
        assert max(rs) <= 1.0
        return rs
    # chained to the kernel's own forward, against the true gradient (fp64 out and lse): on top of the
    # isolated bound, (1) the forward's lse is off by up to e = lse_bound, which scales every P by
    # 2^+-e, i.e. adds e ln 2 A; (2) its out is off by up to fwd_bound, which moves D_q by up to
    # dD_q = sum_d |dO| fwd_bound and dS by P dD: scale sum_k P dD |K| on dQ, scale sum_q P dD |Q| on dK
    out, lse = train_fwd(qkv, NSEQ, L, H, dh, p)
    got = bwd(qkv, dout, out, lse, NSEQ, L, H, dh, p=p)
    args = (qkv, dout, rout, rlse, NSEQ, L, H, dh)
    refs, As = R.ref_bwd(*args, None, keep, p), R.bwd_abs(*args, None, keep, p)
    path = "train32" if dh == 32 else "generic"
    e = float(R.lse_bound(rlse, path).max()) * math.log(2.0)
    fb = R.fwd_bound(qkv, NSEQ, L, H, dh, None, keep, p, path=path)[1]
    dD = R.heads(dout.to(F64).abs() * fb, NSEQ, L, H, dh).sum(-1, keepdim=True)
    q, k, _ = R.split(qkv, NSEQ, L, H, dh)
    extra = (R.merge(dh ** -0.5 * ((P * dD) @ k.abs())), R.merge(dh ** -0.5 * ((P * dD).transpose(-1, -2) @ q.abs())), 0.0)
    rs = [R.ratio(g, r, R.bwd_bound(r, a, f) + e * a + x) for g, r, a, f, x in zip(got, refs, *As, extra)]
    print(f"bwd chained dh={dh} L={L} p={p}: max err/bound dQ {rs[0]:.3f} dK {rs[1]:.3f} dV {rs[2]:.3f}")
    assert max(rs) <= 1.0
    return rs


@pytest.mark.parametrize("dh,L,p", [(dh, L, 0.0) for dh, L in TRAIN_SHAPES] + [(dh, L, 0.1) for L, dh in R.BWD_DROP_SHAPES])
def test_bwd_isolated_random_vs_fp64(dh, L, p):
    _bwd_random(dh, L, p)


@pytest.mark.parametrize("L", [257, 1030])
def test_bwd_chained_to_forward_kernel(L):
    _bwd_random(32, L, 0.0, chained=True)
    _bwd_random(32, L, 0.1, chained=True)


# ---------------------------------------------- e. random forward vs fp64 --
@pytest.mark.parametrize("amp", R.RANDOM_AMPS)
@pytest.mark.parametrize("L", R.L_RANDOM)
@pytest.mark.parametrize("path", ["dma32_pre", "dma32", "train32"])
def test_fwd_random_vs_fp64(path, L, amp):
    dh, pre = 32, path == "dma32_pre"
    scale = R.PRESCALED if pre else dh ** -0.5
    qkv = R.random_qkv(NSEQ, L, H, dh, amp, L, prescaled=pre)
    ref, bound = R.fwd_bound(qkv, NSEQ, L, H, dh, scale, path=path)
    K().attention_fallbacks(True)
    if path == "train32":
        out, lse = train_fwd(qkv, NSEQ, L, H, dh)
        rlse = R.ref_fwd(qkv, NSEQ, L, H, dh)[1]
        _check(lse, rlse, R.lse_bound(rlse, path), f"fwd {path} lse L={L} amp={amp}")
    else:
        out = attn(qkv, NSEQ, L, H, dh, scale)
    _check(out, ref, bound, f"fwd {path} L={L} amp={amp}")
    assert K().attention_fallbacks(True) == 0


# ------------------------------------------------------------ f. isolation --
@pytest.mark.parametrize("seq", [1, 2])
@pytest.mark.parametrize("L", [65, 321, 1030])
def test_other_sequences_and_heads_do_not_leak(L, seq):
    """Every other sequence's and head's Q, K, V and dO overwritten with +-bf16-max: the block of
    (sequence ``seq``, head 1) must stay bit-identical and finite, in the forward kernels and in dQ,
    dK, dV.  seq = 1 has sequence 2 behind it, whose rows its tail tiles stage; seq = 2 is the last
    one, whose tail tiles reach past the tensor into the NaN padding every input here carries: that
    NaN must not reach any output.  NaN in *other sequences* is deliberately not asserted: the ring
    kernels stage whole 64-row tiles, so the tail tile of sequence s holds rows of sequence s + 1;
    their scores are masked but their V rows still meet P = 0 in the MFMA, the kernel documents
    finite data there, and masking V would cost VALU in the hot loop."""
    nseq, Hh, dh = 3, 3, 32
    D = Hh * dh
    qkv = R.random_qkv(nseq, L, Hh, dh, 1.0, L)
    dout = R.random_dout(nseq, L, Hh, dh, L)
    rout, rlse, _ = R.ref_fwd(qkv, nseq, L, Hh, dh)
    rout = rout.to(BF16)
    mine_r = torch.zeros(nseq * L, 1, dtype=torch.bool)
    mine_r[seq * L:(seq + 1) * L] = True
    mine_c = torch.zeros(1, D, dtype=torch.bool)
    mine_c[:, dh:2 * dh] = True
    mine = mine_r & mine_c
    g = torch.Generator().manual_seed(L)
    sign = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(BF16) * BF16_MAX
    qkv2 = torch.where(mine.repeat(1, 3), qkv, sign(qkv.shape))
    dout2 = torch.where(mine, dout, sign(dout.shape))
    rout2 = torch.where(mine, rout, sign(rout.shape))

    def runs(x, o, go):
        res = [attn(x, nseq, L, Hh, dh)]
        with K().option("attn_variant", 3):
            res.append(attn(x, nseq, L, Hh, dh, R.PRESCALED))
        res.append(train_fwd(x, nseq, L, Hh, dh)[0])
        res.append(train_fwd(x, nseq, L, Hh, dh, 0.1)[0])
        res += list(bwd(x, go, o, rlse, nseq, L, Hh, dh))
        res += list(bwd(x, go, o, rlse, nseq, L, Hh, dh, p=0.1))
        return [r[seq * L:(seq + 1) * L, dh:2 * dh] for r in res]

    for i, (a, b) in enumerate(zip(runs(qkv, rout, dout), runs(qkv2, rout2, dout2))):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), f"result {i} of (sequence {seq}, head 1) changed"


# ----------------------------------------------------- g. leading dimensions --
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("L", [65, 257])
def test_leading_dimensions(L, dh):
    """ld_qkv = 3 D + 8, ld_out = D + 8, ld_dout = D + 8, ld_dqkv = 3 D + 4 with NaN in the input
    gaps and the sentinel in the output gaps, against the contiguous call: bit-identical."""
    D = H * dh
    qkv, dout = R.random_qkv(NSEQ, L, H, dh, 1.0, L + dh), R.random_dout(NSEQ, L, H, dh, L)
    lds = dict(ld_qkv=3 * D + 8, ld_out=D + 8)
    pre = R.random_qkv(NSEQ, L, H, dh, 1.0, L + dh, prescaled=True)
    for x, scale in ((qkv, None), (pre, R.PRESCALED)):
        assert torch.equal(attn(x, NSEQ, L, H, dh, scale, **lds), attn(x, NSEQ, L, H, dh, scale, ld_out=D))
    f32 = qkv.to(F32)
    assert torch.equal(attn(f32, NSEQ, L, H, dh, **lds), attn(f32, NSEQ, L, H, dh, ld_out=D))
    for p in (0.0, 0.1):
        o1, l1 = train_fwd(qkv, NSEQ, L, H, dh, p, **lds)
        o0, l0 = train_fwd(qkv, NSEQ, L, H, dh, p, ld_out=D)
        assert torch.equal(o1, o0) and torch.equal(l1, l0), ("train fwd", p)
        g1 = bwd(qkv, dout, o0, l0, NSEQ, L, H, dh, p=p, ld_dout=D + 8, ld_dqkv=3 * D + 4, **lds)
        g0 = bwd(qkv, dout, o0, l0, NSEQ, L, H, dh, p=p, ld_dqkv=3 * D)
        for a, b, nm in zip(g1, g0, ("dQ", "dK", "dV")):
            assert torch.equal(a, b), (nm, p)


@pytest.mark.parametrize("L", [65, 1030])
def test_storage_ends_at_the_last_element(L):
    """qkv (and dout) with no padding at all: the ring kernels' buffer range ends with the tensor
    (total_rows), the rows a tail tile asks for beyond it come back as zeros."""
    dh = 32
    qkv, dout = R.random_qkv(NSEQ, L, H, dh, 1.0, L), R.random_dout(NSEQ, L, H, dh, L)
    pre = R.random_qkv(NSEQ, L, H, dh, 1.0, L, prescaled=True)
    for var in (0, 3, 4):
        with K().option("attn_variant", var):
            assert torch.equal(attn(pre, NSEQ, L, H, dh, R.PRESCALED, pad=0), attn(pre, NSEQ, L, H, dh, R.PRESCALED)), var
    assert torch.equal(attn(qkv, NSEQ, L, H, dh, pad=0), attn(qkv, NSEQ, L, H, dh))
    o1, l1 = train_fwd(qkv, NSEQ, L, H, dh, pad=0)
    o0, l0 = train_fwd(qkv, NSEQ, L, H, dh)
    assert torch.equal(o1, o0) and torch.equal(l1, l0)
    for a, b in zip(bwd(qkv, dout, o0, l0, NSEQ, L, H, dh, pad=0), bwd(qkv, dout, o0, l0, NSEQ, L, H, dh)):
        assert torch.equal(a, b)
