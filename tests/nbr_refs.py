"""Plain numpy restatements of the neighbour-mean family (csrc/knn.hip: rag_mean_kernel<float |
bf16, CNT, BITS>, neighbor_counts_kernel<BITS>; csrc/train.hip: nbr_mean_drop_fwd_kernel,
nbr_mean_drop_bwd_kernel<DET>) for the kernel-level tests, with the per-element bounds and the
shape tables those tests sweep.  Everything runs on the CPU.  Every function takes ``dtype``:
float64 is the reference, float32 an emulation that rounds where the kernel rounds, in the kernel's
order (test_nbr_refs_cpu.py holds it to the bounds and plants faults in it through ``fault``).

The operations, in the kernels' order (ids = tok0, tok1, sos, eos, pad; position l of a window of
n_sites sites is <sos> at 0, site l - 1 at 1..n_sites, <eos> at n_sites + 1, <pad> after it):

  rag_mean      nv_q = #{j: idx[q, j] >= 0},  c[q, s] = sum over those j of the panel's allele at
                (idx[q, j], s) (u8 rows, bit-packed rows, or the ready-made counts[q, s])
                f = c / nv                                     one f32 divide
                dw = W[tok1] - W[tok0]                         one f32 subtract
                site:      x = W[tok0] + f dw                  product, add (0 when nv = 0)
                non-site:  x = W[sos | eos | pad]
                out = x + pe[l] (+ Ar[l])                      one add each; Ar may be absent
                bf16 outputs round out once more.
  counts        counts[q, s] = #{j: row0 <= idx[q, j] < row0 + n_rows, allele 1 at s}, exact, 0 in
                the columns from ld to ld_out.
  nbr forward   keep = attn_helpers.ln_keep_mask(seed, 7, U, L D, p).reshape(U, L, D), sc = f32(1 /
                (1 - p)) (1 at p = 0), m = keep sc
                c = pe[l] + Ar[l];  t_j = W[tok(u_j, l)] + c;  s = fma(m_j, t_j, s) over the valid j
                out = s * f32(1 / max(nv, 1))                  a query with no neighbour gives 0
                tok(u, l) = tok0 + code[u, l - 1] at a site: tok1 is tok0 + 1 here.
  nbr backward  per (l, d) one thread: g = dout[q, l, d] / nv_q, e = g m, then serial sums over (q, j)
                in index order into dAr[l, d] and into the position's token rows (tok0 / tok0 + 1 by
                the neighbour's code, or sos / eos; <pad> gets nothing).  The thread's sums go into
                the block's [V, D] partial; the L block partials are added to dW by atomics in
                arbitrary order, or (deterministic) by colsum_f32_kernel in a fixed one.  dW and
                dAr are accumulated into.

Bounds, per element, u = 2^-24, gamma(n) = n u / (1 - n u) (n roundings in sequence, each relative
to a partial result that is at most A, the sum of the magnitudes of the element's terms):

  rag_mean      site      gamma(RAG_SITE = 6) A, A = |W[tok0]| + f (|W[tok0]| + |W[tok1]|) + |pe| + |Ar|:
                          divide, subtract, product, three adds (A = |pe| + |Ar| when nv = 0)
                non-site  gamma(RAG_PLAIN = 2) (|W[t]| + |pe| + |Ar|): two adds
                bf16      + ulp_bf16(ref) / 2
  nbr forward   gamma(nv + FWD_C = nv + 4) A, A = (1 / nv) sum_j m_j (|W| + |pe| + |Ar|): the pe + Ar
                add, the W + c add, one fma rounding per neighbour, f32(1 / nv), the final product.
                An element dropped under every neighbour has A = 0 and must be exactly 0.
  nbr backward  dAr  gamma(nq k + BWD_AR_C = nq k + 3) (sum |e| + |prior|): T = nq k serial adds, the
                     divide, the product with m, the add onto the prior
                dW   gamma(nq k + L + BWD_W_C = nq k + L + 4) (sum |e| + |prior|): as dAr, plus the add
                     into the block partial and the up to L partials onto the prior.  Any order of
                     L + 1 addends has at most L roundings on any path, so the bound holds for
                     every atomic order and for the fixed one.
                Rows that no position holds (<pad> among them) have A = |prior| and ref = prior:
                gamma(n) |prior| would allow a change, so their bound is set to 0: bit for bit the prior.

The bounds are never measured against a kernel.

Exact tables (kind "exact": bound 0, bit for bit): W, pe, Ar, dout and the priors are small
integers, every nv a power of two, p = 0.5 under dropout (sc = 2, thresh = 32768).  rag_mean:
W[tok1] - W[tok0] is a multiple of 128 >= nv, so f dw is an integer and |out| <= 60 + 128 + 30 +
30 = 248 <= 256, exact in bf16.  nbr: every partial sum is a multiple of 1 / 8 below 2^20."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from attn_helpers import ln_keep_mask

F64, F32 = np.float64, np.float32
U = 2.0 ** -24
SEED = 0x5EED0123456789AB
NBR_STREAM = 7                     # drop_base(seed, 7)

# roundings per output, named in the docstring
RAG_SITE, RAG_PLAIN = 6, 2
FWD_C = 4
BWD_AR_C, BWD_W_C = 3, 4

IDS = dict(tok0=5, tok1=6, sos=2, eos=3, pad=0)          # the model's
IDS_ALT = dict(tok0=4, tok1=7, sos=1, eos=8, pad=9)      # tok1 != tok0 + 1, pad != 0
IDS_NBR_ALT = dict(tok0=3, tok1=4, sos=7, eos=1, pad=5)  # the training kernels fix tok1 = tok0 + 1
VOCAB = 10

RAG_FAULTS = ("tok_swap", "drop_last", "eos_late", "nv_counts_invalid", "units_past_256")
FWD_FAULTS = ("tok_swap", "drop_last", "eos_late", "hash_half", "nv_counts_invalid")
BWD_FAULTS = FWD_FAULTS + ("pad_grad",)


def gamma(n):
    n = np.asarray(n, F64)
    return n * U / (1.0 - n * U)


def drop_scale(p) -> float:
    """make_attn_drop's f32 1 / (1 - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def bf16_ulp(ref):
    """bf16 spacing at each reference value (0 at 0)."""
    _, e = np.frexp(np.asarray(ref, F64))
    return np.where(ref == 0, 0.0, np.ldexp(1.0, e - 8))


def to_bf16(x):
    """f32 -> bf16 (round to nearest even) -> f64, as from_f32<bf16>."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).double().numpy()


def as_np(t):
    return t.detach().cpu().to(torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, F64)


def ratio(got, ref, bound):
    """max |got - ref| / bound; a difference where the bound is 0, or a NaN, gives inf."""
    got, ref = as_np(got), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got - ref)
    if np.isnan(d).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ rag_mean --
def unpack_bits(bits, n_cols):
    """bit-packed rows (site s = bit s & 7 of byte s >> 3) -> 0/1 [n, n_cols]"""
    return np.unpackbits(np.asarray(bits, np.uint8), axis=1, bitorder="little")[:, :n_cols]


def pack_bits(codes):
    return np.packbits(np.asarray(codes, np.uint8) & 1, axis=1, bitorder="little")


def _gather_counts(idx, rows, ok, n_cols):
    out = np.zeros((idx.shape[0], n_cols), np.int64)
    if rows.shape[0] == 0:
        return out
    r = np.where(ok, idx, 0)
    for q in range(idx.shape[0]):                     # [k, n_cols] at a time
        out[q] = (rows[r[q], :n_cols].astype(np.int64) * ok[q][:, None]).sum(0)
    return out


def position_tokens(L, n_sites, ids, eos_late=False):
    """token of every position, tok0 standing for the sites"""
    t = np.full(L, ids["pad"], np.int64)
    t[0] = ids["sos"]
    t[1:1 + n_sites] = ids["tok0"]
    if n_sites + 1 + int(eos_late) < L:
        t[n_sites + 1 + int(eos_late)] = ids["eos"]
    return t


def rag_mean(idx, src, n_sites, W, pe, Ar, L, ids, mode, dtype=F64, fault=None, unit=4, with_abs=False):
    """[nq, L, D] neighbour mean of the complete-token embeddings.  ``src``: u8 panel rows (mode
    "rows"), bit-packed panel rows ("bits") or per-query counts ("counts").  ``unit``: elements per
    16-byte store of the emulated kernel (4 f32, 8 bf16), used by the units_past_256 fault only.
    with_abs: also the A of the bound."""
    idx = np.asarray(idx, np.int64)
    nq, k = idx.shape
    D = W.shape[1]
    ids = dict(ids)
    if fault == "tok_swap":
        ids["tok0"], ids["tok1"] = ids["tok1"], ids["tok0"]
    if fault == "drop_last":
        idx = idx.copy()
        idx[:, -1] = -1
    valid = idx >= 0
    nv = np.full(nq, k) if fault == "nv_counts_invalid" else valid.sum(1)
    if mode == "counts":
        c = np.asarray(src)[:, :n_sites].astype(np.int64)
    else:
        rows = unpack_bits(src, n_sites) if mode == "bits" else np.asarray(src)
        c = _gather_counts(idx, rows, valid, n_sites)
    W, pe = W.astype(dtype), pe.astype(dtype)
    some = nv > 0
    f = np.zeros((nq, n_sites), dtype)
    f[some] = c[some].astype(dtype) / nv[some, None].astype(dtype)
    t = position_tokens(L, n_sites, ids, fault == "eos_late")
    w0, w1 = W[ids["tok0"]], W[ids["tok1"]]
    dw = w1 - w0
    out = np.empty((nq, L, D), dtype)
    out[:] = W[t][None]
    site = slice(1, 1 + n_sites)
    out[:, site] = np.where(some[:, None, None], w0 + f[:, :, None] * dw, dtype(0))
    out = out + pe[:L]
    if Ar is not None:
        out = out + Ar.astype(dtype)
    if fault == "units_past_256":                     # the block's units from 256 on never stored
        cpr = D // unit
        l, d = np.meshgrid(np.arange(L), np.arange(D), indexing="ij")
        out[:, (l % 8) * cpr + d // unit >= 256] = np.nan
    if not with_abs:
        return out
    A = np.empty((nq, L, D), F64)
    A[:] = np.abs(W[t])[None]
    A[:, site] = np.where(some[:, None, None], np.abs(w0) + f[:, :, None] * (np.abs(w0) + np.abs(w1)), 0.0)
    A = A + np.abs(pe[:L]) + (0 if Ar is None else np.abs(Ar))
    return out, A


def rag_mean_bound(A, ref, n_sites, bf16):
    n = np.full(A.shape[1], RAG_PLAIN, F64)
    n[1:1 + n_sites] = RAG_SITE
    return gamma(n)[None, :, None] * A + (bf16_ulp(ref) / 2 if bf16 else 0)


# ------------------------------------------------------------ neighbor_counts --
def neighbor_counts(idx, codes, row0, n_rows, ld_out, bits=False, packed_bytes=False):
    """int64 [nq, ld_out].  packed_bytes: the kernel's four-bytes-in-a-word adds (a count wraps at 256)."""
    idx = np.asarray(idx, np.int64)
    codes = np.asarray(codes, np.uint8)[:n_rows]
    ld = codes.shape[1] * (8 if bits else 1)
    rows = unpack_bits(codes, ld) if bits else codes
    r = idx - row0
    ok = (r >= 0) & (r < n_rows)
    out = np.zeros((idx.shape[0], ld_out), np.int64)
    out[:, :ld] = _gather_counts(r, rows, ok, ld)
    return out & 0xFF if packed_bytes else out


# -------------------------------------------------------------- nbr_mean_drop --
def nbr_tokens(codes, n_sites, L, ids, eos_late=False):
    """[U, L] token of every position of every unique neighbour"""
    codes = np.asarray(codes, np.int64)
    tok = np.tile(position_tokens(L, n_sites, ids, eos_late), (codes.shape[0], 1))
    tok[:, 1:1 + n_sites] = ids["tok0"] + codes[:, :n_sites]
    return tok


def nbr_keep(seed, n_u, L, D, p, wrong_half=False):
    """bool [U, L, D]; wrong_half: feature d takes the half of d ^ 1"""
    keep = ln_keep_mask(seed, NBR_STREAM, n_u, L * D, p).reshape(n_u, L, D)
    return keep.reshape(n_u, L, D // 2, 2)[..., ::-1].reshape(n_u, L, D) if wrong_half else keep


def _fma(m, t, s, dtype):
    if dtype is F64:
        return m * t + s
    return (m.astype(F64) * t.astype(F64) + s.astype(F64)).astype(F32)    # the product is exact in f64


def _nbr_setup(inv, codes, n_sites, L, D, p, seed, ids, dtype, fault):
    inv = np.asarray(inv, np.int64)
    codes = np.asarray(codes, np.uint8)
    if fault == "tok_swap":
        codes = codes ^ 1
    if fault == "drop_last":
        inv = inv.copy()
        inv[:, -1] = -1
    nv = np.full(inv.shape[0], inv.shape[1]) if fault == "nv_counts_invalid" else (inv >= 0).sum(1)
    tok = nbr_tokens(codes, n_sites, L, ids, fault == "eos_late")
    m = nbr_keep(seed, codes.shape[0], L, D, p, fault == "hash_half").astype(dtype) * dtype(drop_scale(p))
    return inv, tok, nv, m


def nbr_mean_drop(inv, codes, n_sites, W, pe, Ar, p, seed, ids, dtype=F64, fault=None, with_abs=False):
    """[nq, L, D]: mean over each query's valid unique neighbours of drop(W[tok] + pe + Ar)"""
    L, D = pe.shape
    inv, tok, nv, m = _nbr_setup(inv, codes, n_sites, L, D, p, seed, ids, dtype, fault)
    W, c = W.astype(dtype), pe.astype(dtype) + Ar.astype(dtype)
    cabs = np.abs(pe.astype(F64)) + np.abs(Ar.astype(F64))
    out = np.zeros((inv.shape[0], L, D), dtype)
    A = np.zeros((inv.shape[0], L, D), F64)
    for q in range(inv.shape[0]):
        s = np.zeros((L, D), dtype)
        inv_nv = dtype(1) / dtype(max(nv[q], 1))
        for u in inv[q][inv[q] >= 0]:
            s = _fma(m[u], W[tok[u]] + c, s, dtype)
            if with_abs:
                A[q] += m[u].astype(F64) * (np.abs(W[tok[u]].astype(F64)) + cabs)
        out[q] = s * inv_nv
        A[q] *= float(inv_nv)
    return (out, A) if with_abs else out


def nbr_forward_bound(A, inv):
    nv = (np.asarray(inv) >= 0).sum(1)
    return gamma(nv + FWD_C)[:, None, None] * A


def nbr_mean_drop_bwd(dout, inv, codes, n_sites, V, p, seed, ids, dW0=None, dAr0=None, dtype=F64, fault=None):
    """(dW [V, D], dAr [L, D]) accumulated onto dW0 / dAr0 (zeros when absent): the exact adjoint of
    nbr_mean_drop in float64, the kernel's order of operations in float32 (block partials added
    in position order)."""
    nq, L, D = dout.shape
    inv, tok, nv, m = _nbr_setup(inv, codes, n_sites, L, D, p, seed, ids, dtype, fault)
    dout = dout.astype(dtype)
    site = np.zeros(L, bool)
    site[1:1 + n_sites] = True
    is1 = tok == ids["tok0"] + 1                      # [U, L]
    ar = np.zeros((L, D), dtype)
    w = np.zeros((2, L, D), dtype)                    # site tokens tok0, tok0 + 1
    ws = np.zeros((L, D), dtype)                      # the position's single token
    zero = dtype(0)
    for q in range(nq):
        if (inv[q] >= 0).sum() == 0:
            continue
        g = dout[q] / dtype(nv[q])
        for u in inv[q][inv[q] >= 0]:
            e = g * m[u]
            ar = ar + e
            for c in (0, 1):
                w[c] = w[c] + np.where((site & (is1[u] == bool(c)))[:, None], e, zero)
            ws = ws + np.where(site[:, None], zero, e)
    dAr = (np.zeros((L, D), dtype) if dAr0 is None else dAr0.astype(dtype)) + ar
    dW = np.zeros((V, D), dtype) if dW0 is None else dW0.astype(dtype).copy()
    tpos = position_tokens(L, n_sites, ids, fault == "eos_late")
    for l in range(L):
        if site[l]:
            dW[ids["tok0"]] = dW[ids["tok0"]] + w[0, l]
            dW[ids["tok0"] + 1] = dW[ids["tok0"] + 1] + w[1, l]
        elif tpos[l] != ids["pad"] or fault == "pad_grad":
            dW[tpos[l]] = dW[tpos[l]] + ws[l]
    return dW, dAr


def nbr_backward_bounds(dout, inv, codes, n_sites, V, p, seed, ids, dW0, dAr0):
    """(bound dW, bound dAr): the reference run on magnitudes gives each element's sum |e| + |prior|"""
    nq, L, _ = dout.shape
    k = np.asarray(inv).shape[1]
    z = lambda t, shape: np.zeros(shape) if t is None else np.abs(t.astype(F64))
    aW, aAr = nbr_mean_drop_bwd(np.abs(dout.astype(F64)), inv, codes, n_sites, V, p, seed, ids)
    held = np.zeros(V, bool)                          # rows that some position adds to
    held[[ids["sos"], ids["tok0"], ids["tok0"] + 1, ids["eos"]]] = True
    bW = gamma(nq * k + L + BWD_W_C) * (aW + z(dW0, aW.shape)) * held[:, None]
    return bW, gamma(nq * k + BWD_AR_C) * (aAr + z(dAr0, aAr.shape))


# -------------------------------------------------------------------- inputs --
def _rng(*key):
    return np.random.default_rng([int(x) & 0xFFFFFFFF for x in key])


def _ints(g, shape, lo, hi):
    return g.integers(lo, hi + 1, size=shape).astype(F32)


def ceil16(n):
    return max(16, cdiv(n, 16) * 16)


def _neighbour_lists(g, nq, k, n_ref, exact, dtype):
    """[nq, k] with query q of pattern q % 4: full, leading -1s, all -1, trailing -1s (a lone query
    is full for k = 1, else has one leading -1).  exact: every count of valid entries a power of two."""
    out = np.full((nq, k), -1, dtype)
    for q in range(nq):
        pat = q % 4 if nq > 1 else (0 if k == 1 else 1)
        if pat == 2:
            continue
        n = k if pat == 0 or k == 1 else (k - 1 if nq == 1 else int(g.integers(1, k)))
        if exact:
            n = 1 << (n.bit_length() - 1)
        rows = g.permutation(n_ref)[:n]
        if pat == 1:
            out[q, k - n:] = rows
        else:
            out[q, :n] = rows
    return out


# (name, nq, k, L, D, n_sites, Ar, ids, kind): see test_gpu_neighbour_mean.py for what each reaches
RAG_CASES = (
    ("one", 1, 1, 8, 8, 6, True, IDS, "random"),
    ("eos_slot0", 15, 8, 17, 64, 7, True, IDS, "exact"),
    ("k128_d136", 16, 128, 15, 136, 11, True, IDS, "exact"),
    ("model_d384", 17, 8, 80, 384, 78, True, IDS, "random"),
    ("no_sites", 33, 128, 9, 136, 0, True, IDS, "random"),
    ("alt_ids_d384", 17, 8, 23, 384, 15, False, IDS_ALT, "exact"),
    ("alt_ids_d64", 33, 8, 16, 64, 13, False, IDS_ALT, "random"),
)
RAG_NAMES = tuple(c[0] for c in RAG_CASES)
RAG_N_REF = 160


@functools.lru_cache(maxsize=None)
def rag_case(name):
    _, nq, k, L, D, n_sites, has_ar, ids, kind = RAG_CASES[RAG_NAMES.index(name)]
    exact = kind == "exact"
    g = _rng(1, RAG_NAMES.index(name))
    if exact:
        W = _ints(g, (VOCAB, D), -60, 60)
        W[ids["tok1"]] = W[ids["tok0"]] + 128 * _ints(g, (D,), -1, 1)
        pe, Ar = _ints(g, (L, D), -30, 30), _ints(g, (L, D), -30, 30)
    else:
        W, pe, Ar = (g.standard_normal(s).astype(F32) for s in ((VOCAB, D), (L, D), (L, D)))
    ld = ceil16(n_sites) + 16                         # rows and counts longer than the window
    codes = g.integers(0, 2, size=(RAG_N_REF, ld)).astype(np.uint8)      # columns past n_sites: noise
    ldb = 2 * cdiv(max(n_sites, 1), 16)
    bits = pack_bits(codes[:, :8 * ldb])              # bits past n_sites: the same noise
    idx = _neighbour_lists(g, nq, k, RAG_N_REF, exact, np.int64)
    counts = np.full((nq, ld), 77, np.uint8)
    counts[:, :n_sites] = _gather_counts(idx, codes, idx >= 0, n_sites)
    return SimpleNamespace(name=name, nq=nq, k=k, L=L, D=D, n_sites=n_sites, ids=ids, exact=exact, W=W, pe=pe,
                           Ar=Ar if has_ar else None, idx=idx, rows=codes, bits=bits, counts=counts)


def rag_src(c, mode):
    return {"rows": c.rows, "bits": c.bits, "counts": c.counts}[mode]


def rag_expected(c, mode, bf16):
    """(reference, bound); bound 0 on the exact tables"""
    ref, A = rag_mean(c.idx, rag_src(c, mode), c.n_sites, c.W, c.pe, c.Ar, c.L, c.ids, mode, with_abs=True)
    return ref, (np.zeros_like(ref) if c.exact else rag_mean_bound(A, ref, c.n_sites, bf16))


# (name, nq, k, ld (sites), ld_out, row0, n_rows)
COUNT_CASES = (
    ("k128_full", 3, 128, 32, 32, 0, 130),
    ("shard_ends", 5, 8, 16, 48, 1000, 20),
    ("two_blocks", 129, 8, 32, 32, 7, 40),
    ("no_rows", 4, 8, 16, 32, 5, 0),
)
COUNT_NAMES = tuple(c[0] for c in COUNT_CASES)


@functools.lru_cache(maxsize=None)
def count_case(name):
    _, nq, k, ld, ld_out, row0, n_rows = COUNT_CASES[COUNT_NAMES.index(name)]
    g = _rng(2, COUNT_NAMES.index(name))
    codes = g.integers(0, 2, size=(n_rows, ld)).astype(np.uint8)
    if name == "k128_full":
        codes[:, [0, 3, 15, 16, 31]] = 1              # every neighbour has a 1: the count is 128
        idx = np.stack([g.permutation(n_rows)[:k] for _ in range(nq)]).astype(np.int64)
    else:
        idx = g.integers(row0 - 4, row0 + n_rows + 4, size=(nq, k)).astype(np.int64)
        idx[:, :5] = [row0 - 1, row0, row0 + n_rows - 1, row0 + n_rows, -1]
        idx[0] = -1
    return SimpleNamespace(name=name, nq=nq, k=k, ld=ld, ld_out=ld_out, row0=row0, n_rows=n_rows, idx=idx,
                           rows=codes, bits=pack_bits(codes).reshape(n_rows, ld // 8))


# (tag, nq, k, L, D, n_sites, U, ids); every case runs at p = 0 (random), 0.5 (exact) and 0.3 (random)
FWD_SHAPES = (
    ("q1_d2", 1, 8, 6, 2, 3, 12, IDS),
    ("q3_d64", 3, 8, 9, 64, 7, 9, IDS_NBR_ALT),
    ("q4_d126", 4, 3, 5, 126, 3, 6, IDS),
    ("q5_d128", 5, 8, 5, 128, 3, 9, IDS),
    ("q3_d130", 3, 8, 5, 130, 3, 9, IDS),
    ("q5_d384", 5, 8, 6, 384, 4, 9, IDS),
    ("q257_d8", 257, 4, 4, 8, 2, 12, IDS),
    ("q260_d8", 260, 4, 4, 8, 2, 12, IDS),
)
# (tag, nq, k, L, D, n_sites, U, V, ids): nthr 64, 128, 192, 256, two strides at the LDS limit, four strides
BWD_SHAPES = (
    ("d2", 5, 8, 6, 2, 3, 12, 10, IDS),
    ("d130", 3, 4, 6, 130, 3, 6, 10, IDS_NBR_ALT),
    ("d384", 3, 8, 7, 384, 4, 9, 10, IDS),
    ("d512", 3, 4, 5, 512, 2, 6, 10, IDS),
    ("d1024_v16", 3, 4, 5, 1024, 2, 6, 16, IDS),
    ("d2048_v8", 3, 4, 5, 2048, 2, 6, 8, IDS),
)
P_KINDS = ((0.0, "random"), (0.5, "exact"), (0.3, "random"))
P_ID = {0.0: "p0", 0.5: "p0.5_exact", 0.3: "p0.3"}
FWD_NAMES = tuple(f"{s[0]}-{P_ID[p]}" for s in FWD_SHAPES for p, _ in P_KINDS)
BWD_NAMES = tuple(f"{s[0]}-{P_ID[p]}" for s in BWD_SHAPES for p, _ in P_KINDS)


def _nbr_case(name, shapes, bwd):
    tag, ptag = name.split("-")
    shape = next(s for s in shapes if s[0] == tag)
    p, kind = next(pk for pk in P_KINDS if P_ID[pk[0]] == ptag)
    _, nq, k, L, D, n_sites, n_u = shape[:7]
    V, ids = (shape[7], shape[8]) if bwd else (VOCAB, shape[7])
    exact = kind == "exact"
    g = _rng(3 + bwd, [s[0] for s in shapes].index(tag), int(p * 10))
    mk = (lambda s, a: _ints(g, s, -a, a)) if exact else (lambda s, a: g.standard_normal(s).astype(F32))
    W, pe, Ar = mk((V, D), 8), mk((L, D), 4), mk((L, D), 4)
    ld = ceil16(n_sites) + 16                         # ld_codes > n_sites
    codes = g.integers(0, 2, size=(n_u, ld)).astype(np.uint8)
    inv = _neighbour_lists(g, nq, k, n_u, exact, np.int32)
    c = SimpleNamespace(name=name, nq=nq, k=k, L=L, D=D, n_sites=n_sites, U=n_u, V=V, ids=ids, p=p, exact=exact,
                        seed=SEED + 977 * len(name) + D, W=W, pe=pe, Ar=Ar, codes=codes, inv=inv)
    if bwd:
        c.dout = mk((nq, L, D), 8)
        c.dW0, c.dAr0 = mk((V, D), 8), mk((L, D), 8)
        c.dW0[ids["pad"]] = 0
    return c


@functools.lru_cache(maxsize=None)
def fwd_case(name):
    return _nbr_case(name, FWD_SHAPES, False)


@functools.lru_cache(maxsize=None)
def bwd_case(name):
    return _nbr_case(name, BWD_SHAPES, True)


@functools.lru_cache(maxsize=None)
def fwd_expected(name):
    c = fwd_case(name)
    ref, A = nbr_mean_drop(c.inv, c.codes, c.n_sites, c.W, c.pe, c.Ar, c.p, c.seed, c.ids, with_abs=True)
    return ref, (np.zeros_like(ref) if c.exact else nbr_forward_bound(A, c.inv))


@functools.lru_cache(maxsize=None)
def bwd_expected(name):
    """(dW, dAr, bound dW, bound dAr)"""
    c = bwd_case(name)
    a = (c.dout, c.inv, c.codes, c.n_sites, c.V, c.p, c.seed, c.ids, c.dW0, c.dAr0)
    dW, dAr = nbr_mean_drop_bwd(*a)
    bW, bAr = nbr_backward_bounds(*a)
    return (dW, dAr, np.zeros_like(dW), np.zeros_like(dAr)) if c.exact else (dW, dAr, bW, bAr)


def keep_of(c):
    """the mask rows of the unique neighbours that some query of the case holds: [n, L, D]"""
    used = np.unique(c.inv[c.inv >= 0])
    return nbr_keep(c.seed, c.U, c.L, c.D, c.p)[used]
