"""Typed torch-tensor wrappers over the C ABI (one function per ``snvrag_*`` entry).

All tensors must be contiguous device tensors; outputs are allocated here unless
passed in.  Every call runs on the current HIP stream.  No CPU fallback.
"""

from __future__ import annotations

import contextlib

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import native as N
from .native import check, ptr, stream_ptr

_dt = N.dtype_code


def _c(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return t


# ------------------------------------------------------------------ linear --
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
           act: int = N.ACT_NONE, slope: float = 0.0,
           row1: Optional[Tuple[torch.Tensor, int, torch.Tensor]] = None,
           row2: Optional[Tuple[torch.Tensor, int, torch.Tensor]] = None,
           row_period: int = 0, resid: Optional[torch.Tensor] = None,
           ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ln_act: int = N.ACT_NONE, ln_eps: float = 1e-5,
           post_base: Optional[torch.Tensor] = None, post_scale: float = 1.0,
           post_af: Optional[torch.Tensor] = None, post_af_period: int = 0, post_maf: bool = False,
           stats_out: Optional[torch.Tensor] = None,
           rownorm: Optional[Tuple[torch.Tensor, int, int, torch.Tensor]] = None,
           out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """out[m, n] = act(x[m] . w[n] + bias[n] + row1[m]*col1[n] + row2[m]*col2[n]) + resid[m, n],
    optionally followed by a fused LayerNorm over the row (``ln=(g, b)``, + ``ln_act`` and the
    ``post_base + post_scale * y * maf(post_af)`` tail), or writing row statistics
    (``stats_out`` float32 [n_tiles, M, 2]); ``rownorm=(stats, n_parts, dim, c1)`` folds a
    LayerNorm of ``x`` into the epilogue (``w`` must be pre-scaled by gamma, ``c1 = w_orig @ gamma``,
    beta folded into ``bias``) — see :func:`fold_layernorm`."""
    N.require_gpu(x, w)
    K = x.shape[-1]
    M = x.numel() // K
    Nn = w.shape[0]
    assert w.shape[1] == K and w.dtype == x.dtype, (tuple(w.shape), K, w.dtype, x.dtype)
    od = out_dtype or (out.dtype if out is not None else x.dtype)
    if out is None:
        out = torch.empty(*x.shape[:-1], Nn, device=x.device, dtype=od)
    e = N.Epilogue()
    e.bias = ptr(bias)
    if row1 is not None:
        e.row1, e.row1_stride, e.col1 = ptr(row1[0]), row1[1], ptr(row1[2])
    if row2 is not None:
        e.row2, e.row2_stride, e.col2 = ptr(row2[0]), row2[1], ptr(row2[2])
    e.row_period, e.act, e.slope = row_period, act, slope
    if resid is not None:
        assert resid.dtype == od and resid.shape[-1] == Nn
        e.resid, e.ld_resid = ptr(_c(resid)), Nn
    if ln is not None:
        e.ln_g, e.ln_b, e.ln_eps, e.ln_act = ptr(ln[0]), ptr(ln[1]), ln_eps, ln_act
    if post_base is not None:
        assert post_base.dtype == od
        e.post_base, e.ld_post, e.post_scale = ptr(_c(post_base)), Nn, post_scale
    if post_af is not None:
        e.post_af, e.post_af_period, e.post_maf = ptr(_c(post_af)), post_af_period, int(post_maf)
    e.stats_out = ptr(stats_out)
    an = None
    if rownorm is not None:
        st, parts, dim, c1 = rownorm
        an = N.RowNormS(ptr(st), parts, dim, 1e-5, ptr(c1))
    check(N.lib().snvrag_linear_ex(_dt(x.dtype), _dt(od), M, Nn, K, ptr(_c(x)), K, ptr(_c(w)), K,
                                   ptr(out), Nn, C.byref(e), C.byref(an) if an is not None else None,
                                   stream_ptr()), "linear")
    return out


def fold_layernorm(w: torch.Tensor, b: torch.Tensor, g: torch.Tensor, beta: torch.Tensor, dtype: torch.dtype):
    """LN(x) W^T + b = rstd*(x (W diag g)^T) - rstd*mean*(W g) + (W beta + b): returns (W', bias', c1)."""
    w64 = w.double()
    wg = (w64 * g.double()[None, :]).to(dtype).contiguous()
    return wg, (w64 @ beta.double() + b.double()).float().contiguous(), (w64 @ g.double()).float().contiguous()


def ffn_vec(b1, b2g, w2g, ln2_g, ln2_b) -> torch.Tensor:
    """[b1 (4D) | b2' | c1 | ln2_g | ln2_b] f32; c1 = row sums of the bf16 w2g."""
    c1 = w2g.to(torch.bfloat16).double().sum(1).float()
    return torch.cat([t.detach().float().reshape(-1) for t in (b1, b2g, c1, ln2_g, ln2_b)]).contiguous()


def tail_pack(w_o: torch.Tensor, w1: torch.Tensor, w2g: torch.Tensor) -> torch.Tensor:
    """One weight stream (W_o', then per 64-unit hidden chunk W1 and W2') of the 32x32-MFMA
    block tail (csrc/tail.hip)."""
    D = w_o.shape[1]
    nbytes = int(N.lib().snvrag_tail_pack_bytes(D))
    if nbytes == 0:
        raise ValueError(f"block tail needs D in (128, 256, 384), got {D}")
    ws = [_c(t.to(torch.bfloat16).contiguous()) for t in (w_o, w1, w2g)]
    assert tuple(ws[0].shape) == (D, D) and tuple(ws[1].shape) == (4 * D, D) and tuple(ws[2].shape) == (D, 4 * D)
    out = torch.empty(nbytes, device=w_o.device, dtype=torch.uint8)
    check(N.lib().snvrag_tail_pack(D, ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(out), stream_ptr()), "tail_pack")
    return out


def proj_pack(w: torch.Tensor) -> torch.Tensor:
    """Stream of W [NC*D, D] (bf16) for ``proj_forward`` (NC = W.shape[0] // D)."""
    N.require_gpu(w)
    n, D = w.shape
    NC = n // D
    nbytes = int(N.lib().snvrag_proj_pack_bytes(D, NC))
    assert nbytes > 0 and NC * D == n, "projection needs D in {128, 256, 384} and NC*D rows"
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    wb = _c(w.to(torch.bfloat16))
    check(N.lib().snvrag_proj_pack(D, NC, ptr(wb), ptr(out), stream_ptr()), "proj_pack")
    return out


def proj_forward(x: torch.Tensor, wstream: torch.Tensor, bias: torch.Tensor, NC: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [M, NC*D] = x W^T + bias on the 32x32-MFMA stream kernel (bf16)."""
    N.require_gpu(x)
    assert x.dtype == torch.bfloat16
    D = x.shape[-1]
    M = x.numel() // D
    if out is None:
        out = torch.empty(M, NC * D, device=x.device, dtype=torch.bfloat16)
    b = _c(bias.float())
    check(N.lib().snvrag_proj_forward(M, D, NC, ptr(_c(x)), ptr(wstream), ptr(b), ptr(out), stream_ptr()),
          "proj_forward")
    return out


def tail_forward(att: torch.Tensor, x: torch.Tensor, wstream: torch.Tensor, b_o, ln1_g, ln1_b,
                 ffn_vec: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """x <- LN2(x1 + FFN(x1)), x1 = LN1(x + att W_o^T + b_o), in place (32x32-MFMA kernel)."""
    N.require_gpu(att, x)
    assert att.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and x.is_contiguous()
    D = x.shape[-1]
    M = x.numel() // D
    f = [_c(t.float().contiguous()) for t in (b_o, ln1_g, ln1_b)]
    check(N.lib().snvrag_tail_forward(M, D, ptr(_c(att)), ptr(x), ptr(wstream), ptr(f[0]), ptr(f[1]), ptr(f[2]),
                                      ptr(_c(ffn_vec)), eps, stream_ptr()), "tail_forward")
    return x


def tail_qkv_forward(att: torch.Tensor, x: torch.Tensor, wstream: torch.Tensor, b_o, ln1_g, ln1_b,
                     ffn_vec: torch.Tensor, qkv_pw: torch.Tensor, b_qkv: torch.Tensor,
                     qkv_out: Optional[torch.Tensor] = None, eps: float = 1e-5):
    """``tail_forward`` in place on x, and in the same launch qkv_out [M, 3 D] = x W_qkv^T + b_qkv of
    the rows it has just written (qkv_pw = ``proj_pack(W_qkv)``): the next layer's QKV projection
    (D = 384, wide-row tail only).  Returns (x, qkv_out)."""
    N.require_gpu(att, x)
    assert att.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and x.is_contiguous()
    D = x.shape[-1]
    M = x.numel() // D
    if qkv_out is None:
        qkv_out = torch.empty(M, 3 * D, device=x.device, dtype=torch.bfloat16)
    assert qkv_out.dtype == torch.bfloat16 and qkv_out.is_contiguous() and qkv_out.numel() == M * 3 * D
    f = [_c(t.float().contiguous()) for t in (b_o, ln1_g, ln1_b, b_qkv)]
    check(N.lib().snvrag_tail_qkv_forward(M, D, ptr(_c(att)), ptr(x), ptr(wstream), ptr(f[0]), ptr(f[1]), ptr(f[2]),
                                          ptr(_c(ffn_vec)), eps, ptr(qkv_pw), ptr(f[3]), ptr(qkv_out), stream_ptr()),
          "tail_qkv_forward")
    return x, qkv_out


def tail_ffn_forward(x1: torch.Tensor, wstream: torch.Tensor, ffn_vec: torch.Tensor, eps: float = 1e-5,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = LN2(x1 + FFN(x1)) (32x32-MFMA kernel, FFN part of the tail stream)."""
    N.require_gpu(x1)
    assert x1.dtype == torch.bfloat16
    D = x1.shape[-1]
    M = x1.numel() // D
    if out is None:
        out = torch.empty_like(x1)
    check(N.lib().snvrag_tail_ffn_forward(M, D, ptr(_c(x1)), ptr(out), ptr(wstream), ptr(_c(ffn_vec)), eps,
                                          stream_ptr()), "tail_ffn_forward")
    return out


def stat_tiles(n: int) -> int:
    """Column tiles of the row-panel GEMM for an N (the stats_out leading dim)."""
    for bn in (384, 256, 128, 64):
        if n % bn == 0:
            return n // bn
    raise ValueError("N must be a multiple of 64")


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, *, resid: Optional[torch.Tensor] = None,
              eps: float = 1e-5, out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
              post_base: Optional[torch.Tensor] = None, post_scale: float = 1.0,
              post_af: Optional[torch.Tensor] = None, af_period: int = 0, maf_weight: bool = False,
              act: int = N.ACT_NONE) -> torch.Tensor:
    N.require_gpu(x)
    Nn = x.shape[-1]
    M = x.numel() // Nn
    od = out_dtype or (out.dtype if out is not None else x.dtype)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=od)
    p = None
    if post_base is not None or post_af is not None or act != N.ACT_NONE:
        p = N.LnPost()
        p.base, p.ld_base, p.scale = ptr(post_base), Nn, post_scale
        p.af, p.af_period, p.maf_weight, p.act = ptr(post_af), af_period, int(maf_weight), act
    check(N.lib().snvrag_layernorm(_dt(x.dtype), _dt(od), M, Nn, ptr(_c(x)), Nn,
                                   ptr(resid), Nn, ptr(g), ptr(b), eps, ptr(out), Nn,
                                   C.byref(p) if p is not None else None, stream_ptr()), "layernorm")
    return out


def attention(qkv: torch.Tensor, nseq: int, L: int, heads: int, dh: int,
              out: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q k^T * scale) v per (sequence, head); scale defaults to 1/sqrt(dh).  scale =
    1/log2(e) declares Q pre-scaled by log2(e)/sqrt(dh) (the engine's q_scale)."""
    N.require_gpu(qkv)
    D = heads * dh
    if out is None:
        out = torch.empty(nseq * L, D, device=qkv.device, dtype=qkv.dtype)
    check(N.lib().snvrag_attention(_dt(qkv.dtype), nseq, L, heads, dh, ptr(_c(qkv)), qkv.shape[-1],
                                   ptr(out), D, 1.0 / float(dh) ** 0.5 if scale is None else float(scale),
                                   stream_ptr()), "attention")
    return out


def attention_fallbacks(reset: bool = True) -> int:
    """Waves that took the exact online-max path of the bf16 dh=32 kernel (see attention.hip)."""
    n = N.lib().snvrag_attention_fallbacks(int(reset))
    if n < 0:
        check(n, "attention_fallbacks")
    return n


# ---------------------------------------------------------------- embedding --
def af_features(af: torch.Tensor, freqs: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    N.require_gpu(af)
    nb = freqs.numel()
    out = torch.empty(*af.shape, 2 * nb, device=af.device, dtype=dtype)
    check(N.lib().snvrag_af_features(_dt(dtype), af.numel(), ptr(_c(af)), ptr(_c(freqs)), nb, ptr(out),
                                     stream_ptr()), "af_features")
    return out


def embed_tokens(tok: torch.Tensor, W: torch.Tensor, pe: torch.Tensor, afemb: Optional[torch.Tensor],
                 af_period: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [nseq, L, D] = W[clamp(tok)] + pe[:L] + afemb[(s % af_period if af_period > 0 else s)];
    ``afemb`` [rows, L, D] (or [L, D] for one shared row), f32 or bf16; ``out`` (e.g. the leading
    rows of a larger block) is filled in place.  Only pointers cross the boundary, so every
    tensor must be the contiguous layout the kernel indexes: anything else raises."""
    N.require_gpu(tok, W, pe, afemb, out)
    assert tok.dtype == torch.int64
    nseq, L = tok.shape
    D = W.shape[1]
    if W.dtype != torch.float32 or pe.dtype != torch.float32 or pe.dim() != 2 or pe.shape[0] < L or pe.shape[1] != D:
        raise ValueError(f"W and pe must be float32 with pe [>= {L}, {D}], got pe {tuple(pe.shape)} {pe.dtype}, W {W.dtype}")
    if afemb is not None:
        rows = af_period if af_period > 0 else nseq
        if afemb.shape[-2:] != (L, D) or afemb.numel() != rows * L * D:
            raise ValueError(f"afemb must be [{rows}, {L}, {D}], got {tuple(afemb.shape)}")
        _c(afemb)
    if out is None:
        out = torch.empty(nseq, L, D, device=tok.device, dtype=dtype)
    elif out.dtype != dtype or tuple(out.shape) != (nseq, L, D):
        raise ValueError(f"out must be {dtype} [{nseq}, {L}, {D}], got {out.dtype} {tuple(out.shape)}")
    check(N.lib().snvrag_embed_tokens(_dt(dtype), nseq, L, D, ptr(_c(tok)), ptr(_c(W)), W.shape[0],
                                      ptr(_c(pe)), ptr(afemb), _dt(afemb.dtype) if afemb is not None else 0,
                                      af_period, ptr(_c(out)), stream_ptr()), "embed_tokens")
    return out


def posfeat(pos: torch.Tensor, w: "N.PosfeatW") -> torch.Tensor:
    N.require_gpu(pos)
    B, L = pos.shape
    out = torch.empty(B, L, device=pos.device, dtype=torch.float32)
    check(N.lib().snvrag_posfeat(B, L, ptr(_c(pos)), C.byref(w), ptr(out), stream_ptr()), "posfeat")
    return out


def af_gate(af: torch.Tensor, af_p: torch.Tensor, w: "N.AfGateW", D: int, dtype: torch.dtype) -> torch.Tensor:
    N.require_gpu(af)
    out = torch.empty(*af.shape, D, device=af.device, dtype=dtype)
    check(N.lib().snvrag_af_gate(_dt(dtype), af.numel(), D, ptr(_c(af)), ptr(_c(af_p)), C.byref(w), ptr(out),
                                 stream_ptr()), "af_gate")
    return out


def rag_concat(q: torch.Tensor, rag: torch.Tensor, wgt: torch.Tensor, period: int) -> torch.Tensor:
    D = q.shape[-1]
    M = q.numel() // D
    out = torch.empty(*q.shape[:-1], 2 * D, device=q.device, dtype=q.dtype)
    check(N.lib().snvrag_rag_weighted_concat(_dt(q.dtype), M, D, ptr(_c(q)), ptr(_c(rag)), ptr(_c(wgt)),
                                             period, ptr(out), stream_ptr()), "rag_concat")
    return out


def hap_head_out(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor, want_logits: bool = True):
    K = h.shape[-1]
    M = h.numel() // K
    probs = torch.empty(*h.shape[:-1], 2, device=h.device, dtype=torch.float32)
    logits = torch.empty_like(probs) if want_logits else None
    check(N.lib().snvrag_hap_head_out(_dt(h.dtype), M, K, ptr(_c(h)), K, ptr(_c(w)), ptr(_c(b)),
                                      ptr(logits), ptr(probs), stream_ptr()), "hap_head_out")
    return logits, probs


def gt_head(p1, p2, ref, het, hom, period: int, w: "N.GtW") -> torch.Tensor:
    M = p1.numel() // 2
    out = torch.empty(*p1.shape[:-1], 4, device=p1.device, dtype=torch.float32)
    check(N.lib().snvrag_gt_head(M, ptr(_c(p1)), ptr(_c(p2)), ptr(_c(ref)), ptr(_c(het)), ptr(_c(hom)), period,
                                 C.byref(w), ptr(out), stream_ptr()), "gt_head")
    return out


# ---------------------------------------------------------------------- kNN --
def knn_lut(tok_q: torch.Tensor, W: torch.Tensor, site_mask: torch.Tensor, n_sites: int, n_sites_pad: int,
            limbs: int = 2, Aq: Optional[torch.Tensor] = None, aq_period: int = 0,
            Ar: Optional[torch.Tensor] = None, tok0: int = 5, tok1: int = 6, mask_tok: int = 4,
            Wp: Optional[torch.Tensor] = None):
    """Returns (lut bytes tensor, exps int32 [nq], consts f32 [nq]).  ``Wp``: the panel side's
    token table when it differs from the queries' (a cached panel embedding, snvrag_knn_lut_panel)."""
    N.require_gpu(tok_q)
    nq, L = tok_q.shape
    D = W.shape[1]
    nbytes = N.lib().snvrag_knn_lut_bytes(nq, n_sites_pad, limbs)
    lut = torch.empty(nbytes, device=tok_q.device, dtype=torch.int8)
    exps = torch.empty(nq, device=tok_q.device, dtype=torch.int32)
    consts = torch.empty(nq, device=tok_q.device, dtype=torch.float32)
    if Wp is not None and Wp is not W:
        assert Wp.shape == W.shape and Wp.dtype == torch.float32
        check(N.lib().snvrag_knn_lut_panel(nq, L, D, ptr(_c(tok_q)), ptr(_c(W)), ptr(_c(Wp)), ptr(Aq), aq_period,
                                           ptr(Ar), ptr(_c(site_mask)), n_sites, n_sites_pad, tok0, tok1, mask_tok,
                                           limbs, ptr(lut), ptr(exps), ptr(consts), stream_ptr()), "knn_lut_panel")
    else:
        check(N.lib().snvrag_knn_lut(nq, L, D, ptr(_c(tok_q)), ptr(_c(W)), ptr(Aq), aq_period, ptr(Ar),
                                     ptr(_c(site_mask)), n_sites, n_sites_pad, tok0, tok1, mask_tok, limbs,
                                     ptr(lut), ptr(exps), ptr(consts), stream_ptr()), "knn_lut")
    return lut, exps, consts


def knn_scan(codes: torch.Tensor, n_sites_pad: int, lut: torch.Tensor, nq: int, limbs: int, k: int,
             ref_offset: int = 0, n_parts: Optional[int] = None, th_init: Optional[torch.Tensor] = None) -> torch.Tensor:
    n_ref, ld = codes.shape
    if n_parts is None:
        n_parts = N.lib().snvrag_knn_scan_parts(n_ref, nq)
    parts = torch.empty(n_parts, nq, k, device=codes.device, dtype=torch.int64)
    if th_init is not None:
        assert th_init.dtype == torch.int32 and th_init.numel() == nq
    check(N.lib().snvrag_knn_scan(ptr(_c(codes)), n_ref, ld, n_sites_pad, ptr(lut), nq, limbs, k, ref_offset,
                                  ptr(parts), n_parts, ptr(th_init), stream_ptr()), "knn_scan")
    return parts


def knn_scan_bits(bits: torch.Tensor, n_sites_pad: int, lut: torch.Tensor, nq: int, limbs: int, k: int,
                  ref_offset: int = 0, n_parts: Optional[int] = None,
                  th_init: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``knn_scan`` over the bit-packed panel (u8 [n_ref, ld_bits], ``panel_pack_bits``): the same
    part keys bit for bit."""
    assert bits.dtype == torch.uint8 and bits.dim() == 2
    n_ref, ldb = bits.shape
    if n_parts is None:
        n_parts = N.lib().snvrag_knn_scan_parts(n_ref, nq)
    parts = torch.empty(n_parts, nq, k, device=bits.device, dtype=torch.int64)
    if th_init is not None:
        assert th_init.dtype == torch.int32 and th_init.numel() == nq
    check(N.lib().snvrag_knn_scan_bits(ptr(_c(bits)), n_ref, ldb, n_sites_pad, ptr(lut), nq, limbs, k, ref_offset,
                                       ptr(parts), n_parts, ptr(th_init), stream_ptr()), "knn_scan_bits")
    return parts


def knn_threshold(keys: torch.Tensor, k: int) -> torch.Tensor:
    """Per-query strict start threshold (int32 [nq]) from merged keys [nq, k]."""
    nq = keys.shape[0]
    th = torch.empty(nq, device=keys.device, dtype=torch.int32)
    check(N.lib().snvrag_knn_threshold(ptr(_c(keys)), nq, k, ptr(th), stream_ptr()), "knn_threshold")
    return th


def topk_merge(keys: torch.Tensor, k: int) -> torch.Tensor:
    """keys int64 view of uint64 [n_lists, nq, k] -> [nq, k]."""
    n_lists, nq, kk = keys.shape
    assert kk == k
    out = torch.empty(nq, k, device=keys.device, dtype=torch.int64)
    wsb = N.lib().snvrag_topk_merge_ws_bytes(n_lists, nq, k)
    ws = torch.empty(wsb, device=keys.device, dtype=torch.uint8)
    check(N.lib().snvrag_topk_merge(ptr(_c(keys)), n_lists, nq, k, ptr(out), ptr(ws), wsb, stream_ptr()),
          "topk_merge")
    return out


def knn_decode(keys: torch.Tensor, exps: Optional[torch.Tensor] = None, consts: Optional[torch.Tensor] = None):
    nq, k = keys.shape
    idx = torch.empty(nq, k, device=keys.device, dtype=torch.int64)
    dist = torch.empty(nq, k, device=keys.device, dtype=torch.float32) if exps is not None else None
    check(N.lib().snvrag_knn_decode(ptr(_c(keys)), nq, k, ptr(exps), ptr(consts), ptr(idx), ptr(dist),
                                    stream_ptr()), "knn_decode")
    return idx, dist


def knn_emb_norms(E: torch.Tensor, chunk: int = 4096) -> torch.Tensor:
    """Squared L2 norms (f32) of the bf16 rows of E [N, K] — computed once when the embedding
    index is built (the stored-norm half of IndexFlatL2's ||q||^2 + ||r||^2 - 2 q.r)."""
    out = torch.empty(E.shape[0], device=E.device, dtype=torch.float32)
    for i in range(0, E.shape[0], chunk):
        out[i:i + chunk] = E[i:i + chunk].float().pow(2).sum(1)
    return out


def knn_emb_pack(E: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scan's index layout (csrc/knn_emb.hip header): bf16 E [N, K] row-major -> bf16
    [ceil(N / 32) * 32, K] viewed storage of 4 KiB 32-row x 64-k tiles, padding rows zero.
    ``out`` (e.g. a slice of a larger packed index starting at a row multiple of 32) is filled in
    place."""
    assert E.dtype == torch.bfloat16 and E.dim() == 2
    n, kk = E.shape
    assert kk % 64 == 0
    rows = int(N.lib().snvrag_knn_emb_packed_bytes(n, kk)) // (2 * kk)
    if out is None:
        out = torch.empty(rows, kk, device=E.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() >= rows * kk
    check(N.lib().snvrag_knn_emb_pack(ptr(_c(E)), n, kk, ptr(out), stream_ptr()), "knn_emb_pack")
    return out


def knn_emb_dist(Et: torch.Tensor, Q: torch.Tensor, rn: torch.Tensor, qn: Optional[torch.Tensor] = None,
                 splits: Optional[int] = None) -> torch.Tensor:
    """Exact squared-L2 distances [Bq, N] between bf16 query rows Q [Bq, K] and the panel's
    flattened window embeddings, packed by ``knn_emb_pack`` (Et; N = len(rn), the rows' squared
    norms) (csrc/knn_emb.hip; the reference's cdist over [N, L * D], embedding_rag_dataset.py:390-402)."""
    assert Et.dtype == torch.bfloat16 and Q.dtype == torch.bfloat16 and Et.shape[1] == Q.shape[1]
    n, kk = rn.shape[0], Et.shape[1]
    assert Et.shape[0] == (n + 31) // 32 * 32, "Et must be knn_emb_pack's output for len(rn) rows"
    bq = Q.shape[0]
    assert 0 < bq <= 128 and kk % 64 == 0
    if splits is None:
        splits = int(N.lib().snvrag_knn_emb_splits(n, kk, bq))
    if qn is None:
        qn = knn_emb_norms(Q)
    ws = torch.empty(int(N.lib().snvrag_knn_emb_ws_bytes(n, bq, splits)) // 4, device=Et.device, dtype=torch.float32)
    check(N.lib().snvrag_knn_emb_scan(ptr(_c(Et)), n, kk, ptr(_c(Q)), bq, splits, ptr(ws), stream_ptr()),
          "knn_emb_scan")
    dist = torch.empty(bq, n, device=Et.device, dtype=torch.float32)
    check(N.lib().snvrag_knn_emb_finish(ptr(ws), splits, bq, n, ptr(_c(qn.float())), ptr(_c(rn.float())), ptr(dist),
                                        stream_ptr()), "knn_emb_finish")
    return dist


def knn_emb_search(Et: torch.Tensor, Q: torch.Tensor, k: int, rn: torch.Tensor, qn: Optional[torch.Tensor] = None):
    """(dist [Bq, k], idx [Bq, k]) — the k nearest panel rows in embedding space, ascending
    (torch.topk(largest=False) of embedding_rag_dataset.py:401 over the distance row); Et packed
    by knn_emb_pack."""
    d = knn_emb_dist(Et, Q, rn, qn)
    return torch.topk(d, k, dim=1, largest=False, sorted=True)


def rag_mean(idx: torch.Tensor, codes: torch.Tensor, n_sites: int, W: torch.Tensor, pe: torch.Tensor,
             Ar: Optional[torch.Tensor], L: int, dtype: torch.dtype, tok0=5, tok1=6, sos=2, eos=3, pad=0,
             out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, bits: bool = False):
    """[nq, L, D] mean over the k neighbours of their complete-token embeddings; ``out`` (e.g. the
    rag half of the encoder's input block) is written in place.  ``counts`` (u8 [nq, ld], the
    per-site alt-allele counts over the neighbours, see ``neighbor_counts``) replaces the panel
    rows ``codes[idx]`` (sharded panels; ``codes`` is then unused).  ``bits``: ``codes`` is the
    bit-packed panel (``panel_pack_bits``), read in place."""
    nq, k = idx.shape
    D = W.shape[1]
    if out is None:
        out = torch.empty(nq, L, D, device=idx.device, dtype=dtype)
    assert out.dtype == dtype and tuple(out.shape) == (nq, L, D) and out.is_contiguous()
    if counts is not None:
        assert counts.dtype == torch.uint8 and counts.shape[0] == nq
        check(N.lib().snvrag_rag_mean_counts(_dt(dtype), nq, L, D, k, ptr(_c(idx)), ptr(_c(counts)), counts.shape[1],
                                             n_sites, ptr(_c(W)), ptr(_c(pe)), ptr(Ar), tok0, tok1, sos, eos, pad,
                                             ptr(out), stream_ptr()), "rag_mean_counts")
        return out
    if bits:
        check(N.lib().snvrag_rag_mean_bits(_dt(dtype), nq, L, D, k, ptr(_c(idx)), ptr(_c(codes)), codes.shape[1],
                                           n_sites, ptr(_c(W)), ptr(_c(pe)), ptr(Ar), tok0, tok1, sos, eos, pad,
                                           ptr(out), stream_ptr()), "rag_mean_bits")
        return out
    check(N.lib().snvrag_rag_mean(_dt(dtype), nq, L, D, k, ptr(_c(idx)), ptr(_c(codes)), codes.shape[1], n_sites,
                                  ptr(_c(W)), ptr(_c(pe)), ptr(Ar), tok0, tok1, sos, eos, pad, ptr(out),
                                  stream_ptr()), "rag_mean")
    return out


def neighbor_counts(idx: torch.Tensor, codes: torch.Tensor, row0: int, ld_out: Optional[int] = None,
                    out: Optional[torch.Tensor] = None, bits: bool = False) -> torch.Tensor:
    """u8 [nq, ld_out]: per-site alt-allele counts over the neighbours ``idx`` (global, int64
    [nq, k]) that fall in this shard's rows [row0, row0 + codes.shape[0]).  ``bits``: ``codes`` is
    the bit-packed shard (``panel_pack_bits``); ld_out defaults to its 8 * ld_bits sites."""
    nq, k = idx.shape
    n_rows, ld = codes.shape
    ld_out = ld_out or (8 * ld if bits else ld)
    if out is None:
        out = torch.empty(nq, ld_out, device=idx.device, dtype=torch.uint8)
    if bits:
        check(N.lib().snvrag_neighbor_counts_bits(nq, k, ptr(_c(idx)), ptr(_c(codes)), ld, row0, n_rows, ptr(out),
                                                  ld_out, stream_ptr()), "neighbor_counts_bits")
        return out
    check(N.lib().snvrag_neighbor_counts(nq, k, ptr(_c(idx)), ptr(_c(codes)), ld, row0, n_rows, ptr(out), ld_out,
                                         stream_ptr()), "neighbor_counts")
    return out


def hamming_topk(codes_wm: torch.Tensor, queries: torch.Tensor, k: int) -> torch.Tensor:
    """Exact top-k keys [nq, k] ((d + 2^30) << 32 | row, (d, row) order) of bit-packed 0/1 rows
    (word-major int32 [nw, N]) for bit-packed queries (int32 [nq, nw]); d = Hamming distance."""
    nw, n = codes_wm.shape
    nq = queries.shape[0]
    assert queries.shape[1] == nw and codes_wm.dtype == torch.int32 and queries.dtype == torch.int32
    n_lists = int(N.lib().snvrag_hamming_list_count())
    lists = torch.empty(n_lists, nq, k, device=queries.device, dtype=torch.int64)
    check(N.lib().snvrag_hamming_lists(nq, n, nw, k, ptr(_c(codes_wm)), ptr(_c(queries)), ptr(lists),
                                       stream_ptr()), "hamming_lists")
    return topk_merge(lists, k)


def panel_synth(n_ref: int, n_sites: int, af: torch.Tensor, seed: int, ld: Optional[int] = None,
                row0: int = 0) -> torch.Tensor:
    """Rows [row0, row0 + n_ref) of the hash-generated synthetic panel (u8 [n_ref, ld])."""
    N.require_gpu(af)
    ld = ld or max(256, ((n_sites + 255) // 256) * 256)
    codes = torch.empty(n_ref, ld, device=af.device, dtype=torch.uint8)
    check(N.lib().snvrag_panel_synth_rows(ptr(codes), row0, n_ref, ld, n_sites, ptr(_c(af)), seed, stream_ptr()),
          "panel_synth")
    return codes


def panel_synth_bits(n_ref: int, n_sites: int, af: torch.Tensor, seed: int, ld_bits: Optional[int] = None,
                     row0: int = 0) -> torch.Tensor:
    """``panel_synth``'s rows written straight as bits (u8 [n_ref, ld_bits], site s = bit s & 7 of
    byte s >> 3): the u8 form of the panel never exists."""
    N.require_gpu(af)
    ld_bits = ld_bits or max(256, ((n_sites + 255) // 256) * 256) // 8
    bits = torch.empty(n_ref, ld_bits, device=af.device, dtype=torch.uint8)
    check(N.lib().snvrag_panel_synth_bits(ptr(bits), row0, n_ref, ld_bits, n_sites, ptr(_c(af)), seed, stream_ptr()),
          "panel_synth_bits")
    return bits


def panel_pack_bits(codes: torch.Tensor) -> torch.Tensor:
    """u8 0/1 codes [n, ld] on the device -> bits u8 [n, ld / 8] (numpy.packbits(bitorder="little")
    of each row)."""
    N.require_gpu(codes)
    assert codes.dtype == torch.uint8 and codes.dim() == 2 and codes.shape[1] % 16 == 0
    n, ld = codes.shape
    bits = torch.empty(n, ld // 8, device=codes.device, dtype=torch.uint8)
    check(N.lib().snvrag_panel_pack_bits(ptr(_c(codes)), n, ld, ptr(bits), ld // 8, stream_ptr()), "panel_pack_bits")
    return bits


def panel_unpack_rows(bits: torch.Tensor, rows: torch.Tensor, ld_out: Optional[int] = None) -> torch.Tensor:
    """u8 [len(rows), ld_out] 0/1 codes of the bit rows ``rows`` (int64, local row numbers); rows
    outside [0, n_ref) come out zero.  ld_out defaults to the 8 * ld_bits sites of a bit row."""
    N.require_gpu(bits, rows)
    assert bits.dtype == torch.uint8 and bits.dim() == 2 and rows.dtype == torch.int64 and rows.dim() == 1
    n_ref, ldb = bits.shape
    ld_out = ld_out or 8 * ldb
    out = torch.empty(rows.numel(), ld_out, device=bits.device, dtype=torch.uint8)
    check(N.lib().snvrag_panel_unpack_rows(ptr(_c(bits)), n_ref, ldb, ptr(_c(rows)), rows.numel(), ptr(out), ld_out,
                                           stream_ptr()), "panel_unpack_rows")
    return out


def encoder_forward(x: torch.Tensor, layers: Sequence["N.LayerW"], heads: int, ws: torch.Tensor) -> torch.Tensor:
    nseq, L, D = x.shape
    arr = (N.LayerW * len(layers))(*layers)
    check(N.lib().snvrag_encoder_forward(_dt(x.dtype), nseq, L, D, heads, len(layers), arr, ptr(_c(x)),
                                         ptr(ws), ws.numel(), stream_ptr()), "encoder_forward")
    return x


def encoder_ws_bytes(dtype: torch.dtype, nseq: int, L: int, D: int, heads: int) -> int:
    return int(N.lib().snvrag_encoder_ws_bytes(_dt(dtype), nseq, L, D, heads))


def selftest_mfma() -> int:
    return int(N.lib().snvrag_selftest_mfma(stream_ptr()))


def set_option(name: str, value: int) -> int:
    """Set a library option (snvrag_set_option: test hooks / micro-benchmark switches, see
    include/snvrag.h); returns the previous value."""
    import ctypes
    prev = ctypes.c_int64()
    check(N.lib().snvrag_get_option(name.encode(), ctypes.byref(prev)), "get_option")
    check(N.lib().snvrag_set_option(name.encode(), int(value)), "set_option")
    return int(prev.value)


@contextlib.contextmanager
def option(name: str, value: int):
    """``with option("knn_no_reduce", 1): ...`` — the previous value restored afterwards."""
    prev = set_option(name, value)
    try:
        yield
    finally:
        set_option(name, prev)


# --------------------------------------------------- deterministic mode --
# Library option ``deterministic`` (default 0): linear_dw, linear_dw_parts, nbr_mean_drop_bwd and
# focal_loss call the fixed-order ``*_det`` entry points, whose partials go to one cached
# workspace per (device, stream) — launches of one stream run one after the other and reuse it, two
# streams never share one.  With the option off nothing here is touched.
_det_ws: dict = {}


def deterministic() -> bool:
    v = C.c_int64()
    check(N.lib().snvrag_get_option(b"deterministic", C.byref(v)), "get_option")
    return bool(v.value)


def _det_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), stream_ptr())
    ws = _det_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _det_ws[key] = torch.empty(max(int(nbytes), 16), device=dev, dtype=torch.uint8)
    return ws


# ---------------------------------------------------------------- training --
def attention_train_fwd(qkv: torch.Tensor, nseq: int, L: int, heads: int, dh: int, dropout_p: float = 0.0,
                        seed: int = 0):
    """bf16 attention forward that also returns lse [nseq, heads, L] (log2 domain) for the backward;
    ``dropout_p`` > 0: attention-probability dropout with the counter-based mask of ``seed``."""
    N.require_gpu(qkv)
    assert qkv.dtype == torch.bfloat16
    D = heads * dh
    out = torch.empty(nseq * L, D, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(nseq, heads, L, device=qkv.device, dtype=torch.float32)
    check(N.lib().snvrag_attention_train_fwd(nseq, L, heads, dh, ptr(_c(qkv)), qkv.shape[-1], ptr(out), D,
                                             ptr(lse), 1.0 / float(dh) ** 0.5, float(dropout_p), int(seed) & (2 ** 64 - 1),
                                             stream_ptr()), "attention_train_fwd")
    return out, lse


def attention_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, nseq: int, L: int,
                  heads: int, dh: int, dropout_p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """d(qkv) [nseq*L, 3D] bf16 of the unmasked softmax attention (csrc/attention_train.hip)."""
    N.require_gpu(qkv, out, dout, lse)
    D = heads * dh
    dqkv = torch.empty(nseq * L, 3 * D, device=qkv.device, dtype=torch.bfloat16)
    ws = torch.empty(nseq * heads * L, device=qkv.device, dtype=torch.float32)
    check(N.lib().snvrag_attention_bwd(nseq, L, heads, dh, ptr(_c(qkv)), qkv.shape[-1], ptr(_c(out)), out.shape[-1],
                                       ptr(_c(dout)), dout.shape[-1], ptr(_c(lse)), ptr(ws), ptr(dqkv), 3 * D,
                                       1.0 / float(dh) ** 0.5, float(dropout_p), int(seed) & (2 ** 64 - 1),
                                       stream_ptr()), "attention_bwd")
    return dqkv


def focal_loss(probs: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor, gamma: float, weight: float,
               loss_acc: Optional[torch.Tensor] = None):
    """(loss_sum [1] f32 (accumulated into loss_acc when given), d(weight*loss)/dprobs)."""
    N.require_gpu(probs)
    Cc = probs.shape[-1]
    M = probs.numel() // Cc
    p = _c(probs.float().contiguous())
    lab = labels.reshape(-1).long().contiguous()
    msk = mask.reshape(-1).to(torch.uint8).contiguous()
    if loss_acc is None:
        loss_acc = torch.zeros(1, device=probs.device, dtype=torch.float32)
    grad = torch.empty_like(p)
    if deterministic():
        nb = int(N.lib().snvrag_focal_loss_det_ws_bytes(M))
        ws = _det_workspace(p.device, nb)
        check(N.lib().snvrag_focal_loss_det(M, Cc, ptr(p), ptr(lab), ptr(msk), float(gamma), float(weight),
                                            ptr(loss_acc), ptr(grad), ptr(ws), ws.numel(), stream_ptr()),
              "focal_loss_det")
        return loss_acc, grad
    check(N.lib().snvrag_focal_loss(M, Cc, ptr(p), ptr(lab), ptr(msk), float(gamma), float(weight), ptr(loss_acc),
                                    ptr(grad), stream_ptr()), "focal_loss")
    return loss_acc, grad


def sqnorm(x: torch.Tensor, acc: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum x^2 (f32, fixed reduction order) into acc [1]; the per-block partials go to ``ws`` (a
    caller-owned f32 buffer of snvrag_sqnorm_ws_bytes(), allocated here when not given) — never
    shared between calls on different streams."""
    N.require_gpu(x)
    assert x.dtype == torch.float32
    if acc is None:
        acc = torch.empty(1, device=x.device, dtype=torch.float32)
    nb = int(N.lib().snvrag_sqnorm_ws_bytes())
    if ws is None or ws.numel() * ws.element_size() < nb:
        ws = torch.empty(nb // 4, device=x.device, dtype=torch.float32)
    check(N.lib().snvrag_sqnorm_ws(x.numel(), ptr(_c(x)), ptr(acc), ptr(ws), ws.numel() * ws.element_size(),
                                   stream_ptr()), "sqnorm")
    return acc


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, betas=(0.9, 0.999),
              eps: float = 1e-8, weight_decay: float = 0.0, step: int, grad_scale: float = 1.0,
              max_norm: float = 0.0, sq: Optional[torch.Tensor] = None, p_bf16: Optional[torch.Tensor] = None):
    N.require_gpu(p, g, m, v)
    a = N.AdamS(lr, betas[0], betas[1], eps, weight_decay, grad_scale, max_norm, step)
    check(N.lib().snvrag_adam_step(p.numel(), ptr(_c(p)), ptr(_c(g)), ptr(_c(m)), ptr(_c(v)), ptr(p_bf16), ptr(sq),
                                   C.byref(a), stream_ptr()), "adam_step")


def confusion(probs: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor, counts: torch.Tensor,
              mask2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts int64 [3, C] (tp, fp, fn) += cal_pr over the masked rows, on the device."""
    N.require_gpu(probs)
    Cc = probs.shape[-1]
    M = probs.numel() // Cc
    p = probs.float().contiguous()
    m2 = mask2.reshape(-1).to(torch.uint8).contiguous() if mask2 is not None else None
    check(N.lib().snvrag_confusion(M, Cc, ptr(p), ptr(labels.reshape(-1).long().contiguous()),
                                   ptr(mask.reshape(-1).to(torch.uint8).contiguous()), ptr(m2), ptr(_c(counts)),
                                   stream_ptr()), "confusion")
    return counts


def infer_post(probs_h1: torch.Tensor, probs_h2: torch.Tensor):
    """(p1, p2 [...], gt [..., 4]) of infer_embedding_rag.py:145-152 (second softmax included)."""
    N.require_gpu(probs_h1, probs_h2)
    a, b = probs_h1.float().contiguous(), probs_h2.float().contiguous()
    M = a.numel() // 2
    p1 = torch.empty(a.shape[:-1], device=a.device, dtype=torch.float32)
    p2 = torch.empty_like(p1)
    gt = torch.empty(*a.shape[:-1], 4, device=a.device, dtype=torch.float32)
    check(N.lib().snvrag_infer_post(M, ptr(a), ptr(b), ptr(p1), ptr(p2), ptr(gt), stream_ptr()), "infer_post")
    return p1, p2, gt


def _rows_host(rows_host: torch.Tensor, B: int) -> int:
    assert not rows_host.is_cuda and rows_host.dtype == torch.int32 and rows_host.is_contiguous() and \
        rows_host.numel() >= 3 * B
    return int(rows_host.data_ptr())


def infer_scatter(probs_h1: torch.Tensor, probs_h2: torch.Tensor, mask: torch.Tensor, rows_dev: torch.Tensor,
                  rows_host: torch.Tensor, window_len: int, hap1: torch.Tensor, hap2: torch.Tensor, gp: torch.Tensor,
                  mask_out: torch.Tensor) -> None:
    """``infer_post`` of one batch written straight into the site-major result arrays of
    infer_embedding_rag.geometry: hap1 / hap2 f32 [n_variants, S], gp f32 [n_variants, S, 4], mask_out
    i64 [n_variants, S] (zeroed once by the caller).  ``rows_dev`` / ``rows_host``: the batch's int32
    [3, B] row table (sample, window, flags) on the device and on the host."""
    N.require_gpu(probs_h1, probs_h2, mask, rows_dev, hap1, hap2, gp, mask_out)
    B, L = mask.shape
    assert probs_h1.shape == (B, L, 2) and probs_h2.shape == (B, L, 2) and mask.dtype == torch.int64
    assert probs_h1.dtype == torch.float32 and probs_h2.dtype == torch.float32
    assert rows_dev.dtype == torch.int32 and rows_dev.numel() >= 3 * B
    n_variants, S = hap1.shape
    assert hap2.shape == (n_variants, S) and gp.shape == (n_variants, S, 4) and mask_out.shape == (n_variants, S)
    assert hap1.dtype == hap2.dtype == gp.dtype == torch.float32 and mask_out.dtype == torch.int64
    check(N.lib().snvrag_infer_scatter(B, L, ptr(_c(probs_h1)), ptr(_c(probs_h2)), ptr(_c(mask)), ptr(_c(rows_dev)),
                                       _rows_host(rows_host, B), window_len, n_variants, S, ptr(_c(hap1)),
                                       ptr(_c(hap2)), ptr(_c(gp)), ptr(_c(mask_out)), stream_ptr()), "infer_scatter")


def batch_features(tables: "N.FeatureTables", rows_dev: torch.Tensor, rows_host: torch.Tensor, B: int, L: int,
                   token_ids: Sequence[int], labels: bool = False):
    """One launch builds a batch from the device-resident tables (``dataset.device_features``):
    returns tokens i64 [2B, L] (hap_1 rows, then hap_2 rows), mask i64 [B, L], floats f32 [6, B, L]
    (pos, af, af_p, ref, het, hom) and labels i64 [3, B, L] (hap_1_label, hap_2_label, gt_label) or
    None.  ``rows_dev`` / ``rows_host``: int32 [3, B] (sample, window, flags) on the device and on the
    host; ``token_ids`` = (sos, eos, pad, mask, tok0, tok1)."""
    N.require_gpu(rows_dev)
    assert rows_dev.dtype == torch.int32 and rows_dev.is_contiguous() and rows_dev.numel() >= 3 * B
    dev = rows_dev.device
    tokens = torch.empty(2 * B, L, device=dev, dtype=torch.int64)
    mask = torch.empty(B, L, device=dev, dtype=torch.int64)
    floats = torch.empty(6, B, L, device=dev, dtype=torch.float32)
    lab = torch.empty(3, B, L, device=dev, dtype=torch.int64) if labels else None
    sos, eos, pad, msk, tok0, tok1 = (int(v) for v in token_ids)
    check(N.lib().snvrag_batch_features(C.byref(tables), ptr(rows_dev), _rows_host(rows_host, B), B, L, sos, eos, pad,
                                        msk, tok0, tok1, ptr(tokens), ptr(mask), ptr(floats), ptr(lab), stream_ptr()),
          "batch_features")
    return tokens, mask, floats, lab


def vcf_format(h1: torch.Tensor, h2: torch.Tensor, gt: torch.Tensor, rows: torch.Tensor, line_off: torch.Tensor,
               prefix_off: torch.Tensor, prefix_blob: torch.Tensor, out: torch.Tensor, out_bytes: int,
               bad_count: torch.Tensor) -> None:
    """The text of one chunk of VCF records (``vcf_device.write_vcf_device``): line i = prefix i followed by
    the S cells of site row ``rows[i]`` of h1 / h2 f32 [n, S], gt f32 [n, S, 4], at ``out[line_off[i]:]``.
    rows i32 [n_lines], line_off i64 [n_lines + 1], prefix_off i32 [n_lines + 1] into prefix_blob u8; out u8
    with at least ``out_bytes`` bytes; bad_count i32 [1] += the values that do not print as d.ddd."""
    N.require_gpu(h1, h2, gt, rows, line_off, prefix_off, prefix_blob, out, bad_count)
    n, S = h1.shape
    n_lines = rows.numel()
    assert h2.shape == (n, S) and gt.shape == (n, S, 4)
    assert h1.dtype == h2.dtype == gt.dtype == torch.float32
    assert h1.is_contiguous() and h2.is_contiguous() and gt.is_contiguous()
    assert rows.dtype == torch.int32 and prefix_off.dtype == torch.int32 and line_off.dtype == torch.int64
    assert rows.is_contiguous() and line_off.is_contiguous() and prefix_off.is_contiguous()
    assert line_off.numel() == n_lines + 1 and prefix_off.numel() == n_lines + 1
    assert prefix_blob.dtype == torch.uint8 and out.dtype == torch.uint8 and bad_count.dtype == torch.int32
    assert prefix_blob.is_contiguous() and out.is_contiguous() and 0 <= out_bytes <= out.numel()
    check(N.lib().snvrag_vcf_format(n, S, ptr(h1), ptr(h2), ptr(gt), n_lines, ptr(rows), ptr(line_off),
                                    ptr(prefix_off), ptr(prefix_blob), prefix_blob.numel(), ptr(out), out_bytes,
                                    ptr(bad_count), stream_ptr()), "vcf_format")


def site_stats(h1: torch.Tensor, h2: torch.Tensor, gt: torch.Tensor, truth: Optional[torch.Tensor] = None,
               truth_row: Optional[torch.Tensor] = None, truth_col: Optional[torch.Tensor] = None,
               bad_count: Optional[torch.Tensor] = None):
    """(est f64 [n, 5], acc f64 [n, 3], table i32 [n, 9]) of the site-major result arrays h1 / h2 f32 [n, S],
    gt f32 [n, S, 4] (``quality.site_stats_host`` is the specification; include/snvrag.h lists the sums).
    ``truth`` i8 [n_truth, S_truth, 2] with ``truth_row`` i32 [n] and ``truth_col`` i32 [S] (-1: none); without
    it only ``est`` is computed and acc / table are None.  ``bad_count`` i32 [1] += the indices out of range
    (allocated and zeroed here when not given; ``quality.site_stats`` reads it)."""
    N.require_gpu(h1, h2, gt, truth, truth_row, truth_col, bad_count)
    n, S = h1.shape
    assert h2.shape == (n, S) and gt.shape == (n, S, 4)
    assert h1.dtype == h2.dtype == gt.dtype == torch.float32
    assert h1.is_contiguous() and h2.is_contiguous() and gt.is_contiguous()
    dev = h1.device
    est = torch.empty(n, 5, device=dev, dtype=torch.float64)
    acc = table = None
    n_truth = S_truth = 0
    if truth is not None:
        assert truth_row is not None and truth_col is not None, "truth needs truth_row and truth_col"
        assert truth.dtype == torch.int8 and truth.dim() == 3 and truth.shape[2] == 2 and truth.is_contiguous()
        assert truth_row.dtype == truth_col.dtype == torch.int32
        assert truth_row.is_contiguous() and truth_col.is_contiguous()
        assert truth_row.numel() == n and truth_col.numel() == S
        n_truth, S_truth = truth.shape[:2]
        acc = torch.empty(n, 3, device=dev, dtype=torch.float64)
        table = torch.empty(n, 9, device=dev, dtype=torch.int32)
        if bad_count is None:
            bad_count = torch.zeros(1, device=dev, dtype=torch.int32)
        assert bad_count.dtype == torch.int32 and bad_count.numel() >= 1
    check(N.lib().snvrag_site_stats(n, S, ptr(h1), ptr(h2), ptr(gt), ptr(truth), n_truth, S_truth, ptr(truth_row),
                                    ptr(truth_col), ptr(est), ptr(acc), ptr(table), ptr(bad_count), stream_ptr()),
          "site_stats")
    return est, acc, table


def _text_ok(text: torch.Tensor, nbytes: int) -> None:
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous()
    assert 1 <= nbytes and (nbytes + 15) // 16 * 16 <= text.numel(), "the text buffer must hold the '\\n' padding"


def vcf_line_index(text: torch.Tensor, nbytes: int, max_lines: int):
    """(line_off i64 [max_lines + 1], n_lines i64 [1], both on the device) of the text chunk ``text[:nbytes]``
    (u8, starts at a line start, padded with '\\n' to a multiple of 16 bytes): the sorted offsets of the
    lines of non-zero length, then ``nbytes``.  ``n_lines`` may exceed ``max_lines`` (offsets past it
    are dropped): the caller checks."""
    N.require_gpu(text)
    _text_ok(text, nbytes)
    dev = text.device
    line_off = torch.empty(max_lines + 1, device=dev, dtype=torch.int64)
    n_lines = torch.empty(1, device=dev, dtype=torch.int64)
    nws = N.lib().snvrag_vcf_line_index_ws_bytes(nbytes)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    check(N.lib().snvrag_vcf_line_index(ptr(text), nbytes, max_lines, ptr(line_off), ptr(n_lines), ptr(ws), nws,
                                        stream_ptr()), "vcf_line_index")
    return line_off, n_lines


def vcf_parse_gt(text: torch.Tensor, nbytes: int, line_off: torch.Tensor, n_lines: int, S: int, codes: torch.Tensor,
                 force_general: bool = False):
    """Parse lines ``line_off[:n_lines]`` of the chunk: returns (pos i32 [n_lines], flags u32-in-i32
    [n_lines]) and fills rows [0, n_lines) of ``codes`` u8 [>= n_lines, ld_codes] (one byte per sample;
    include/snvrag.h lists the flag and code bits).  ``force_general``: every line on the general path."""
    N.require_gpu(text, line_off, codes)
    _text_ok(text, nbytes)
    assert line_off.dtype == torch.int64 and line_off.is_contiguous() and line_off.numel() >= n_lines
    assert codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous()
    assert codes.shape[0] >= n_lines and codes.shape[1] >= S and codes.shape[1] % 4 == 0
    dev = text.device
    pos = torch.empty(n_lines, device=dev, dtype=torch.int32)
    flags = torch.empty(n_lines, device=dev, dtype=torch.int32)
    nws = N.lib().snvrag_vcf_parse_ws_bytes(n_lines, S)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    check(N.lib().snvrag_vcf_parse_gt(ptr(text), nbytes, ptr(line_off), n_lines, S, int(bool(force_general)), ptr(pos),
                                      ptr(flags), ptr(codes), codes.shape[1], ptr(ws), nws, stream_ptr()),
          "vcf_parse_gt")
    return pos, flags


def vcf_pack_rows(codes: torch.Tensor, n_lines: int, S: int, alt_bits: torch.Tensor, miss_bits: torch.Tensor,
                  site0: int = 0) -> None:
    """Rows [0, n_lines) of ``codes`` (records) -> sites [site0, site0 + n_lines) of ``alt_bits`` /
    ``miss_bits`` u8 [2 S, ld_bits] (haplotype h of sample s = row 2 s + h, site r = bit r & 7 of byte
    r >> 3).  site0 % 64 == 0, ld_bits % 8 == 0."""
    N.require_gpu(codes, alt_bits, miss_bits)
    assert codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous() and codes.shape[0] >= n_lines
    for b in (alt_bits, miss_bits):
        assert b.dtype == torch.uint8 and b.is_contiguous() and b.shape == (2 * S, alt_bits.shape[1])
    check(N.lib().snvrag_vcf_pack_rows(ptr(codes), codes.shape[1], n_lines, S, site0, ptr(alt_bits), ptr(miss_bits),
                                       alt_bits.shape[1], stream_ptr()), "vcf_pack_rows")


def panel_gather_bits(bits: torch.Tensor, n_src_sites: int, site_idx: torch.Tensor, n_sites_pad: int,
                      packed: bool) -> torch.Tensor:
    """Sites ``site_idx`` (i32 [n]; -1 gives 0) of the bit rows ``bits`` u8 [N, ld_bits] as one window's index
    rows: u8 [N, n_sites_pad / 8] bits (``packed``) or u8 [N, n_sites_pad] 0/1 codes; padding sites 0."""
    N.require_gpu(bits, site_idx)
    assert bits.dtype == torch.uint8 and bits.dim() == 2 and bits.is_contiguous()
    assert site_idx.dtype == torch.int32 and site_idx.dim() == 1 and site_idx.is_contiguous()
    out = torch.empty(bits.shape[0], n_sites_pad // 8 if packed else n_sites_pad, device=bits.device,
                      dtype=torch.uint8)
    check(N.lib().snvrag_panel_gather_bits(ptr(bits), bits.shape[0], bits.shape[1], n_src_sites, ptr(site_idx),
                                           site_idx.numel(), n_sites_pad, int(bool(packed)), ptr(out), stream_ptr()),
          "panel_gather_bits")
    return out


def vcf_unpack_gt(alt_bits: torch.Tensor, miss_bits: torch.Tensor, n_sites: int) -> torch.Tensor:
    """i8 [n_sites, S, 2] on the device: 0 / 1 from ``alt_bits``, -1 where ``miss_bits`` is set."""
    N.require_gpu(alt_bits, miss_bits)
    assert alt_bits.dtype == miss_bits.dtype == torch.uint8 and alt_bits.shape == miss_bits.shape
    assert alt_bits.dim() == 2 and alt_bits.is_contiguous() and miss_bits.is_contiguous() and alt_bits.shape[0] % 2 == 0
    S = alt_bits.shape[0] // 2
    gt = torch.empty(n_sites, S, 2, device=alt_bits.device, dtype=torch.int8)
    check(N.lib().snvrag_vcf_unpack_gt(ptr(alt_bits), ptr(miss_bits), alt_bits.shape[1], S, n_sites, ptr(gt),
                                       stream_ptr()), "vcf_unpack_gt")
    return gt


def vcf_cols_span(text: torch.Tensor, nbytes: int, line_off: torch.Tensor, n_lines: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spans i32 [n_lines, 8]: (start, length) in ``text`` of CHROM, ID, REF and ALT of the lines
    ``line_off[:n_lines]`` of the chunk (``dataset/vcf_reader.py`` record_columns is the specification; a
    column the line does not reach has length 0)."""
    N.require_gpu(text, line_off)
    _text_ok(text, nbytes)
    assert line_off.dtype == torch.int64 and line_off.is_contiguous() and line_off.numel() >= n_lines
    if out is None:
        out = torch.empty(n_lines, 8, device=text.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (n_lines, 8)
    check(N.lib().snvrag_vcf_cols_span(ptr(text), nbytes, ptr(line_off), n_lines, ptr(out), stream_ptr()),
          "vcf_cols_span")
    return out


def vcf_cols_gather(text: torch.Tensor, nbytes: int, spans: torch.Tensor, off: torch.Tensor,
                    blob: torch.Tensor) -> None:
    """The strings of ``spans`` i32 [n, 8] packed into ``blob`` u8: item c * n + r (column c of record r) at
    ``blob[off[i]:off[i + 1]]``, ``off`` i64 [4 n + 1] the exclusive prefix sum of the lengths in that order.
    An item that does not fit its range or the blob is not copied."""
    N.require_gpu(text, spans, off, blob)
    _text_ok(text, nbytes)
    n = spans.shape[0]
    assert spans.dtype == torch.int32 and spans.is_contiguous() and spans.shape == (n, 8)
    assert off.dtype == torch.int64 and off.is_contiguous() and off.numel() == 4 * n + 1
    assert blob.dtype == torch.uint8 and blob.dim() == 1 and blob.is_contiguous()
    check(N.lib().snvrag_vcf_cols_gather(ptr(text), nbytes, ptr(spans), n, ptr(off), ptr(blob), blob.numel(),
                                         stream_ptr()), "vcf_cols_gather")


def panel_counts(alt_bits: torch.Tensor, miss_bits: torch.Tensor, n_sites: int, order: torch.Tensor,
                 pop_start: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Genotype counts i32 [6, 5, n_sites] of the bit rows ``alt_bits`` / ``miss_bits`` u8 [2 S, >= ceil(n_sites / 8)]
    (``VcfGenotypes`` layout; rows may be views: any row stride that holds the sites, any byte alignment) per
    population: ``order`` i32 [S] the samples sorted by population, ``pop_start`` i32 [P + 1], 1 <= P <= 5.
    Row p < P is population p, rows P..4 are zero, row 5 the whole panel; columns n_ref, n_het, n_hom, n_alt,
    n_called (``dataset/panel_stats.py`` panel_counts_host is the specification).  Every element of the result
    is written (``out``: a contiguous i32 [6, 5, n_sites] to write into)."""
    N.require_gpu(alt_bits, miss_bits, order, pop_start)
    nb = (n_sites + 7) // 8
    for b in (alt_bits, miss_bits):
        assert b.dtype == torch.uint8 and b.dim() == 2 and b.shape[0] == alt_bits.shape[0] and b.shape[1] >= nb
        assert b.shape[1] <= 1 or b.stride(1) == 1
    S = alt_bits.shape[0] // 2
    assert alt_bits.shape[0] == 2 * S and S >= 1
    ld = alt_bits.stride(0) if alt_bits.shape[0] > 1 else max(alt_bits.shape[1], nb)
    assert all(b.shape[0] <= 1 or b.stride(0) == ld for b in (alt_bits, miss_bits)) and ld >= nb
    assert order.dtype == pop_start.dtype == torch.int32 and order.is_contiguous() and pop_start.is_contiguous()
    assert order.numel() == S and pop_start.numel() >= 2
    if out is None:
        out = torch.empty(6, 5, n_sites, device=alt_bits.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (6, 5, n_sites)
    check(N.lib().snvrag_panel_counts(ptr(alt_bits), ptr(miss_bits), ld, S, n_sites, ptr(order), ptr(pop_start),
                                      pop_start.numel() - 1, ptr(out), stream_ptr()), "panel_counts")
    return out


def typed_overlay(h1: torch.Tensor, h2: torch.Tensor, gt: torch.Tensor, alt_bits: torch.Tensor,
                  miss_bits: torch.Tensor, n_target: int, site_row: torch.Tensor, col: torch.Tensor,
                  missing: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The target's observed genotypes written over the site-major result arrays h1 / h2 f32 [n, S], gt f32
    [n, S, 4] in place (``typed_sites.typed_overlay_host`` is the specification; include/snvrag.h states the
    rule).  ``alt_bits`` / ``miss_bits`` u8 [2 S_target, ld_bits] hold ``n_target`` records (rows may be views
    of one row stride); ``site_row`` i32 [n] is the target record of each site row, ``col`` i32 [S] the target
    sample of each column (-1 or out of range: untouched).  Returns ``missing`` i32 [n]: per site row, the mapped
    cells left as they were because a call is missing (``missing``: a contiguous i32 [n] to write into)."""
    N.require_gpu(h1, h2, gt, alt_bits, miss_bits, site_row, col, missing)
    n, S = h1.shape
    assert h2.shape == (n, S) and gt.shape == (n, S, 4)
    assert h1.dtype == h2.dtype == gt.dtype == torch.float32
    assert h1.is_contiguous() and h2.is_contiguous() and gt.is_contiguous()
    nb = (n_target + 7) // 8
    for b in (alt_bits, miss_bits):
        assert b.dtype == torch.uint8 and b.dim() == 2 and b.shape[0] == alt_bits.shape[0] and b.shape[1] >= nb
        assert b.shape[1] <= 1 or b.stride(1) == 1
    S_target = alt_bits.shape[0] // 2
    assert alt_bits.shape[0] == 2 * S_target and S_target >= 1
    ld = alt_bits.stride(0) if alt_bits.shape[0] > 1 else max(alt_bits.shape[1], nb)
    assert all(b.shape[0] <= 1 or b.stride(0) == ld for b in (alt_bits, miss_bits)) and ld >= nb
    assert site_row.dtype == col.dtype == torch.int32 and site_row.is_contiguous() and col.is_contiguous()
    assert site_row.numel() == n and col.numel() == S
    if missing is None:
        missing = torch.empty(n, device=h1.device, dtype=torch.int32)
    assert missing.dtype == torch.int32 and missing.is_contiguous() and missing.numel() == n
    if n == 0:                                     # empty tensors have no address to pass
        return missing
    check(N.lib().snvrag_typed_overlay(ptr(alt_bits), ptr(miss_bits), ld, n_target, S_target, ptr(site_row), ptr(col),
                                       n, S, ptr(h1), ptr(h2), ptr(gt), ptr(missing), stream_ptr()), "typed_overlay")
    return missing


def bgzf_table(in_off, out_off, in_len, isize, crc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The block table of ``bgzf_inflate`` from five sequences: host i64 [n, 4] = in_off, out_off,
    in_len | isize << 32, crc (into the first rows of ``out`` when given, e.g. a pinned buffer)."""
    import numpy as np
    n = len(in_off)
    t = np.empty((n, 4), np.int64)
    t[:, 0], t[:, 1] = in_off, out_off
    t[:, 2] = np.asarray(in_len, np.int64) & 0xffffffff | np.asarray(isize, np.int64) << 32
    t[:, 3] = np.asarray(crc, np.int64) & 0xffffffff
    if out is None:
        return torch.from_numpy(t)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.shape[0] >= n and out.shape[1:] == (4,)
    out.numpy()[:n] = t
    return out[:n]


def bgzf_inflate(comp: torch.Tensor, table: torch.Tensor, text: torch.Tensor, status: Optional[torch.Tensor] = None,
                 table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inflate the BGZF blocks of ``table`` (host i64 [n, 4], ``bgzf_table``) from ``comp`` (device u8) into
    ``text`` (device u8) at their ``out_off``; returns status i32 [n] on the device (src/dataset/bgzf.py lists the
    codes; a block is written only with status 0 or 9).  A pinned ``table`` must stay unchanged until the
    stream has passed this call."""
    N.require_gpu(comp, text)
    assert comp.dtype == torch.uint8 and comp.dim() == 1 and comp.is_contiguous()
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous()
    assert table.device.type == "cpu" and table.dtype == torch.int64 and table.is_contiguous()
    assert table.dim() == 2 and table.shape[1] == 4
    n = table.shape[0]
    dev = text.device
    if status is None:
        status = torch.empty(n, device=dev, dtype=torch.int32)
    if table_dev is None:
        table_dev = torch.empty(n, 4, device=dev, dtype=torch.int64)
    assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() >= n
    assert table_dev.dtype == torch.int64 and table_dev.is_contiguous() and table_dev.numel() >= 4 * n
    check(N.lib().snvrag_bgzf_inflate(ptr(comp), comp.numel(), ptr(table), ptr(table_dev), n, ptr(text), text.numel(),
                                      ptr(status), stream_ptr()), "bgzf_inflate")
    return status[:n]


def text_last_newline(text: torch.Tensor, nbytes: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device i64 [1]: the index of the last '\\n' in ``text[:nbytes]`` (u8, 16-byte aligned), or -1."""
    N.require_gpu(text)
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous() and 0 <= nbytes <= text.numel()
    if out is None:
        out = torch.empty(1, device=text.device, dtype=torch.int64)
    assert out.dtype == torch.int64 and out.numel() >= 1
    check(N.lib().snvrag_text_last_newline(ptr(text), nbytes, ptr(out), stream_ptr()), "text_last_newline")
    return out


BGZF_SLOT = 65536                    # bytes between two members of ``bgzf_deflate``


def bgzf_deflate(text: torch.Tensor, nbytes: int, block_size: int = 0xff00, members: Optional[torch.Tensor] = None,
                 member_len: Optional[torch.Tensor] = None):
    """``text[:nbytes]`` (device u8, any alignment) cut into pieces of ``block_size`` bytes, each deflated into
    one BGZF member: returns (members u8 [n_blocks, 65536], member_len i32 [n_blocks]) on the device; member b
    is ``members[b, :member_len[b]]`` and the rest of its slot is not touched."""
    N.require_gpu(text)
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous()
    if not 0 <= nbytes <= text.numel() or nbytes >= 1 << 31:
        raise ValueError(f"bgzf_deflate: nbytes {nbytes} must lie in [0, min(text bytes, 2^31))")
    if not 1 <= block_size <= 0xff00:
        raise ValueError(f"bgzf_deflate: block_size {block_size} must lie in [1, 0xff00]")
    n = -(-nbytes // block_size)
    dev = text.device
    if members is None:
        members = torch.empty(n, BGZF_SLOT, device=dev, dtype=torch.uint8)
    if member_len is None:
        member_len = torch.empty(n, device=dev, dtype=torch.int32)
    assert members.dtype == torch.uint8 and members.is_contiguous() and members.numel() >= n * BGZF_SLOT
    assert member_len.dtype == torch.int32 and member_len.is_contiguous() and member_len.numel() >= n
    if members.data_ptr() % 16:
        raise ValueError("bgzf_deflate: members must be 16-byte aligned")
    if n:
        check(N.lib().snvrag_bgzf_deflate(ptr(text), nbytes, block_size, ptr(members), ptr(member_len), stream_ptr()),
              "bgzf_deflate")
    return members.view(-1)[:n * BGZF_SLOT].view(n, BGZF_SLOT), member_len[:n]


def bgzf_pack(members: torch.Tensor, member_len: torch.Tensor, out: torch.Tensor,
              total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The members of ``bgzf_deflate`` copied back to back into ``out`` (device u8); returns total i64 [1] on the
    device: the bytes written, or -1 (and nothing written) where they do not fit ``out``."""
    N.require_gpu(members, member_len, out)
    assert members.dtype == torch.uint8 and members.is_contiguous() and out.dtype == torch.uint8 and out.is_contiguous()
    assert member_len.dtype == torch.int32 and member_len.dim() == 1 and member_len.is_contiguous()
    n = member_len.numel()
    assert members.numel() >= n * BGZF_SLOT
    if members.data_ptr() % 16:
        raise ValueError("bgzf_pack: members must be 16-byte aligned")
    if total is None:
        total = torch.empty(1, device=out.device, dtype=torch.int64)
    assert total.dtype == torch.int64 and total.numel() >= 1 and total.data_ptr() % 8 == 0
    check(N.lib().snvrag_bgzf_pack(ptr(members), ptr(member_len), n, ptr(out), out.numel(), ptr(total), stream_ptr()),
          "bgzf_pack")
    return total


def ln_fwd_train(x: torch.Tensor, r: Optional[torch.Tensor], g: torch.Tensor, b: torch.Tensor, eps: float,
                 p_r: float = 0.0, p_out: float = 0.0, seed: int = 0, slope_x: float = 0.0, slope_r: float = 0.0):
    """(y bf16, s bf16 = act_x(x) + drop(act_r(r)) (x itself when r is None), stats f32 [M, 2]); y
    carries the output dropout p_out (masks: counter-based hash of seed, row, column).  slope_x /
    slope_r: LeakyReLU on x (no residual; s is then the pre-activation x) / on r before its dropout."""
    N.require_gpu(x)
    Nn = x.shape[-1]
    M = x.numel() // Nn
    y = torch.empty_like(x)
    s = torch.empty_like(x) if r is not None else x
    stats = torch.empty(M, 2, device=x.device, dtype=torch.float32)
    check(N.lib().snvrag_ln_fwd_train_act(M, Nn, ptr(_c(x)), ptr(_c(r)) if r is not None else None,
                                          ptr(_c(g)), ptr(_c(b)), eps, ptr(y), ptr(s) if r is not None else None,
                                          ptr(stats), float(p_r), float(p_out), int(seed) & (2 ** 64 - 1),
                                          float(slope_x), float(slope_r), stream_ptr()), "ln_fwd_train")
    return y, s, stats


def ln_bwd(dy: torch.Tensor, s: torch.Tensor, stats: torch.Tensor, g: torch.Tensor, p_r: float = 0.0,
           p_out: float = 0.0, seed: int = 0, dg: Optional[torch.Tensor] = None,
           db: Optional[torch.Tensor] = None, slope_x: float = 0.0, slope_r: float = 0.0,
           r_pre: Optional[torch.Tensor] = None):
    """(ds bf16, dres bf16 or None, dg f32 [N], db f32 [N]) of y = drop_o(LN(s) g + b),
    s = x + drop_r(r): ds = dx, dres = dr (None when p_r == 0 and no residual activation: dr =
    ds).  dg / db given (f32, contiguous: the parameters' .grad) are accumulated into, else fresh.
    slope_x: s is the pre-activation x of y = LN(lrelu(x)); slope_r: r_pre is the pre-activation
    residual (dres through the activation)."""
    Nn = s.shape[-1]
    M = s.numel() // Nn
    ds = torch.empty_like(s)
    dres = torch.empty_like(s) if (p_r > 0 or slope_r != 0.0) else None
    assert slope_r == 0.0 or r_pre is not None
    acc = dg is not None
    if dg is None:
        dg = torch.empty(Nn, device=s.device, dtype=torch.float32)
        db = torch.empty_like(dg)
    assert db is not None and dg.is_contiguous() and db.is_contiguous() and dg.dtype == db.dtype == torch.float32
    wsb = N.lib().snvrag_ln_bwd_ws_bytes(M, Nn)
    ws = torch.empty(wsb, device=s.device, dtype=torch.uint8)
    check(N.lib().snvrag_ln_bwd_act(M, Nn, ptr(_c(dy)), ptr(_c(s)), ptr(_c(stats)), ptr(_c(g)), ptr(ds), ptr(dres),
                                    ptr(_c(r_pre)) if r_pre is not None else None, ptr(dg), ptr(db), int(acc),
                                    float(p_r), float(p_out), int(seed) & (2 ** 64 - 1), float(slope_x),
                                    float(slope_r), ptr(ws), wsb, stream_ptr()), "ln_bwd")
    return ds, dres, dg, db


def nbr_mean_drop(inv: torch.Tensor, codes: torch.Tensor, n_sites: int, W: torch.Tensor, pe: torch.Tensor,
                  Ar: torch.Tensor, p: float, seed: int, tok0: int = 5, sos: int = 2, eos: int = 3,
                  pad: int = 0) -> torch.Tensor:
    """f32 [nq, L, D]: each query's mean over its valid unique neighbours inv [nq, k] (int32, < 0:
    none) of drop(W[tok] + pe + Ar), one dropout mask per unique neighbour (csrc/train.hip)."""
    N.require_gpu(inv, codes, W)
    nq, k = inv.shape
    L, D = pe.shape
    out = torch.empty(nq, L, D, device=W.device, dtype=torch.float32)
    check(N.lib().snvrag_nbr_mean_drop_fwd(nq, k, L, D, n_sites, codes.shape[1], W.shape[0], ptr(_c(inv)),
                                           ptr(_c(codes)), ptr(_c(W)), ptr(_c(pe)), ptr(_c(Ar)), float(p),
                                           int(seed) & (2 ** 64 - 1), tok0, sos, eos, pad, ptr(out), stream_ptr()),
          "nbr_mean_drop_fwd")
    return out


def nbr_mean_drop_bwd(dout: torch.Tensor, inv: torch.Tensor, codes: torch.Tensor, n_sites: int, W: torch.Tensor,
                      pe: torch.Tensor, Ar: torch.Tensor, p: float, seed: int, dW: torch.Tensor, dAr: torch.Tensor,
                      tok0: int = 5, sos: int = 2, eos: int = 3, pad: int = 0) -> None:
    """Accumulates dW [V, D] and dAr [L, D] (f32) of :func:`nbr_mean_drop` for dout [nq, L, D] f32."""
    nq, k = inv.shape
    L, D = pe.shape
    assert dW.dtype == dAr.dtype == torch.float32 and dW.is_contiguous() and dAr.is_contiguous()
    if deterministic():
        nb = int(N.lib().snvrag_nbr_mean_drop_bwd_det_ws_bytes(L, W.shape[0], D))
        ws = _det_workspace(dW.device, nb)
        check(N.lib().snvrag_nbr_mean_drop_bwd_det(nq, k, L, D, n_sites, codes.shape[1], W.shape[0], ptr(_c(inv)),
                                                   ptr(_c(codes)), ptr(_c(W)), ptr(_c(pe)), ptr(_c(Ar)), float(p),
                                                   int(seed) & (2 ** 64 - 1), tok0, sos, eos, pad,
                                                   ptr(_c(dout.float())), ptr(dW), ptr(dAr), ptr(ws), ws.numel(),
                                                   stream_ptr()), "nbr_mean_drop_bwd_det")
        return
    check(N.lib().snvrag_nbr_mean_drop_bwd(nq, k, L, D, n_sites, codes.shape[1], W.shape[0], ptr(_c(inv)),
                                           ptr(_c(codes)), ptr(_c(W)), ptr(_c(pe)), ptr(_c(Ar)), float(p),
                                           int(seed) & (2 ** 64 - 1), tok0, sos, eos, pad,
                                           ptr(_c(dout.float())), ptr(dW), ptr(dAr), stream_ptr()),
          "nbr_mean_drop_bwd")


def linear_dw(dy: torch.Tensor, x: torch.Tensor, bias: bool = False, splits: int = 0,
              dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None):
    """dW f32 [N, K] += dy^T x and (bias) db f32 [N] += column sums of dy, for bf16 dy [M, N] and
    x [M, K] whose rows may be strided (a column slice of a fused output: dy[:, a:b]); N, K
    multiples of 128 (csrc/dw.hip).  dw / db are ACCUMULATED into when given (f32, contiguous:
    e.g. a parameter's .grad), else zero-initialised.  Returns (dw, db or None)."""
    N.require_gpu(dy, x)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.shape[0] == x.shape[0]
    assert dy.stride(1) == 1 and x.stride(1) == 1
    M, Nn = dy.shape
    Kk = x.shape[1]
    if dw is None:
        dw = torch.zeros(Nn, Kk, device=dy.device, dtype=torch.float32)
    assert dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == (Nn, Kk)
    if bias and db is None:
        db = torch.zeros(Nn, device=dy.device, dtype=torch.float32)
    if db is not None:
        assert db.dtype == torch.float32 and db.is_contiguous() and db.numel() == Nn
    if deterministic():
        nb = int(N.lib().snvrag_linear_dw_det_ws_bytes(M, Nn, Kk, int(splits)))
        ws = _det_workspace(dy.device, nb)
        check(N.lib().snvrag_linear_dw_det(M, Nn, Kk, ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), ptr(db),
                                           int(splits), ptr(ws), ws.numel(), stream_ptr()), "linear_dw_det")
        return dw, db
    check(N.lib().snvrag_linear_dw(M, Nn, Kk, ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), ptr(db),
                                   int(splits), stream_ptr()), "linear_dw")
    return dw, db


def linear_dw_parts(dy: torch.Tensor, x: torch.Tensor, dws, dbs=None, splits: int = 0) -> None:
    """dws[i] f32 [N / n, K] += dy[:, i N/n : (i+1) N/n]^T x (and dbs[i] += its column sums) in ONE
    launch over the fused output (csrc/dw.hip, snvrag_linear_dw_parts): the q/k/v weights'
    gradient buffers of one N = 3D projection."""
    N.require_gpu(dy, x)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.shape[0] == x.shape[0]
    assert dy.stride(1) == 1 and x.stride(1) == 1
    M, Nn = dy.shape
    Kk = x.shape[1]
    n = len(dws)
    for t in dws:
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (Nn // n, Kk)
    if dbs is not None:
        for t in dbs:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == Nn // n
    import ctypes
    wp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dws])
    bp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dbs]) if dbs is not None else None
    if deterministic():
        nb = int(N.lib().snvrag_linear_dw_det_ws_bytes(M, Nn, Kk, int(splits)))
        ws = _det_workspace(dy.device, nb)
        check(N.lib().snvrag_linear_dw_parts_det(M, Nn, Kk, ptr(dy), dy.stride(0), ptr(x), x.stride(0), n, wp, bp,
                                                 int(splits), ptr(ws), ws.numel(), stream_ptr()),
              "linear_dw_parts_det")
        return
    check(N.lib().snvrag_linear_dw_parts(M, Nn, Kk, ptr(dy), dy.stride(0), ptr(x), x.stride(0), n, wp, bp,
                                         int(splits), stream_ptr()), "linear_dw_parts")


def colsum(x: torch.Tensor) -> torch.Tensor:
    """f32 column sums of a bf16 matrix [..., N] (bias gradients)."""
    Nn = x.shape[-1]
    M = x.numel() // Nn
    out = torch.empty(Nn, device=x.device, dtype=torch.float32)
    wsb = N.lib().snvrag_colsum_ws_bytes(M, Nn)
    ws = torch.empty(wsb, device=x.device, dtype=torch.uint8)
    check(N.lib().snvrag_colsum_bf16(M, Nn, ptr(_c(x)), ptr(out), ptr(ws), wsb, stream_ptr()), "colsum")
    return out


SG_ACT, SG_HEAD2, SG_LN = 0, 1, 2


def sgemm_pack(w: torch.Tensor) -> torch.Tensor:
    """Tile-major fragment stream of W [N, D] for the stream GEMM (csrc/sgemm.hip)."""
    N.require_gpu(w)
    Nn, D = w.shape
    nbytes = int(N.lib().snvrag_sgemm_pack_bytes(D, Nn))
    if nbytes == 0:
        raise ValueError(f"stream GEMM needs D in (128, 256, 384) and N % 64 == 0, got {tuple(w.shape)}")
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    check(N.lib().snvrag_sgemm_pack(D, Nn, ptr(_c(w.to(torch.bfloat16).contiguous())), ptr(out), stream_ptr()),
          "sgemm_pack")
    return out


def gemm256_pack(w: torch.Tensor) -> torch.Tensor:
    """Fragment stream of W [N, K] for the wide-row GEMM (csrc/gemm256.hip)."""
    N.require_gpu(w)
    Nn, Kk = w.shape
    nbytes = int(N.lib().snvrag_gemm256_pack_bytes(Nn, Kk))
    if nbytes == 0:
        raise ValueError(f"wide-row GEMM pack needs N % 128 == 0 and K % 64 == 0, got {tuple(w.shape)}")
    wb = w.to(torch.bfloat16)
    if wb.stride(1) != 1:
        wb = wb.contiguous()
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    check(N.lib().snvrag_gemm256_pack(Nn, Kk, ptr(wb), wb.stride(0), ptr(out), stream_ptr()), "gemm256_pack")
    return out


def gemm256(a: torch.Tensor, wpacked: torch.Tensor, n_out: int, bias: Optional[torch.Tensor] = None,
            resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [M, N] = a [M, K] W^T (+ bias f32 [N]) (+ resid bf16 [M, N]) on the wide-row GEMM
    (csrc/gemm256.hip; W packed by :func:`gemm256_pack` or derive kind DERIVE_G2PACK).  ``out`` may
    alias ``resid`` (each element is read before it is written, by the same lane)."""
    N.require_gpu(a)
    assert a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1
    M, Kk = a.shape
    assert wpacked.numel() * wpacked.element_size() == int(N.lib().snvrag_gemm256_pack_bytes(n_out, Kk))
    if out is None:
        out = torch.empty(M, n_out, device=a.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.shape == (M, n_out) and out.stride(1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == n_out
    if resid is not None:
        assert resid.dtype == torch.bfloat16 and resid.shape == (M, n_out) and resid.stride(1) == 1
    check(N.lib().snvrag_gemm256_forward(M, n_out, Kk, ptr(a), a.stride(0), ptr(wpacked),
                                         ptr(bias) if bias is not None else None,
                                         ptr(resid) if resid is not None else None,
                                         resid.stride(0) if resid is not None else 0, ptr(out), out.stride(0),
                                         stream_ptr()), "gemm256")
    return out


def gemm256_ln(a: torch.Tensor, wpacked: torch.Tensor, bias: Optional[torch.Tensor], ln: Tuple[torch.Tensor, torch.Tensor],
               base: Optional[torch.Tensor] = None, post_scale: float = 1.0, post_af: Optional[torch.Tensor] = None,
               post_af_period: int = 0, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [M, 384] = base + post_scale * LN(a W^T + bias) * w(post_af[m % period]) on the wide-row
    GEMM (csrc/gemm256.hip EPI 1): the rag fusion's fusion[3] -> fusion[4] -> MAF -> residual
    (fusion.py:152-162), the same arithmetic as :func:`linear` with ``ln=``, ``post_base=``,
    ``post_maf=True``."""
    N.require_gpu(a)
    assert a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1
    M, Kk = a.shape
    n_out = 384
    assert wpacked.numel() * wpacked.element_size() == int(N.lib().snvrag_gemm256_pack_bytes(n_out, Kk))
    if out is None:
        out = torch.empty(M, n_out, device=a.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.shape == (M, n_out) and out.stride(1) == 1
    for t in (bias, ln[0], ln[1]) if bias is not None else ln:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_out
    if base is not None:
        assert base.dtype == torch.bfloat16 and base.shape == (M, n_out) and base.stride(1) == 1
    if post_af is not None:
        assert post_af.dtype == torch.float32 and post_af.is_contiguous()
        assert post_af.numel() >= (post_af_period if post_af_period > 0 else M)
    check(N.lib().snvrag_gemm256_ln_forward(M, n_out, Kk, ptr(a), a.stride(0), ptr(wpacked),
                                            ptr(bias) if bias is not None else None, ptr(ln[0]), ptr(ln[1]), eps,
                                            ptr(base) if base is not None else None,
                                            base.stride(0) if base is not None else 0, post_scale,
                                            ptr(post_af) if post_af is not None else None, post_af_period,
                                            ptr(out), out.stride(0), stream_ptr()), "gemm256_ln")
    return out


DERIVE_F32, DERIVE_BF16, DERIVE_SGPACK, DERIVE_G2PACK = 0, 1, 2, 3


def derive_job(kind: int, parts, dst: torch.Tensor, dst_ld: int = 0) -> "N.DeriveJob":
    """One snvrag_derive job: ``parts`` = f32 2-D (strided) views stacked along their rows (1-D
    views count as columns [n, 1]); ``dst`` receives kind DERIVE_F32 / DERIVE_BF16 (row-major with
    row stride ``dst_ld``, default the column count), DERIVE_SGPACK (the stream-GEMM pack of the
    [N, D] matrix) or DERIVE_G2PACK (the wide-row GEMM pack of the [N, K] matrix).  piece0 / pieces are filled by ``derive_table``."""
    assert 1 <= len(parts) <= 4
    views = [t.unsqueeze(1) if t.dim() == 1 else t for t in parts]
    cols = views[0].shape[1]
    assert all(v.dim() == 2 and v.shape[1] == cols and v.dtype == torch.float32 and v.is_cuda for v in views)
    j = N.DeriveJob()
    j.kind, j.nparts = kind, len(views)
    j.rows, j.cols = sum(v.shape[0] for v in views), cols
    j.dst_ld = dst_ld or cols
    for i, v in enumerate(views):
        j.part_rows[i], j.rs[i], j.cs[i], j.src[i] = v.shape[0], v.stride(0), v.stride(1), v.data_ptr()
    if kind == DERIVE_SGPACK:
        assert int(N.lib().snvrag_sgemm_pack_bytes(cols, j.rows)) == dst.numel() * dst.element_size()
        j.pieces = j.rows * cols // 8
    elif kind == DERIVE_G2PACK:
        assert int(N.lib().snvrag_gemm256_pack_bytes(j.rows, cols)) == dst.numel() * dst.element_size()
        j.pieces = j.rows * cols // 8
    else:
        assert dst.dtype == (torch.float32 if kind == DERIVE_F32 else torch.bfloat16)
        assert (j.rows - 1) * j.dst_ld + cols <= dst.numel()
        j.pieces = (j.rows * cols + 7) // 8
    j.dst = dst.data_ptr()
    return j


def derive_table(jobs, device) -> Tuple[torch.Tensor, int, int]:
    """(device job table, job count, total pieces) for :func:`derive`."""
    total = 0
    for j in jobs:
        j.piece0 = total
        total += j.pieces
    arr = (N.DeriveJob * len(jobs))(*jobs)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(jobs), total


def derive(table: Tuple[torch.Tensor, int, int]) -> None:
    """Run every job of a :func:`derive_table` in one launch (csrc/sgemm.hip derive_kernel)."""
    t, n, total = table
    check(N.lib().snvrag_derive(ptr(t), n, total, stream_ptr()), "derive")


def tokgrad(tok: torch.Tensor, g: torch.Tensor, V: int, padding_idx: Optional[int] = None) -> torch.Tensor:
    """f32 [V, D] weight gradient of W[tok] for the f32 output gradient g [..., D] (csrc/train.hip)."""
    N.require_gpu(g)
    D = g.shape[-1]
    t = _c(tok.reshape(-1).long())
    g2 = _c(g.reshape(-1, D).float())
    M = t.numel()
    dw = torch.empty(V, D, device=g.device, dtype=torch.float32)
    wsb = int(N.lib().snvrag_tokgrad_ws_bytes(M, V, D))
    ws = torch.empty(wsb // 4, device=g.device, dtype=torch.float32)
    check(N.lib().snvrag_tokgrad(M, V, D, -1 if padding_idx is None else int(padding_idx), ptr(t), ptr(g2), ptr(dw),
                                 ptr(ws), wsb, stream_ptr()), "tokgrad")
    return dw


def head2_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """f32 [..., 2] = x w^T + b for bf16 x [..., K], f32 w [2, K], b [2] (csrc/train.hip head2)."""
    N.require_gpu(x)
    Kd = x.shape[-1]
    M = x.numel() // Kd
    out = torch.empty(*x.shape[:-1], 2, device=x.device, dtype=torch.float32)
    check(N.lib().snvrag_head2_fwd(M, Kd, ptr(_c(x)), ptr(_c(w.float())), ptr(_c(b.float())), ptr(out),
                                   stream_ptr()), "head2_fwd")
    return out


def head2_bwd(g: torch.Tensor, x: torch.Tensor, w: torch.Tensor, want_dx: bool = True,
              dw: Optional[torch.Tensor] = None, accumulate: bool = False):
    """(dx bf16 [..., K] or None, dw f32 [2, K]) of :func:`head2_fwd` for the f32 gradient g [..., 2];
    ``dw`` given: written or (accumulate) added in place."""
    Kd = x.shape[-1]
    M = x.numel() // Kd
    dx = torch.empty_like(x) if want_dx else None
    if dw is None:
        dw = torch.empty(2, Kd, device=x.device, dtype=torch.float32)
    wsb = int(N.lib().snvrag_head2_ws_bytes(M, Kd))
    ws = torch.empty(wsb // 4, device=x.device, dtype=torch.float32)
    check(N.lib().snvrag_head2_bwd(M, Kd, ptr(_c(g.float())), ptr(_c(x)), ptr(_c(w.float())), ptr(dx), ptr(dw),
                                   int(accumulate), ptr(ws), wsb, stream_ptr()), "head2_bwd")
    return dx, dw


def sgemm_vec(bias: torch.Tensor, c1: Optional[torch.Tensor] = None, c2: Optional[torch.Tensor] = None,
              ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """f32 vector table of :func:`sgemm`: [bias | c1, c2 | ln g, b | head w_out [2, N], b_out [2]]."""
    parts = [bias]
    if c1 is not None:
        parts += [c1, c2]
    if ln is not None:
        parts += list(ln)
    if head is not None:
        parts += [head[0].reshape(-1), head[1].reshape(-1)]
    return torch.cat([t.detach().float().reshape(-1) for t in parts]).contiguous()


def sgemm(x: torch.Tensor, wstream: torch.Tensor, n_out: int, vec: torch.Tensor, *, epi: int = SG_ACT,
          act: int = N.ACT_NONE, slope: float = 0.0,
          rank: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, eps: float = 1e-5,
          out: Optional[torch.Tensor] = None, want_logits: bool = False):
    """Stream GEMM (bf16): SG_ACT -> act(x W^T + b [+ r1 c1 + r2 c2]) [..., n_out] bf16;
    SG_LN -> LN(act(.) + x) [..., D] bf16; SG_HEAD2 -> (logits or None, probs) [..., 2] f32.
    ``rank = (r1 f32, r2 f32, period)``: row scalars indexed by row % period."""
    N.require_gpu(x)
    assert x.dtype == torch.bfloat16
    D = x.shape[-1]
    M = x.numel() // D
    probs = logits = None
    if epi == SG_HEAD2:
        probs = torch.empty(*x.shape[:-1], 2, device=x.device, dtype=torch.float32)
        logits = torch.empty_like(probs) if want_logits else None
    elif out is None:
        out = torch.empty(*x.shape[:-1], n_out, device=x.device, dtype=torch.bfloat16)
    r1 = r2 = None
    period = 0
    if rank is not None:
        r1, r2 = _c(rank[0].float()), _c(rank[1].float())
        period = int(rank[2])
        assert r1.numel() >= period and r2.numel() >= period and period > 0
    check(N.lib().snvrag_sgemm_forward(M, D, n_out, epi, act, slope, ptr(_c(x)), ptr(wstream), ptr(vec), ptr(r1),
                                       ptr(r2), period, eps, ptr(out), ptr(probs), ptr(logits), stream_ptr()),
          "sgemm")
    return (logits, probs) if epi == SG_HEAD2 else out


def mlp_pack(w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """Stream of the fused MLP kernel (csrc/sgemm.hip mlp_kernel): W1 [4D, D], W2 [D, 4D] (bf16)."""
    N.require_gpu(w1, w2)
    D = w1.shape[1]
    nbytes = int(N.lib().snvrag_mlp_pack_bytes(D))
    if nbytes == 0 or tuple(w1.shape) != (4 * D, D) or tuple(w2.shape) != (D, 4 * D):
        raise ValueError(f"MLP stream needs W1 [4D, D], W2 [D, 4D] with D = 384, got {tuple(w1.shape)}, {tuple(w2.shape)}")
    out = torch.empty(nbytes, device=w1.device, dtype=torch.uint8)
    check(N.lib().snvrag_mlp_pack(D, ptr(_c(w1.to(torch.bfloat16).contiguous())),
                                  ptr(_c(w2.to(torch.bfloat16).contiguous())), ptr(out), stream_ptr()), "mlp_pack")
    return out


def mlp(x: torch.Tensor, wstream: torch.Tensor, vec: torch.Tensor, *, epi2: int,
        rank: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, eps: float = 1e-5) -> torch.Tensor:
    """EPI2(GELU(x W1^T + b1 [+ rank]) W2^T + b2) [..., D] bf16 in one launch; epi2 0 = sigmoid,
    1 = LayerNorm; vec = [b1 | c1, c2 | b2 | g, be] (f32)."""
    N.require_gpu(x)
    assert x.dtype == torch.bfloat16
    D = x.shape[-1]
    M = x.numel() // D
    out = torch.empty_like(x)
    r1 = r2 = None
    period = 0
    if rank is not None:
        r1, r2, period = _c(rank[0].float()), _c(rank[1].float()), int(rank[2])
    check(N.lib().snvrag_mlp_forward(M, D, epi2, ptr(_c(x)), ptr(wstream), ptr(vec), ptr(r1), ptr(r2), period, eps,
                                     ptr(out), stream_ptr()), "mlp")
    return out


def mlp_afgate_pack(ag_t, mlp_vec: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gate fragments bf16, vector table f32) of :func:`mlp_afgate` from CrossAFInteraction's
    weights ``ag_t`` = [gate_net[0].weight [32, 2], .bias, gate_net[2].weight [D, 32], .bias,
    joint_encoder[0].weight [D, 2], .bias, joint_encoder[1].weight, .bias] (f32) and the af_adapter
    MLP's table ``mlp_vec`` = [b1 | b2] (include/snvrag.h snvrag_mlp_afgate_forward)."""
    g1w, g1b, g2w, g2b, jw, jb, lnw, lnb = [t.detach().float() for t in ag_t]
    D = g2w.shape[0]
    assert D == 384 and g2w.shape[1] == 32 and g1w.shape == (32, 2) and jw.shape == (D, 2)
    cols = [jw[:, 0].double(), jw[:, 1].double(), jb.double()]
    mu = [c.mean() for c in cols]
    cc = [c - m for c, m in zip(cols, mu)]
    mom = torch.stack(mu + [(cc[0] * cc[0]).mean(), (cc[1] * cc[1]).mean(), (cc[0] * cc[1]).mean(),
                            (cc[0] * cc[2]).mean(), (cc[1] * cc[2]).mean(), (cc[2] * cc[2]).mean()]).float()
    vec = torch.cat([mlp_vec.float().reshape(-1), g2b, jw[:, 0], jw[:, 1], jb, lnw, lnb, g1w.reshape(-1), g1b,
                     mom.to(g2b.device)]).contiguous()
    dev = g2w.device
    m = torch.arange(32, device=dev)
    outf = 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3)
    T = torch.arange(12, device=dev).view(12, 1, 1, 1)
    s = torch.arange(2, device=dev).view(1, 2, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 1, 8)
    rows = 32 * T + outf[lane % 32]
    cols = 16 * (lane // 32) + 8 * s + j
    w = g2w[rows.expand(12, 2, 64, 8), cols.expand(12, 2, 64, 8)]          # [T, s, lane, 8]
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    frags = torch.stack([hi, lo], 2).contiguous()                          # [T, s, part, lane, 8]
    return frags, vec


def mlp_afgate(af: torch.Tensor, af_p: torch.Tensor, frags: torch.Tensor, res_scale: float, wstream: torch.Tensor,
               vec: torch.Tensor, D: int = 384) -> torch.Tensor:
    """sigmoid(GELU(x W1^T + b1) W2^T + b2) with x = CrossAFInteraction(af, af_p) computed inside
    the launch (fusion.py:135-138); [*af.shape, D] bf16."""
    N.require_gpu(af, af_p)
    af, af_p = _c(af.float()), _c(af_p.float())
    assert af.numel() == af_p.numel()
    out = torch.empty(*af.shape, D, device=af.device, dtype=torch.bfloat16)
    check(N.lib().snvrag_mlp_afgate_forward(af.numel(), D, ptr(af), ptr(af_p), ptr(frags), res_scale, ptr(wstream),
                                            ptr(vec), ptr(out), stream_ptr()), "mlp_afgate")
    return out


def sgemm_cat(q: torch.Tensor, x2: torch.Tensor, g2: torch.Tensor, period: int, wstream: torch.Tensor, n_out: int,
              vec: torch.Tensor) -> torch.Tensor:
    """GELU([q | bf16(x2 * g2[m % period])] W^T + b) [..., n_out] (bf16; the rag fusion's
    cat(h, aw * h_rag) input of fusion.py:157 built in registers); W packed by sgemm_pack."""
    N.require_gpu(q, x2, g2)
    Dh = q.shape[-1]
    M = q.numel() // Dh
    assert q.dtype == x2.dtype == g2.dtype == torch.bfloat16 and x2.numel() == q.numel()
    assert g2.numel() >= period * Dh
    out = torch.empty(*q.shape[:-1], n_out, device=q.device, dtype=torch.bfloat16)
    check(N.lib().snvrag_sgemm_cat_forward(M, Dh, n_out, ptr(_c(q)), ptr(_c(x2)), ptr(_c(g2)), period, ptr(wstream),
                                           ptr(vec), ptr(out), stream_ptr()), "sgemm_cat")
    return out

