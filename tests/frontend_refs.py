"""Plain torch restatements of the embedding, feature and head kernels (csrc/embed.hip and
rag_concat of csrc/norm.hip) for the kernel-level tests.  Each takes the raw tensors the kernel
takes and evaluates on the CPU in ``dtype``: float64 is the reference; float32 is the
calibration run that shows a test's inputs are benign (a plain f32 evaluation already meets the
test's bound, so a miss is the kernel's).  Weight lists are in the field order of the native
structs (native.PosfeatW / AfGateW / GtW)."""

import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """One bf16 unit in the last place at each reference value (0 at 0): 2^(e - 7) for
    |ref| in [2^e, 2^(e + 1))."""
    _, e = torch.frexp(ref.double())                       # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref, dtype=F64), torch.ldexp(torch.ones_like(ref, dtype=F64), e - 8))


def af_features(af, freqs, dtype=F64):
    """[sin | cos] of the model's f32 angle f32(f32(2 pi) * f32(af * f)) (af_embedding.py:79-84):
    the operation is sin/cos of that f32 number, not of the real-number angle."""
    x = _t(af, torch.float32)[..., None] * _t(freqs, torch.float32)
    a = (torch.tensor(2 * math.pi, dtype=torch.float32) * x).to(dtype)
    return torch.cat([torch.sin(a), torch.cos(a)], -1)


def embed(tok, W, pe, afemb, period, dtype=F64):
    """(W[clamp(tok, 0, vocab - 1)] + pe[l]) + afemb[(s % period if period > 0 else s), l]
    (embedding/bert.py:66-75); tok [nseq, L], afemb [P, L, D] or [L, D] or None."""
    nseq, L = tok.shape
    t = tok.detach().cpu().long().clamp(0, W.shape[0] - 1)
    out = _t(W, dtype)[t] + _t(pe, dtype)[:L]
    if afemb is not None:
        a = _t(afemb, dtype).reshape(-1, L, W.shape[1])
        s = torch.arange(nseq)
        out = out + a[s % period if period > 0 else s]
    return out


def posfeat(pos, w, eps, dtype=F64):
    """conv(k=9, pad=4) -> lrelu 0.05 -> eval BatchNorm, twice, then conv -> lrelu 0.05
    (fusion.py:324-332).  w: c1_w c1_b c2_w c2_b c3_w c3_b, then weight / bias / running mean /
    running var of norm1 and of norm2."""
    c1w, c1b, c2w, c2b, c3w, c3b, g1, b1, m1, v1, g2, b2, m2, v2 = [_t(t, dtype) for t in w]

    def bn(x, g, b, m, v):
        return (x - m[None, :, None]) / torch.sqrt(v[None, :, None] + eps) * g[None, :, None] + b[None, :, None]

    x = _t(pos, dtype)[:, None, :]
    x = bn(F.leaky_relu(F.conv1d(x, c1w.view(4, 1, 9), c1b, padding=4), 0.05), g1, b1, m1, v1)
    x = bn(F.leaky_relu(F.conv1d(x, c2w.view(4, 4, 9), c2b, padding=4), 0.05), g2, b2, m2, v2)
    return F.leaky_relu(F.conv1d(x, c3w.view(1, 4, 9), c3b, padding=4), 0.05)[:, 0, :]


def layernorm(x, g, b, eps=1e-5):
    """Direct per-row LayerNorm: the row's own mean and (biased) variance."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def af_gate(af, af_p, w, res_scale, dtype=F64):
    """af + rs * sigmoid(W2 gelu(W1 c + b1) + b2) * gelu(LN(Wj c + bj)), c = (af, af_p)
    (fusion.py:82-86).  w: g1_w [32, 2], g1_b, g2_w [D, 32], g2_b, j_w [D, 2], j_b, ln_w, ln_b."""
    g1w, g1b, g2w, g2b, jw, jb, lw, lb = [_t(t, dtype) for t in w]
    af = _t(af, dtype)
    c = torch.stack([af, _t(af_p, dtype)], -1)
    gate = torch.sigmoid(F.gelu(c @ g1w.T + g1b) @ g2w.T + g2b)
    enc = F.gelu(layernorm(c @ jw.T + jb, lw, lb))
    return af[..., None] + res_scale * (gate * enc)


def rag_concat(q, rag, wgt, period, dtype=F64):
    """[q | rag * wgt[m % period]] over flattened rows m (fusion.py:139-150 with K = 1)."""
    D = q.shape[-1]
    q2, r2, w2 = _t(q, dtype).reshape(-1, D), _t(rag, dtype).reshape(-1, D), _t(wgt, dtype).reshape(-1, D)
    m = torch.arange(q2.shape[0])
    return torch.cat([q2, r2 * w2[m % period if period > 0 else m]], -1)


def hap_head(h, w, b, dtype=F64):
    """(logits, softmax(logits)) of Linear(K -> 2) (foundation_model.py:77-80)."""
    logits = _t(h, dtype) @ _t(w, dtype).T + _t(b, dtype)
    return logits, torch.softmax(logits, -1)


def gt_head(p1, p2, ref, het, hom, period, w, dtype=F64):
    """Linear(7, 16) -> lrelu 0.01 -> LN -> [Linear -> lrelu 0.1 -> LN -> Linear -> lrelu 0.1] ->
    Linear(16, 4) -> softmax (foundation_model.py:159-176); row m reads ref / het / hom at
    m % period (period > 0).  w: f_w f_b n_w n_b w1 b1 ln_w ln_b w2 b2 c_w c_b."""
    fw, fb, nw, nb, w1, b1, lw, lb, w2, b2, cw, cb = [_t(t, dtype) for t in w]
    p1, p2 = _t(p1, dtype).reshape(-1, 2), _t(p2, dtype).reshape(-1, 2)
    m = torch.arange(p1.shape[0])
    mr = m % period if period > 0 else m
    side = [_t(t, dtype).reshape(-1)[mr][:, None] for t in (ref, het, hom)]
    x = torch.cat([p1, p2] + side, -1)
    x = layernorm(F.leaky_relu(x @ fw.view(16, 7).T + fb, 0.01), nw, nb)
    x = layernorm(F.leaky_relu(x @ w1.view(16, 16).T + b1, 0.1), lw, lb)
    x = F.leaky_relu(x @ w2.view(16, 16).T + b2, 0.1)
    return torch.softmax(x @ cw.view(4, 16).T + cb, -1)
