"""The block tail that also computes the next layer's QKV projection (csrc/tailw.hip, the projection
phase of tailw_kernel; snvrag_tail_qkv_forward; engine option tail_qkv).

The tail phases are untouched and the projection phase runs the chunk loop projw_kernel runs
(pw_chunks: the same operands, the same MFMAs in the same k order, the same epilogue), per token
group, so x must equal snvrag_tail_forward's and qkv snvrag_proj_forward's (proj_wide = 1) bit for bit.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
# one row, the edges of the 32-row token groups and of the 128-row tile, a tile + a group, and more
# than 256 tiles with a remainder of 3 tiles + 5 rows <= tail_split: 128-row (G = 4) and 32-row
# (G = 1) workgroups in one launch
M_SPLIT = 257 * 128 + 32 * 3 + 5
SHAPES = [1, 31, 32, 33, 127, 128, 129, 160, M_SPLIT]


def K():
    from src import kernels
    return kernels


def N():
    from src import native
    return native


_weights = {}


def _case(M):
    """Seeded bf16 operands of one block tail + the next layer's QKV weights (shared by every M)."""
    bf = torch.bfloat16
    if not _weights:
        g = torch.Generator(device="cpu").manual_seed(384)
        w = {}
        w["w_o"] = (torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV, bf)
        w["b_o"] = (0.1 * torch.randn(D, generator=g)).to(DEV)
        w["g1"], w["be1"] = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
        w1 = (torch.randn(4 * D, D, generator=g) / math.sqrt(D)).to(DEV, bf)
        w2 = (torch.randn(D, 4 * D, generator=g) / math.sqrt(4 * D)).to(DEV)
        b1, b2 = torch.randn(4 * D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
        gf, bff = (1 + 0.2 * torch.randn(4 * D, generator=g)).to(DEV), (0.1 * torch.randn(4 * D, generator=g)).to(DEV)
        g2, be2 = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
        w2g, b2g, _ = K().fold_layernorm(w2, b2, gf, bff, bf)
        w["vec"] = K().ffn_vec(b1, b2g, w2g, g2, be2)
        w["ts"] = K().tail_pack(w["w_o"], w1, w2g)
        w["w_qkv"] = (torch.randn(3 * D, D, generator=g) / math.sqrt(D)).to(DEV, bf)
        w["b_qkv"] = torch.randn(3 * D, generator=g).to(DEV)
        w["pw"] = K().proj_pack(w["w_qkv"])
        _weights.update(w)
    g = torch.Generator(device="cpu").manual_seed(1000 + M)
    x = torch.randn(M, D, generator=g).to(DEV, bf)
    att = (0.5 * torch.randn(M, D, generator=g)).to(DEV, bf)
    return dict(_weights, x=x, att=att)


def _fused(c, M, pad=2):
    x = c["x"].clone()
    qkv = torch.full((M + pad, 3 * D), 7.0, device=DEV, dtype=torch.bfloat16)   # sentinel rows past M
    K().tail_qkv_forward(c["att"], x, c["ts"], c["b_o"], c["g1"], c["be1"], c["vec"], c["pw"], c["b_qkv"],
                         qkv_out=qkv[:M])
    return x, qkv


def _halves(c, M):
    x = c["x"].clone()
    K().tail_forward(c["att"], x, c["ts"], c["b_o"], c["g1"], c["be1"], c["vec"])
    with K().option("proj_wide", 1):
        qkv = K().proj_forward(x, c["pw"], c["b_qkv"], 3)
    return x, qkv


@pytest.mark.parametrize("M,split", [(M, 64) for M in SHAPES] + [(M_SPLIT, 0)])
def test_tail_qkv_equals_tail_then_projection(M, split):
    """K.tail_qkv_forward == K.tail_forward followed by K.proj_forward (proj_wide = 1), bit for bit, on
    x and on qkv; rows >= M of a padded qkv buffer keep their sentinel.  The largest M runs 128-row and
    32-row workgroups in one launch (tail_split = 64) and 128-row workgroups only (tail_split = 0)."""
    c = _case(M)
    with K().option("tail_wide", 1), K().option("tail_split", split):
        xa, qa = _fused(c, M)
        xb, qb = _halves(c, M)
    assert torch.isfinite(xa.float()).all() and torch.isfinite(qa[:M].float()).all()
    assert torch.equal(xa, xb), float((xa.float() - xb.float()).abs().max())
    assert torch.equal(qa[:M], qb), float((qa[:M].float() - qb.float()).abs().max())
    assert (qa[M:] == 7.0).all()                          # nothing written past the last row
    # and the projection is the projection: float64 torch on the same bf16 operands, the bar of
    # test_gpu_kernels.py::test_proj_kernel_vs_fp64
    ref = xb.double() @ c["w_qkv"].double().T + c["b_qkv"].double()
    torch.testing.assert_close(qa[:M].double(), ref, rtol=2e-2, atol=2e-2)


def test_tail_qkv_refuses_what_it_cannot_run():
    """Only D = 384 on the wide-row tail: anything else is an argument error, never another kernel."""
    c = _case(33)
    with K().option("tail_wide", 0), pytest.raises(RuntimeError):
        _fused(c, 33)
    x = torch.zeros(4, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        K().tail_qkv_forward(x.clone(), x, c["ts"], c["b_o"][:256], c["g1"][:256], c["be1"][:256], c["vec"], c["pw"],
                             c["b_qkv"])


# ------------------------------------------------------------------------------ engine --
_engine = {}


def _packed():
    if not _engine:
        from src.model import build_model
        from src.engine import engine_for
        torch.manual_seed(0)
        m = build_model(12, D, 3, 12).to(DEV).eval()
        eng = engine_for(m)
        eng.set_dtype(torch.bfloat16)
        _engine["eng"], _engine["P"] = eng, eng.packed()
    return _engine["P"]


def _encode(x0, layers, **opts):
    """(output, kinds of the launches the encoder logged) under the given options."""
    nseq, L, _ = x0.shape
    ws = torch.empty(K().encoder_ws_bytes(torch.bfloat16, nseq, L, D, 12), device=DEV, dtype=torch.uint8)
    x = x0.clone()
    lib, cap = N().lib(), 256
    prev = {k: K().set_option(k, v) for k, v in opts.items()}
    try:
        lib.snvrag_evlog_enable(cap)
        K().encoder_forward(x, layers, 12, ws)
        torch.cuda.synchronize()
        kinds, ms, work = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.float64)
        n = lib.snvrag_evlog_read(kinds.ctypes.data, ms.ctypes.data, work.ctypes.data, cap)
    finally:
        lib.snvrag_evlog_enable(0)
        for k, v in prev.items():
            K().set_option(k, v)
    return x, kinds[:n].tolist(), work[:n].tolist()


@pytest.mark.parametrize("nseq,L", [(5, 1030), (2, 70)])
def test_encoder_tail_qkv_equals_separate_launches(nseq, L):
    """3 layers: with tail_qkv = 1 only layer 0 launches a QKV GEMM (1 GEMM-kind launch instead of 3,
    the fused tails logged as block launches with the projection's work added), and the output equals
    the tail_qkv = 0 sequence bit for bit."""
    P = _packed()
    g = torch.Generator(device="cpu").manual_seed(nseq * L)
    x0 = torch.randn(nseq, L, D, generator=g).to(DEV, torch.bfloat16)
    a, ka, wa = _encode(x0, P.layers, tail_qkv=1)
    b, kb, wb = _encode(x0, P.layers, tail_qkv=0)
    assert ka.count(1) == 1 and kb.count(1) == 3, (ka, kb)
    assert ka.count(2) == 3 and ka.count(8) == 3 and kb.count(8) == 3, (ka, kb)
    M = nseq * L
    blocks = [w for k, w in zip(ka, wa) if k == 8]
    assert blocks == [24.0 * M * D * D, 24.0 * M * D * D, 18.0 * M * D * D], blocks
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


def test_encoder_tail_qkv_falls_back_to_separate_launches():
    """tail_qkv = 1 where the fused form cannot run — tail_kernel (tail_wide = 0), or layer records
    without the packed projection stream — is the old launch sequence with the old result."""
    P = _packed()
    g = torch.Generator(device="cpu").manual_seed(9)
    x0 = torch.randn(2, 70, D, generator=g).to(DEV, torch.bfloat16)
    a, ka, _ = _encode(x0, P.layers, tail_qkv=1, tail_wide=0)
    b, kb, _ = _encode(x0, P.layers, tail_qkv=0, tail_wide=0)
    assert ka == kb and ka.count(1) == 3, (ka, kb)
    assert torch.equal(a, b)
    bare = [N().LayerW(**{k: v.data_ptr() for k, v in t.items() if k != "qkv_pw"}, q_scale=ly.q_scale)
            for t, ly in zip(P.layers_t, P.layers)]
    c, kc, _ = _encode(x0, bare, tail_qkv=1)
    d, kd, _ = _encode(x0, P.layers, tail_qkv=0)
    assert kc == kd and kc.count(1) == 3, (kc, kd)
    assert torch.equal(c, d)
