"""CPU proof of tests/attn_refs.py, the yardstick of tests/test_gpu_attention.py: the fp64
references equal torch autograd of the plain formula, the emulations (the references with the
kernels' rounding points) stay inside the derived elementwise bounds on every random-input shape the
GPU file runs (max err / bound printed per case, must be <= 1), and under the emulations every
exact-answer builder gives its exact answer at every L of the sweep with every precondition met."""
import math

import pytest
import torch

import attn_refs as R

F64 = torch.float64


def _autograd(qkv, dout, nseq, L, H, dh, scale, keep, p):
    x = qkv.to(F64).clone().requires_grad_(True)
    q, k, v = x.view(nseq, L, 3, H, dh).permute(2, 0, 3, 1, 4)
    P = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
    if keep is not None:
        P = P * torch.as_tensor(keep).to(F64) / (1.0 - R._f32(p))
    out = (P @ v).permute(0, 2, 1, 3).reshape(nseq * L, H * dh)
    out.backward(dout.to(F64))
    D = H * dh
    return out.detach(), x.grad[:, :D], x.grad[:, D:2 * D], x.grad[:, 2 * D:]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("L,H,dh", [(1, 1, 16), (37, 2, 32), (130, 3, 64)])
def test_refs_equal_autograd(L, H, dh, p):
    nseq, scale = 2, dh ** -0.5
    qkv, dout = R.random_qkv(nseq, L, H, dh, 1.5, L), R.random_dout(nseq, L, H, dh, L)
    keep = R.keep_mask(nseq, H, L, p)
    out, lse, P = R.ref_fwd(qkv, nseq, L, H, dh, scale, keep, p)
    a_out, a_dq, a_dk, a_dv = _autograd(qkv, dout, nseq, L, H, dh, scale, keep, p)
    dq, dk, dv = R.ref_bwd(qkv, dout, out, lse, nseq, L, H, dh, scale, keep, p)
    for name, got, want in (("out", out, a_out), ("dQ", dq, a_dq), ("dK", dk, a_dk), ("dV", dv, a_dv)):
        err = float((got - want).abs().max())
        print(f"{name} L={L} dh={dh} p={p}: max |ref - autograd| {err:.2e}")
        assert err <= 1e-12, name
    assert float((P.sum(-1) - 1).abs().max()) <= 1e-12
    q, k, _ = R.split(qkv, nseq, L, H, dh)
    want_lse = torch.logsumexp((q @ k.transpose(-1, -2)) * scale, -1) * R.LOG2E
    assert float((lse - want_lse).abs().max()) <= 1e-12 * (1 + float(want_lse.abs().max()))


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.75, 2.0 ** -20], dtype=F64)
    assert R.bf16_ulp(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0 ** -27]


# ---------------------------------------------------------- emulation inside the bounds --
@pytest.mark.parametrize("amp", R.RANDOM_AMPS)
@pytest.mark.parametrize("L", R.L_RANDOM)
@pytest.mark.parametrize("path", ["dma32_pre", "dma32", "train32"])
def test_emu_fwd_within_bound(path, L, amp):
    nseq, H, dh = 2, 2, 32
    pre = path == "dma32_pre"
    scale = R.PRESCALED if pre else dh ** -0.5
    qkv = R.random_qkv(nseq, L, H, dh, amp, L, prescaled=pre)
    ref, bound = R.fwd_bound(qkv, nseq, L, H, dh, scale, path=path)
    out, lse, nfall = R.emu_fwd(qkv, nseq, L, H, dh, scale, path=path)
    r = R.ratio(out, ref, bound)
    print(f"emu fwd {path} L={L} amp={amp}: max err/bound {r:.3f}")
    assert r <= 1.0 and nfall == 0
    if path == "train32":                                # the only one of the three kernels that writes lse
        _, rlse, _ = R.ref_fwd(qkv, nseq, L, H, dh, scale)
        assert R.ratio(lse, rlse, R.lse_bound(rlse, path)) <= 1.0


@pytest.mark.parametrize("L,dh,path", [(65, 64, "generic"), (257, 64, "generic"), (129, 16, "generic"),
                                       (129, 48, "generic"), (257, 32, "f32"), (65, 16, "f32")])
def test_emu_fwd_generic_and_f32_within_bound(L, dh, path):
    nseq, H = 2, 2
    qkv = R.random_qkv(nseq, L, H, dh, 1.5, L + dh)
    ref, bound = R.fwd_bound(qkv, nseq, L, H, dh, path=path)
    out, _, _ = R.emu_fwd(qkv, nseq, L, H, dh, path=path)
    r = R.ratio(out, ref, bound)
    print(f"emu fwd {path} dh={dh} L={L}: max err/bound {r:.3f}")
    assert r <= 1.0


def _bwd_case(L, dh, p):
    nseq, H = 2, 2
    qkv, dout = R.random_qkv(nseq, L, H, dh, R.BWD_AMP, 3 * L + dh), R.random_dout(nseq, L, H, dh, L)
    keep = R.keep_mask(nseq, H, L, p)
    out, lse, _ = R.ref_fwd(qkv, nseq, L, H, dh, None, keep, p)
    out, lse = out.to(torch.bfloat16), lse.to(torch.float32)
    refs = R.ref_bwd(qkv, dout, out, lse, nseq, L, H, dh, None, keep, p)
    As = R.bwd_abs(qkv, dout, out, lse, nseq, L, H, dh, None, keep, p)
    emu = R.emu_bwd(qkv, dout, out, lse, nseq, L, H, dh, None, keep, p)
    return [R.ratio(e, r, R.bwd_bound(r, a, f)) for e, r, a, f in zip(emu, refs, *As)]


@pytest.mark.parametrize("L,dh,p", [(L, 32, 0.0) for L in R.L_SWEEP] + [(L, 64, 0.0) for L in R.L_DH64]
                         + [(L, dh, 0.1) for L, dh in R.BWD_DROP_SHAPES])
def test_emu_bwd_within_bound(L, dh, p):
    r = _bwd_case(L, dh, p)
    print(f"emu bwd dh={dh} L={L} p={p}: max err/bound dQ {r[0]:.3f} dK {r[1]:.3f} dV {r[2]:.3f}")
    assert max(r) <= 1.0


# ------------------------------------------------------- builders under the emulation --
def _paths(dh):
    return (("dma32_pre", True), ("dma32", False), ("train32", False)) if dh == 32 else (("generic", False), ("f32", False))


@pytest.mark.parametrize("dh,L", [(32, L) for L in R.L_SWEEP] + [(dh, L) for dh in (16, 48, 64) for L in R.L_GENERIC])
def test_builders_exact_under_emulation(dh, L):
    nseq, H = 2, 2
    for path, pre in _paths(dh):
        scale = R.PRESCALED if pre else dh ** -0.5
        qkv, cnt = R.uniform_case(L, H, dh, nseq)
        out, lse, nfall = R.emu_fwd(qkv, nseq, L, H, dh, scale, path=path)
        assert torch.equal(R.decode_counts(out, L), cnt.repeat(H).expand(nseq * L, H * dh)), ("uniform", path)
        assert nfall == 0
        if lse is not None:
            assert float((lse - math.log2(L)).abs().max()) <= 2.0 ** -22 * max(1.0, math.log2(L))
        for over in ((False, True) if L > R.KT else (False,)):
            qkv, expect, sc, pi = R.onehot_case(L, H, dh, over, nseq, prescaled=pre)
            out, lse, nfall = R.emu_fwd(qkv, nseq, L, H, dh, sc, path=path)
            assert torch.equal(out, expect), ("onehot", path, over)
            if path == "train32" or (path == "generic" and dh == 64):       # the training forwards
                rlse = R.ref_fwd(qkv, nseq, L, H, dh, sc)[1]
                assert R.ratio(lse, rlse, 1e-5 * (1 + rlse.abs())) <= 1.0, ("onehot lse", path, over)
            if dh == 32:
                assert (nfall > 0) == over, (path, over, nfall)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dh,L", [(32, L) for L in R.L_SWEEP] + [(64, L) for L in R.L_DH64])
def test_dropout_counts_under_emulation(dh, L, p):
    nseq, H = 2, 2
    keep = R.keep_mask(nseq, H, L, p)
    qkv, _ = R.uniform_case(L, H, dh, nseq)
    out, lse, _ = R.emu_fwd(qkv, nseq, L, H, dh, None, keep, p, path="train32" if dh == 32 else "generic")
    assert torch.equal(R.decode_counts(out, L * (1 - p)), R.kept_counts(keep, L, H, dh, "k"))
    assert float((lse - math.log2(L)).abs().max()) <= 2.0 ** -22 * max(1.0, math.log2(L))
    # the backward twin, fed the reference's bf16 out and f32 lse
    rout, rlse, _ = R.ref_fwd(qkv, nseq, L, H, dh, None, keep, p)
    dout = R.uniform_dout(L, H, dh, nseq)
    dq, dk, dv = R.emu_bwd(qkv, dout, rout.to(torch.bfloat16), rlse.to(torch.float32), nseq, L, H, dh, None, keep, p)
    assert torch.equal(R.decode_counts(dv, L * (1 - p)), R.kept_counts(keep, L, H, dh, "q"))
    assert not dk.any()


@pytest.mark.parametrize("dh,L", [(32, L) for L in R.L_SWEEP] + [(64, L) for L in R.L_DH64])
def test_uniform_backward_twin_under_emulation(dh, L):
    nseq, H = 2, 2
    qkv, cnt = R.uniform_case(L, H, dh, nseq)
    rout, rlse, _ = R.ref_fwd(qkv, nseq, L, H, dh)
    dout = R.uniform_dout(L, H, dh, nseq)
    args = (qkv, dout, rout.to(torch.bfloat16), rlse.to(torch.float32), nseq, L, H, dh)
    dq, dk, dv = R.emu_bwd(*args)
    assert torch.equal(R.decode_counts(dv, L), cnt.repeat(H).expand(nseq * L, H * dh))
    assert not dk.any()
    rq = R.ref_bwd(*args)[0]
    ab = R.bwd_abs(*args)
    assert R.ratio(dq, rq, R.bwd_bound(rq, ab[0][0], ab[1][0])) <= 1.0


def test_onehot_pi_covers_the_tile_edges():
    for L in R.L_SWEEP:
        pi = set(R.onehot_pi(L).tolist())
        want = set(range(min(64, L))) | {L - 1}
        for t in range(0, L, 64):
            want |= {t, min(t + 64, L) - 1}
        assert want <= pi, L
