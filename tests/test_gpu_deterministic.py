"""The deterministic training mode (library option ``deterministic``, trainer keyword, CLI flag):
every reduction of a training step in an order fixed by the shapes alone.

  * dW (csrc/dw.hip, ``*_det``): per-chunk partial tiles + one fixed-order reduce.  Bitwise equal
    across launches and across ``dw_xcd`` 0 / 1 (two different hand-outs of the chunks to the
    workgroups), within ``test_linear_dw_kernel_vs_fp32``'s tolerance of the f64 reference, and
    accumulation == prior + zero-start result in f32.
  * token-table gradient (``snvrag_nbr_mean_drop_bwd_det``): bitwise equal across launches, within
    the adjoint tolerance of ``test_fused_neighbour_mean_dropout_vs_torch`` (1e-4 of the largest
    reference entry) of torch's f64 autograd, ``<pad>`` row zero.
  * focal loss (``snvrag_focal_loss_det``): bitwise equal across launches and equal, bit for bit,
    to a host f32 sum in the documented order (wave butterfly, four wave partials left to right,
    blocks in index order) of the KERNEL's per-row losses (read back by giving every row a block
    of its own).  The numpy oracle's per-row losses differ from the kernel's expf / logf / powf in
    the last bits, so against the oracle the sum is held to the existing test's 1e-5 relative.
  * the whole ``train_step`` in two fresh processes (the second with ``dw_xcd`` 0): losses,
    weights and retrieved neighbours equal bit for bit over three steps.
  * option off: the wrappers call the atomic entry points and never touch the workspace cache.
"""

import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------- dW --
def _dw(K, dy, x, splits, n_parts, prior=None):
    """(dw [N, K], db [N]) of one deterministic launch: zero start or onto ``prior`` = (w, b)."""
    N_, K_ = dy.shape[1], x.shape[1]
    w = torch.zeros(N_, K_, device=DEV) if prior is None else prior[0].clone()
    b = torch.zeros(N_, device=DEV) if prior is None else prior[1].clone()
    if n_parts == 1:
        K.linear_dw(dy, x, splits=splits, dw=w, db=b)
        return w, b
    ws = [p.clone() for p in w.chunk(n_parts)]                  # separately allocated parts
    bs = [p.clone() for p in b.chunk(n_parts)]
    K.linear_dw_parts(dy, x, ws, bs, splits=splits)
    return torch.cat(ws), torch.cat(bs)


@pytest.mark.parametrize("M,N,K_,splits,n_parts", [(1, 128, 128, 0, 1), (1000, 1152, 384, 0, 3),
                                                   (4097, 384, 1536, 0, 1), (4097, 384, 1536, 3, 1)])
def test_dw_fixed_order(M, N, K_, splits, n_parts):
    from src import kernels as K
    g = torch.Generator(device="cpu").manual_seed(M + N)
    dy = torch.randn(M, N, generator=g).to(DEV, torch.bfloat16)
    x = torch.randn(M, K_, generator=g).to(DEV, torch.bfloat16)
    prior = (torch.randn(N, K_, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV))
    ref_w = dy.double().t() @ x.double()
    ref_b = dy.double().sum(0)
    tol = 1e-5 * math.sqrt(M) * 4
    with K.option("deterministic", 1):
        assert K.deterministic()
        with K.option("dw_xcd", 1):
            w1, b1 = _dw(K, dy, x, splits, n_parts)
            w2, b2 = _dw(K, dy, x, splits, n_parts)
            wa, ba = _dw(K, dy, x, splits, n_parts, prior)
        with K.option("dw_xcd", 0):
            w0, b0 = _dw(K, dy, x, splits, n_parts)
        # the single-output entry point sums the same partials in the same order
        ws_, bs_ = _dw(K, dy, x, splits, 3 if n_parts == 1 and N % 384 == 0 else 1)
    ew, eb = (w1.double() - ref_w).abs().max().item(), (b1.double() - ref_b).abs().max().item()
    print(f"dW det M={M} N={N} K={K_} splits={splits}: max |dw - ref| {ew:.3e} |db - ref| {eb:.3e} (tol {tol:.3e})")
    assert ew < tol and eb < tol
    assert _same(w1, w2) and _same(b1, b2), "two launches differ"
    assert _same(w1, w0) and _same(b1, b0), "dw_xcd 0 and 1 differ"
    assert _same(w1, ws_) and _same(b1, bs_), "linear_dw and linear_dw_parts differ"
    # accumulation: prior + (ws[0] + ... + ws[S-1]), the prior added last, in f32
    assert _same(wa, prior[0] + w1) and _same(ba, prior[1] + b1)


# --------------------------------------------------------------------- token-table gradient --
def _nbr_case(nq, empty_query):
    g = torch.Generator(device="cpu").manual_seed(11)
    k, U, L, D, n = 8, 40, 300, 64, 290
    inv = torch.randint(0, U, (12, k), generator=g).to(torch.int32)[:nq].contiguous()
    if nq > 3:
        inv[3, 5:] = -1
    if empty_query:
        inv[nq - 1, :] = -1                                   # a query with no valid neighbour
    codes = torch.randint(0, 2, (U, n), generator=g).to(torch.uint8)
    W = torch.randn(10, D, generator=g)
    W[0] = 0
    pe = torch.randn(L, D, generator=g) * 0.1
    Ar = torch.randn(L, D, generator=g) * 0.1
    R = torch.randn(12, L, D, generator=g)[:nq].contiguous()
    return inv, codes, W, pe, Ar, R, n


@pytest.mark.parametrize("nq,empty_query", [(1, False), (6, True), (12, True)])
def test_token_table_gradient_fixed_order(nq, empty_query):
    from src import kernels as K
    inv, codes, W, pe, Ar, R, n = _nbr_case(nq, empty_query)
    U, L, D = codes.shape[0], pe.shape[0], pe.shape[1]
    d = lambda t: t.to(DEV)
    # torch f64 autograd at p = 0: embed the unique neighbours, average per query
    tok = torch.zeros(U, L, dtype=torch.long)
    tok[:, 0] = 2
    tok[:, n + 1] = 3
    tok[:, 1:1 + n] = 5 + codes.long()
    Wr, Arr = W.double().requires_grad_(True), Ar.double().requires_grad_(True)
    E = Wr[tok] + pe.double() + Arr
    out = torch.stack([E[inv[q][inv[q] >= 0].long()].mean(0) if (inv[q] >= 0).any() else torch.zeros(L, D).double()
                       for q in range(nq)])
    out.backward(R.double())
    ref_w = Wr.grad.clone()
    ref_w[0] = 0                                               # padding_idx: no gradient

    def run(p, seed):
        gW, gA = torch.zeros(10, D, device=DEV), torch.zeros(L, D, device=DEV)
        K.nbr_mean_drop_bwd(d(R), d(inv), d(codes), n, d(W), d(pe), d(Ar), p, seed, gW, gA)
        return gW, gA

    with K.option("deterministic", 1):
        w1, a1 = run(0.0, 1)
        w2, a2 = run(0.0, 1)
        wd1, ad1 = run(0.3, 9)
        wd2, ad2 = run(0.3, 9)
        prior = torch.randn(10, D, generator=torch.Generator().manual_seed(3)).to(DEV)
        acc = prior.clone()
        K.nbr_mean_drop_bwd(d(R), d(inv), d(codes), n, d(W), d(pe), d(Ar), 0.3, 9, acc, torch.zeros(L, D, device=DEV))
    wd_atomic, ad_atomic = run(0.3, 9)                         # the default (atomic) path, same mask
    assert _same(w1, w2) and _same(a1, a2) and _same(wd1, wd2) and _same(ad1, ad2)
    scale = ref_w.abs().max().item()
    err_w = (w1.cpu().double() - ref_w).abs().max().item()
    err_a = (a1.cpu().double() - Arr.grad).abs().max().item()
    err_d = (wd1 - wd_atomic).abs().max().item()
    print(f"nbr det nq={nq}: max |dW - ref| {err_w:.3e} of {scale:.3e}, |dAr - ref| {err_a:.3e}, "
          f"det vs atomic (p = 0.3) {err_d:.3e}")
    assert err_w <= 1e-4 * scale and err_a <= 1e-4 * Arr.grad.abs().max().item()
    assert err_d <= 1e-4 * wd_atomic.abs().max().item()
    assert (ad1 - ad_atomic).abs().max().item() <= 1e-4 * ad_atomic.abs().max().item()
    assert float(w1[0].abs().max()) == 0.0 and float(wd1[0].abs().max()) == 0.0      # <pad>
    assert _same(acc, prior + wd1)                             # accumulated, prior added last


# ------------------------------------------------------------------------------ focal loss --
def _host_sum_documented_order(rows: np.ndarray) -> np.float32:
    """f32 sum of per-row losses as focal_kernel<DET> + focal_final_kernel take it: 256 rows per
    block; per 64-lane wave a butterfly over lane distances 32, 16, .., 1; the four wave sums left
    to right; the block sums one after the other in index order, from 0."""
    nb = (len(rows) + 255) // 256
    v = np.zeros(nb * 256, np.float32)
    v[:len(rows)] = rows
    v = v.reshape(nb, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    blocks = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s = np.float32(0)
    for b in blocks:
        s = np.float32(s + b)
    return s


def _kernel_row_losses(x, y, m, gamma, weight):
    """The kernel's own per-row losses: row i placed alone (with 255 masked rows) in block i, so
    the block partial the entry point leaves in the caller's workspace is that row's loss."""
    from src import native as N
    M, C = x.shape
    xs = torch.zeros(M * 256, C, device=DEV)
    ys = torch.zeros(M * 256, dtype=torch.long, device=DEV)
    ms = torch.zeros(M * 256, dtype=torch.uint8, device=DEV)
    xs[::256], ys[::256], ms[::256] = x, y, m.to(torch.uint8)
    ws = torch.zeros(M, device=DEV)
    loss, grad = torch.zeros(1, device=DEV), torch.empty_like(xs)
    assert int(N.lib().snvrag_focal_loss_det_ws_bytes(M * 256)) == 4 * M
    N.check(N.lib().snvrag_focal_loss_det(M * 256, C, N.ptr(xs), N.ptr(ys), N.ptr(ms), gamma, weight, N.ptr(loss),
                                          N.ptr(grad), N.ptr(ws), 4 * M, N.stream_ptr()))
    return ws.cpu().numpy()


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("M", [1, 255, 257, 49440 // 8 + 5])
def test_focal_loss_fixed_order(M, C):
    from oracle import train_np
    from src import kernels as K
    g = torch.Generator(device="cpu").manual_seed(M * 8 + C)
    x = torch.softmax(torch.randn(M, C, generator=g) * 2, -1).to(DEV)
    y = torch.randint(0, C, (M,), generator=g).to(DEV)
    m = (torch.rand(M, generator=g) < 0.6).to(DEV)
    m[0] = True
    loss0, grad0 = K.focal_loss(x, y, m, 2.0, 3.0)             # default path
    with K.option("deterministic", 1):
        l1, g1 = K.focal_loss(x, y, m, 2.0, 3.0)
        l2, g2 = K.focal_loss(x, y, m, 2.0, 3.0)
        acc = torch.full((1,), 5.0, device=DEV)
        K.focal_loss(x, y, m, 2.0, 3.0, loss_acc=acc)
    assert _same(l1, l2) and _same(g1, g2)
    assert _same(g1, grad0), "grad differs from the default path's"
    rows = _kernel_row_losses(x, y, m, 2.0, 3.0)
    want = _host_sum_documented_order(rows)
    got = l1.cpu().numpy()[0]
    ol, _ = train_np.focal_loss(x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy(), 2.0)
    print(f"focal det M={M} C={C}: {got!r} host order {want!r} oracle {3.0 * ol!r} atomic {loss0.item()!r}")
    assert got.view(np.int32) == want.view(np.int32), (got, want)
    assert acc.cpu().numpy()[0].view(np.int32) == np.float32(np.float32(5.0) + want).view(np.int32)
    np.testing.assert_allclose(got, 3.0 * ol, rtol=1e-5)


# -------------------------------------------------------------------------- off means off --
def test_option_off_calls_the_atomic_entry_points():
    from src import kernels as K
    assert not K.deterministic()
    before = dict(K._det_ws)
    calls = []
    lib = K.N.lib()
    names = ("snvrag_linear_dw", "snvrag_linear_dw_parts", "snvrag_nbr_mean_drop_bwd", "snvrag_focal_loss")
    orig = {n: getattr(lib, n) for n in names + tuple(n + "_det" for n in names)}

    def spy(n):
        def f(*a):
            calls.append(n)
            return orig[n](*a)
        return f
    try:
        for n in orig:
            setattr(lib, n, spy(n))
        dy = torch.randn(64, 384, device=DEV).bfloat16()
        x = torch.randn(64, 128, device=DEV).bfloat16()
        K.linear_dw(dy, x, bias=True)
        K.linear_dw_parts(dy, x, [torch.zeros(128, 128, device=DEV) for _ in range(3)])
        inv, codes, W, pe, Ar, R, n = _nbr_case(2, False)
        d = lambda t: t.to(DEV)
        K.nbr_mean_drop_bwd(d(R), d(inv), d(codes), n, d(W), d(pe), d(Ar), 0.0, 1, torch.zeros(10, 64, device=DEV),
                            torch.zeros(300, 64, device=DEV))
        K.focal_loss(torch.rand(10, 2, device=DEV), torch.zeros(10, dtype=torch.long, device=DEV),
                     torch.ones(10, dtype=torch.bool, device=DEV), 2.0, 1.0)
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(lib, n, f)
    assert calls == list(names), calls
    assert K._det_ws == before and all(K._det_ws[k] is before[k] for k in before)


# --------------------------------------------------------- whole step, two fresh processes --
def _child(dims: int, heads: int, xcd: int) -> None:
    """Three deterministic train_steps on tests/test_gpu_ddp.py's tiny setup (at ``dims``), printing
    per step the loss bits, a hash of the flat parameter buffer and a hash of the retrieved
    neighbours; after the first backward also one hash per parameter gradient (diagnostic)."""
    import faulthandler
    faulthandler.dump_traceback_later(150, exit=True)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rag-snvbert_amd")]
    from src import kernels as K
    from src.dataset.embedding_rag_dataset import embedding_rag_collate_fn
    from src.dataset.synthetic import make_rag_dataset
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized
    from src.model import build_model
    torch.manual_seed(0)
    np.random.seed(0)                   # the construction-time window masks draw from the global RNG
    ds, vocab = make_rag_dataset(n_samples=8, n_sites=300, n_windows=2, n_ref_samples=40, seed=5, name="train")
    ds.panel_cache = "window"
    m = build_model(len(vocab), dims, 2, heads, dropout=0.1).to(DEV)
    tr = BERTTrainerWithValidationOptimized(m, None, None, vocab, lr=1e-3, warmup_steps=1, grad_accum_steps=1,
                                            log_freq=0, deterministic=True)
    tr.rag_train_dataset = ds
    tr.rag_k = 4
    K.set_option("dw_xcd", xcd)
    sha = lambda t: hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
    names = {id(p): n for n, p in m.named_parameters()}
    orig_step = tr.optim.step

    def step(grad_scale=1.0):
        if tr.optim.step_count == 0:
            for i, p in enumerate(tr.flat.params):
                print(f"GRAD {names[id(p)]} {sha(tr.flat.view(tr.flat.grad, i))}")
        orig_step(grad_scale)
    tr.optim.step = step
    for s, items in enumerate(([0, 2, 4, 6], [1, 3, 5], [0, 1, 2, 3])):      # one or two window groups
        batch = embedding_rag_collate_fn([ds[i] for i in items])
        loss = tr.train_step(batch)
        data = tr._last[1]
        idx = "-".join(sha(data[k]) for k in ("rag_idx_h1", "rag_idx_h2") if k in data)
        assert idx, "no retrieval in the step"
        print(f"STEP {s} loss {loss.float().view(torch.int32).item()} params {sha(tr.flat.flat)} rag_idx {idx}")
    assert not K.deterministic()        # the trainer restored the option after its steps
    assert K._det_ws, "the deterministic workspace was never used"
    print("DONE", flush=True)


def _run_child(dims, heads, xcd):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(dims), str(heads), str(xcd)],
                       capture_output=True, text=True, timeout=170)
    return r


@pytest.mark.parametrize("dims,heads", [(64, 2), (256, 4)])
def test_whole_step_two_fresh_processes_bitwise_equal(dims, heads):
    a = _run_child(dims, heads, 1)
    assert a.returncode == 0 and "DONE" in a.stdout, (a.returncode, a.stdout[-2000:], a.stderr[-4000:])
    b = _run_child(dims, heads, 0)      # not started when A ended on a signal or its limit (assert / raise above)
    assert b.returncode == 0 and "DONE" in b.stdout, (b.returncode, b.stdout[-2000:], b.stderr[-4000:])
    pick = lambda out, tag: [ln for ln in out.splitlines() if ln.startswith(tag)]
    sa, sb = pick(a.stdout, "STEP"), pick(b.stdout, "STEP")
    assert len(sa) == 3
    ga, gb = pick(a.stdout, "GRAD"), pick(b.stdout, "GRAD")
    diff = [x.split()[1] for x, y in zip(ga, gb) if x != y]
    print("\n".join(sa + sb))
    print(f"d{dims}: {len(diff)} of {len(ga)} parameter gradients differ after the first backward: {diff[:20]}")
    assert len(ga) == len(gb) > 50 and not diff, diff
    assert sa == sb, (sa, sb)


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "child":
    _child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
