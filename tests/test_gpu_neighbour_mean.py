"""The neighbour-mean kernels per element against the float64 restatements of tests/nbr_refs.py
(proved on the CPU by test_nbr_refs_cpu.py): rag_mean_kernel<float | bf16, CNT, BITS> and
neighbor_counts_kernel<BITS> (csrc/knn.hip), nbr_mean_drop_fwd_kernel and
nbr_mean_drop_bwd_kernel<DET> (csrc/train.hip), through the C entry points.

Every case compares every element with ratio(got, ref, bound) <= 1; the bounds come from the
kernels' f32 operation order (nbr_refs docstring) and are 0 on the exact tables, where the result
must match bit for bit.  Outputs are views into the middle of a NaN-filled (0xA5 for u8) storage
and are NaN-filled themselves: an element left unwritten fails its comparison, a write outside the
output changes a guard.  Float inputs are prefix views of NaN-padded storage.

Shapes (nbr_refs tables), the smallest that reach each branch:
  rag_mean   D = 8 / 64 (one 256-thread pass of 16-byte units), 136 (272 f32 units: a pass and a
             partial one), 384 (three passes f32, two bf16); L % 8 in {0, 1, 7}; <eos> on slot 0 and on
             slot 7 of a block, no <pad> position, no sites; nq 1, 15, 16, 17, 33 either side of the 16
             queries of a block; k 1, 8, 128; leading, trailing and only -1 neighbours; Ar absent;
             token ids with tok1 != tok0 + 1 and pad != 0; rows, bit rows and counts longer than the
             window, n_sites % 8 != 0.
  counts     k = 128 with columns of count 128, neighbours at both ends of the shard's row range
             and one outside each, -1, ld_out > ld, more than 256 threads' work, an empty shard.
  nbr fwd    p 0, 0.5 (exact), 0.3 at k > 1; nq 1, 3, 4, 5 (four queries per block) and 257, 260 (the
             grid's query stride); D 2, 64, 126, 128, 130 (64 pairs per pass), 384; a query without
             neighbours; ld_codes > n_sites.
  nbr bwd    D 2, 130, 384, 512 (64, 128, 192, 256 threads), 1024 with V = 16 (two passes, the 64 KiB
             LDS limit), 2048 with V = 8; atomic and deterministic; onto a prior dW and dAr."""
import numpy as np
import pytest
import torch

import nbr_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT_ID = {F32: "f32", BF16: "bf16"}.get
PAD = 64                               # guard elements either side of an output
WORST = {}                             # kernel instantiation -> [worst ratio, cases]


def K():
    from src import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n== worst max err / bound per kernel instantiation (cases) ==")
    for name, (r, n) in sorted(WORST.items()):
        print(f"{name:<52s} {r:.3f}  ({n})")


def _note(kernel, what, r):
    print(f"{kernel} {what}: max err/bound {r:.3f}")
    w = WORST.setdefault(kernel, [0.0, 0])
    w[0], w[1] = max(w[0], r), w[1] + 1


def _in(a, pad=PAD):
    """device copy of a numpy input; a float one is a prefix view of storage that goes on with NaNs"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not t.dtype.is_floating_point:
        return t.to(DEV)
    flat = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype, device=DEV)
    flat[:t.numel()] = t.reshape(-1).to(DEV)
    return flat[:t.numel()].view(t.shape)


def _out(shape, dtype, init=None):
    """(storage, view): the output in the middle of guard elements; NaN / 0xA5 throughout unless
    ``init`` (a prior to accumulate onto) is given"""
    n = int(np.prod(shape))
    fill = 0xA5 if dtype == torch.uint8 else float("nan")
    flat = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    view = flat[PAD:PAD + n].view(shape)
    if init is not None:
        view.copy_(torch.from_numpy(init).to(DEV))
    return flat, view


def _guards_intact(flat):
    g = torch.cat([flat[:PAD], flat[-PAD:]])
    return bool((g == 0xA5).all()) if flat.dtype == torch.uint8 else bool(torch.isnan(g).all())


# ------------------------------------------------------------------ rag_mean --
@pytest.mark.parametrize("dt", [F32, BF16], ids=DT_ID)
@pytest.mark.parametrize("mode", ["rows", "bits", "counts"])
@pytest.mark.parametrize("name", R.RAG_NAMES)
def test_rag_mean_vs_fp64(name, mode, dt):
    c = R.rag_case(name)
    ref, bound = R.rag_expected(c, mode, dt == BF16)
    flat, out = _out((c.nq, c.L, c.D), dt)
    src = _in(R.rag_src(c, mode))
    K().rag_mean(_in(c.idx), src, c.n_sites, _in(c.W), _in(c.pe), None if c.Ar is None else _in(c.Ar), c.L, dt,
                 out=out, counts=src if mode == "counts" else None, bits=mode == "bits", **c.ids)
    torch.cuda.synchronize()
    r = R.ratio(out.float(), ref, bound)
    _note(f"rag_mean_kernel<{DT_ID(dt)}, CNT={int(mode == 'counts')}, BITS={int(mode == 'bits')}>",
          f"{name}{' exact' if c.exact else ''}", r)
    assert _guards_intact(flat), "write outside the output"
    assert r <= 1


# ------------------------------------------------------------ neighbor_counts --
@pytest.mark.parametrize("bits", [False, True], ids=["u8", "bits"])
@pytest.mark.parametrize("name", R.COUNT_NAMES)
def test_neighbor_counts_exact(name, bits):
    c = R.count_case(name)
    ref = R.neighbor_counts(c.idx, c.bits if bits else c.rows, c.row0, c.n_rows, c.ld_out, bits=bits)
    assert ref.max() <= 128 and (name != "k128_full" or (ref == 128).any())
    flat, out = _out((c.nq, c.ld_out), torch.uint8)
    K().neighbor_counts(_in(c.idx), _in(c.bits if bits else c.rows), c.row0, c.ld_out, out=out, bits=bits)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.int64)
    bad = np.argwhere(got != ref)
    _note(f"neighbor_counts_kernel<BITS={int(bits)}>", name, float("inf") if len(bad) else 0.0)
    assert _guards_intact(flat), "write outside the output"
    assert not len(bad), f"{len(bad)} of {ref.size} counts differ, first at {bad[0].tolist()}"
    assert not got[:, c.ld:].any()


# ------------------------------------------------------ nbr_mean_drop forward --
@pytest.mark.parametrize("name", R.FWD_NAMES)
def test_nbr_mean_drop_forward_vs_fp64(name):
    c = R.fwd_case(name)
    ref, bound = R.fwd_expected(name)
    k = K()
    flat, out = _out((c.nq, c.L, c.D), F32)
    a = [_in(t) for t in (c.inv, c.codes, c.W, c.pe, c.Ar)]
    k.check(k.N.lib().snvrag_nbr_mean_drop_fwd(c.nq, c.k, c.L, c.D, c.n_sites, c.codes.shape[1], c.V,
                                               *[k.ptr(t) for t in a], float(c.p), c.seed & (2 ** 64 - 1),
                                               c.ids["tok0"], c.ids["sos"], c.ids["eos"], c.ids["pad"], k.ptr(out),
                                               k.stream_ptr()), "nbr_mean_drop_fwd")
    torch.cuda.synchronize()
    r = R.ratio(out, ref, bound)
    _note("nbr_mean_drop_fwd_kernel", name, r)
    assert _guards_intact(flat), "write outside the output"
    assert r <= 1
    via = k.nbr_mean_drop(*a[:2], c.n_sites, *a[2:], c.p, c.seed, **{i: c.ids[i] for i in ("tok0", "sos", "eos", "pad")})
    assert torch.equal(via, out), "the wrapper passes other arguments than the direct call"


# ----------------------------------------------------- nbr_mean_drop backward --
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", R.BWD_NAMES)
def test_nbr_mean_drop_backward_vs_fp64(name, det):
    c = R.bwd_case(name)
    dW, dAr, bW, bAr = R.bwd_expected(name)
    k = K()
    fW, gW = _out((c.V, c.D), F32, c.dW0)
    fA, gA = _out((c.L, c.D), F32, c.dAr0)
    ids = {i: c.ids[i] for i in ("tok0", "sos", "eos", "pad")}
    with k.option("deterministic", int(det)):
        k.nbr_mean_drop_bwd(_in(c.dout), _in(c.inv), _in(c.codes), c.n_sites, _in(c.W), _in(c.pe), _in(c.Ar), c.p,
                            c.seed, gW, gA, **ids)
    torch.cuda.synchronize()
    rW, rA = R.ratio(gW, dW, bW), R.ratio(gA, dAr, bAr)
    _note(f"nbr_mean_drop_bwd_kernel<DET={int(det)}> dW", name, rW)
    _note(f"nbr_mean_drop_bwd_kernel<DET={int(det)}> dAr", name, rA)
    assert _guards_intact(fW) and _guards_intact(fA), "write outside dW or dAr"
    assert rW <= 1 and rA <= 1
    assert not gW[c.ids["pad"]].any(), "the <pad> row got a gradient"
