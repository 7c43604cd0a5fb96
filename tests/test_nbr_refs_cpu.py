"""CPU proof of tests/nbr_refs.py, which test_gpu_neighbour_mean.py holds the kernels to:

  * the float64 references equal the materialised form: rag_mean the mean over the valid neighbours
    of W[tok] + pe + Ar written as a loop; nbr_mean_drop and its adjoint torch's float64 autograd of
    E = (W[tok] + pe + Ar) keep scale averaged per query, at p = 0 and p > 0;
  * the float32 emulation of each kernel's documented order stays inside the bound on every table
    of the GPU tests and equals the reference bit for bit on the exact ones;
  * every planted fault pushes at least one element past its bound on every table it is planted in
    (a fault cannot show where it changes nothing: see RAG_FAULT_TABLES);
  * conditions of the tables: every dropout table has kept and dropped elements at every position,
    every bound covers every element (full shape, finite, no element masked out), the launch edges
    that the shapes are there for are the ones they reach."""
import numpy as np
import pytest
import torch

import nbr_refs as R

F64, F32 = R.F64, R.F32
MODES = ("rows", "bits", "counts")


# ------------------------------------------------------------ the references --
@pytest.mark.parametrize("ids", [R.IDS, R.IDS_ALT], ids=["ids", "alt_ids"])
@pytest.mark.parametrize("has_ar", [True, False])
def test_rag_mean_reference_is_the_mean_of_embeddings(ids, has_ar):
    g = np.random.default_rng(5)
    nq, k, L, D, n, n_ref = 6, 5, 9, 8, 6, 20
    W, pe, Ar = g.standard_normal((10, D)), g.standard_normal((L, D)), g.standard_normal((L, D))
    rows = g.integers(0, 2, size=(n_ref, 16)).astype(np.uint8)
    idx = g.integers(0, n_ref, size=(nq, k))
    idx[1, :3] = -1
    idx[2, 2:] = -1
    idx[3] = -1
    want = np.zeros((nq, L, D))
    for q in range(nq):
        v = idx[q][idx[q] >= 0]
        for l in range(L):
            if l == 0 or l > n:
                e = W[ids["sos"] if l == 0 else ids["eos"] if l == n + 1 else ids["pad"]]
            elif len(v):
                e = np.mean([W[ids["tok1"] if rows[r, l - 1] else ids["tok0"]] for r in v], axis=0)
            else:
                e = 0.0
            want[q, l] = e + pe[l] + (Ar[l] if has_ar else 0)
    counts = np.stack([rows[idx[q][idx[q] >= 0]].sum(0) for q in range(nq)]).astype(np.uint8)
    for mode, src in zip(MODES, (rows, R.pack_bits(rows), counts)):
        got = R.rag_mean(idx, src, n, W, pe, Ar if has_ar else None, L, ids, mode)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-14, err_msg=mode)


def test_neighbor_counts_reference():
    g = np.random.default_rng(6)
    rows = g.integers(0, 2, size=(7, 16)).astype(np.uint8)
    idx = np.array([[99, 100, 106, 107, -1, 103, 103]])
    want = rows[0] + rows[6] + 2 * rows[3]
    for bits in (False, True):
        got = R.neighbor_counts(idx, R.pack_bits(rows) if bits else rows, 100, 7, 48, bits=bits)
        assert got.shape == (1, 48) and (got[0, :16] == want).all() and not got[0, 16:].any()
    full = np.ones((128, 16), np.uint8)
    all_rows = np.arange(128)[None]
    assert (R.neighbor_counts(all_rows, full, 0, 128, 16, packed_bytes=True) == 128).all()   # no carry at k = 128


def _torch_materialised(c, W, Ar):
    tok = torch.from_numpy(R.nbr_tokens(c.codes, c.n_sites, c.L, c.ids))
    m = torch.from_numpy(R.nbr_keep(c.seed, c.U, c.L, c.D, c.p).astype(F64) * R.drop_scale(c.p))
    E = (W[tok] + torch.from_numpy(c.pe.astype(F64)) + Ar) * m
    return torch.stack([E[torch.from_numpy(v[v >= 0]).long()].mean(0) if (v >= 0).any()
                        else torch.zeros(c.L, c.D, dtype=torch.float64) for v in c.inv])


@pytest.mark.parametrize("name", ["d2-p0", "d2-p0.3", "d130-p0", "d130-p0.3", "d384-p0.5_exact"])
def test_nbr_references_equal_autograd(name):
    c = R.bwd_case(name)
    W = torch.from_numpy(c.W.astype(F64)).requires_grad_(True)
    Ar = torch.from_numpy(c.Ar.astype(F64)).requires_grad_(True)
    out = _torch_materialised(c, W, Ar)
    ref = R.nbr_mean_drop(c.inv, c.codes, c.n_sites, c.W, c.pe, c.Ar, c.p, c.seed, c.ids)
    assert np.abs(out.detach().numpy() - ref).max() <= 1e-13
    out.backward(torch.from_numpy(c.dout.astype(F64)))
    want_w = W.grad.numpy().copy()
    want_w[c.ids["pad"]] = 0                                     # nn.Embedding(padding_idx): no gradient
    dW, dAr = R.nbr_mean_drop_bwd(c.dout, c.inv, c.codes, c.n_sites, c.V, c.p, c.seed, c.ids)
    assert np.abs(dW - want_w).max() <= 1e-12 and np.abs(dAr - Ar.grad.numpy()).max() <= 1e-12
    aW, aAr = R.nbr_mean_drop_bwd(c.dout, c.inv, c.codes, c.n_sites, c.V, c.p, c.seed, c.ids, c.dW0, c.dAr0)
    assert np.abs(aW - (dW + c.dW0)).max() <= 1e-12 and np.abs(aAr - (dAr + c.dAr0)).max() <= 1e-12


def test_keep_mask_halves_and_constants():
    """feature d uses half d & 1 of the pair's hash; p = 0.5 gives scale 2; p = 0 keeps all"""
    k = R.nbr_keep(R.SEED, 3, 4, 6, 0.3)
    flat = R.ln_keep_mask(R.SEED, R.NBR_STREAM, 3, 24, 0.3)
    assert k.shape == (3, 4, 6) and (k[1, 2, 5] == flat[1, 2 * 6 + 5]) and (k.reshape(3, 24) == flat).all()
    sw = R.nbr_keep(R.SEED, 3, 4, 6, 0.3, wrong_half=True)
    assert (sw[..., 0::2] == k[..., 1::2]).all() and (sw[..., 1::2] == k[..., 0::2]).all()
    assert R.drop_scale(0.5) == 2.0 and R.drop_scale(0.0) == 1.0
    assert R.drop_scale(0.3) == float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    assert R.nbr_keep(R.SEED, 2, 3, 4, 0.0).all()


# --------------------------------------------------- emulation inside the bounds --
def _rag_emu(c, mode, bf16, fault=None):
    e = R.rag_mean(c.idx, R.rag_src(c, mode), c.n_sites, c.W, c.pe, c.Ar, c.L, c.ids, mode, dtype=F32, fault=fault,
                   unit=8 if bf16 else 4)
    assert e.dtype == F32
    return R.to_bf16(e) if bf16 else e


def _fwd_emu(c, fault=None):
    return R.nbr_mean_drop(c.inv, c.codes, c.n_sites, c.W, c.pe, c.Ar, c.p, c.seed, c.ids, dtype=F32, fault=fault)


def _bwd_emu(c, fault=None):
    return R.nbr_mean_drop_bwd(c.dout, c.inv, c.codes, c.n_sites, c.V, c.p, c.seed, c.ids, c.dW0, c.dAr0, dtype=F32,
                               fault=fault)


def _covers(bound, ref, exact):
    """every element is compared: a bound of the output's shape, finite, all 0 on an exact table"""
    assert bound.shape == ref.shape and np.isfinite(bound).all() and np.isfinite(ref).all()
    assert (bound >= 0).all() and (not exact or not bound.any())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", R.RAG_NAMES)
def test_rag_mean_emulation_inside_bound(name, mode, bf16):
    c = R.rag_case(name)
    ref, bound = R.rag_expected(c, mode, bf16)
    _covers(bound, ref, c.exact)
    assert c.exact or (bound > 0).all()
    emu = _rag_emu(c, mode, bf16)
    if c.exact:
        assert np.array_equal(emu.astype(F64), ref) and np.abs(ref).max() <= 256 and (ref == np.rint(ref)).all()
    assert R.ratio(emu, ref, bound) <= 1


@pytest.mark.parametrize("name", R.FWD_NAMES)
def test_nbr_forward_emulation_inside_bound(name):
    c = R.fwd_case(name)
    ref, bound = R.fwd_expected(name)
    _covers(bound, ref, c.exact)
    emu = _fwd_emu(c)
    assert emu.dtype == F32 and R.ratio(emu, ref, bound) <= 1
    if c.exact:
        assert np.array_equal(emu.astype(F64), ref) and np.abs(ref).max() < 2 ** 20


@pytest.mark.parametrize("name", R.BWD_NAMES)
def test_nbr_backward_emulation_inside_bound(name):
    c = R.bwd_case(name)
    dW, dAr, bW, bAr = R.bwd_expected(name)
    _covers(bW, dW, c.exact)
    _covers(bAr, dAr, c.exact)
    eW, eAr = _bwd_emu(c)
    assert eW.dtype == eAr.dtype == F32
    assert R.ratio(eW, dW, bW) <= 1 and R.ratio(eAr, dAr, bAr) <= 1
    assert not dW[c.ids["pad"]].any() and not eW[c.ids["pad"]].any()
    if c.exact:
        assert np.array_equal(eW.astype(F64), dW) and np.array_equal(eAr.astype(F64), dAr)


def test_exact_sums_are_order_free():
    """the exact tables' terms are multiples of 1 / 8 whose magnitudes sum below 2^20: every order
    of f32 adds gives the same bits, so the atomic path must match bit for bit too"""
    for name in R.BWD_NAMES:
        c = R.bwd_case(name)
        if not c.exact:
            continue
        aW, aAr = R.nbr_mean_drop_bwd(np.abs(c.dout.astype(F64)), c.inv, c.codes, c.n_sites, c.V, c.p, c.seed, c.ids,
                                      np.abs(c.dW0), np.abs(c.dAr0))
        assert max(aW.max(), aAr.max()) < 2 ** 20
        nv = (c.inv >= 0).sum(1)
        assert all(v == 0 or (v & (v - 1)) == 0 and v <= 8 for v in nv)
        for t in (c.dout, c.dW0, c.dAr0, c.W, c.pe, c.Ar):
            assert (t == np.rint(t)).all()


# -------------------------------------------------------------- planted faults --
# tables where the fault changes what is computed: swapped tokens, a dropped neighbour and a wrong nv
# need sites and neighbours, units past 256 need more than 256 units in a block
RAG_FAULT_TABLES = {
    "tok_swap": ("eos_slot0", "k128_d136", "model_d384", "alt_ids_d384", "alt_ids_d64"),
    "drop_last": ("eos_slot0", "k128_d136", "model_d384", "alt_ids_d384", "alt_ids_d64"),
    "eos_late": R.RAG_NAMES,
    "nv_counts_invalid": ("eos_slot0", "k128_d136", "model_d384", "alt_ids_d384", "alt_ids_d64"),
    "units_past_256": ("k128_d136", "model_d384", "no_sites", "alt_ids_d384"),
}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fault", R.RAG_FAULTS)
def test_rag_mean_planted_fault_is_caught(fault, mode, bf16):
    for name in RAG_FAULT_TABLES[fault]:
        c = R.rag_case(name)
        if fault == "units_past_256" and 8 * c.D // (8 if bf16 else 4) <= 256:
            continue
        ref, bound = R.rag_expected(c, mode, bf16)
        r = R.ratio(_rag_emu(c, mode, bf16, fault), ref, bound)
        assert r > 1, (fault, name, mode, r)


def test_rag_units_fault_needs_the_second_stride():
    """shapes with D = 64 cannot see a fault past the first 256 units of a block"""
    assert 8 * 64 // 4 <= 256 and 8 * 136 // 4 == 272 and 8 * 384 // 4 == 768 and 8 * 384 // 8 == 384
    c = R.rag_case("eos_slot0")
    ref, bound = R.rag_expected(c, "rows", False)
    assert R.ratio(_rag_emu(c, "rows", False, "units_past_256"), ref, bound) == 0


@pytest.mark.parametrize("fault", R.FWD_FAULTS)
def test_nbr_forward_planted_fault_is_caught(fault):
    for name in R.FWD_NAMES:
        c = R.fwd_case(name)
        if fault == "hash_half" and c.p == 0:
            continue
        ref, bound = R.fwd_expected(name)
        r = R.ratio(_fwd_emu(c, fault), ref, bound)
        assert r > 1, (fault, name, r)


@pytest.mark.parametrize("fault", R.BWD_FAULTS)
def test_nbr_backward_planted_fault_is_caught(fault):
    for name in R.BWD_NAMES:
        c = R.bwd_case(name)
        if fault == "hash_half" and c.p == 0:
            continue
        dW, dAr, bW, bAr = R.bwd_expected(name)
        eW, eAr = _bwd_emu(c, fault)
        r = max(R.ratio(eW, dW, bW), R.ratio(eAr, dAr, bAr))
        assert r > 1, (fault, name, r)


# ------------------------------------------------------- conditions of the tables --
@pytest.mark.parametrize("name", [n for n in R.FWD_NAMES + R.BWD_NAMES if not n.endswith("-p0")])
def test_dropout_tables_keep_and_drop_at_every_position(name):
    c = R.fwd_case(name) if name in R.FWD_NAMES else R.bwd_case(name)
    keep = R.keep_of(c)
    for l in range(c.L):
        assert keep[:, l].any() and not keep[:, l].all(), (name, l)
    if c.exact:
        assert c.p == 0.5 and R.drop_scale(c.p) == 2.0


def test_shapes_reach_the_launch_edges():
    rag = {c[0]: c for c in R.RAG_CASES}
    assert {c[4] for c in R.RAG_CASES} == {8, 64, 136, 384}
    assert {c[3] % 8 for c in R.RAG_CASES} == {0, 1, 7} and max(c[3] for c in R.RAG_CASES) <= 80
    assert {c[1] for c in R.RAG_CASES} == {1, 15, 16, 17, 33} and {c[2] for c in R.RAG_CASES} == {1, 8, 128}
    assert (rag["eos_slot0"][5] + 1) % 8 == 0 and (rag["model_d384"][5] + 1) % 8 == 7
    assert (rag["alt_ids_d384"][5] + 1) % 8 == 0 and (rag["one"][5] + 1) % 8 == 7
    assert rag["model_d384"][5] + 2 == rag["model_d384"][3] and rag["no_sites"][5] == 0
    assert any(c[5] % 8 for c in R.RAG_CASES) and any(not c[6] for c in R.RAG_CASES)
    a = R.IDS_ALT
    assert a["tok1"] != a["tok0"] + 1 and a["pad"] != 0
    for name in R.RAG_NAMES:
        c = R.rag_case(name)
        nv = (c.idx >= 0).sum(1)
        assert c.counts.shape[1] > c.n_sites and c.rows.shape[1] > c.n_sites and 8 * c.bits.shape[1] >= c.n_sites
        if c.nq >= 4:
            assert (nv == 0).any() and ((c.idx[:, -1] < 0) & (nv > 0)).any()
            assert c.k == 1 or ((c.idx[:, 0] < 0) & (nv > 0)).any()
        if c.exact:
            assert all(v == 0 or v & (v - 1) == 0 for v in nv)
    cnt = {c[0]: c for c in R.COUNT_CASES}
    assert cnt["two_blocks"][1] * cnt["two_blocks"][4] // 16 > 256 and cnt["no_rows"][6] == 0
    assert cnt["shard_ends"][4] > cnt["shard_ends"][3] and cnt["k128_full"][2] == 128
    c = R.count_case("k128_full")
    assert (R.neighbor_counts(c.idx, c.rows, c.row0, c.n_rows, c.ld_out) == 128).any()
    c = R.count_case("shard_ends")
    assert {c.row0 - 1, c.row0, c.row0 + c.n_rows - 1, c.row0 + c.n_rows, -1} <= set(c.idx[1].tolist())
    assert {s[1] for s in R.FWD_SHAPES} == {1, 3, 4, 5, 257, 260}
    assert {s[4] for s in R.FWD_SHAPES} >= {2, 64, 126, 128, 130, 384}
    assert all((s[3], s[4]) == (4, 8) for s in R.FWD_SHAPES if s[1] > 256)
    nthr = lambda D: min(256, (D // 2 + 63) // 64 * 64)
    assert [nthr(s[4]) for s in R.BWD_SHAPES] == [64, 128, 192, 256, 256, 256]
    assert all(s[3] > s[5] + 2 for s in R.BWD_SHAPES)               # a <pad> position in every backward table
    assert [(s[4], s[7]) for s in R.BWD_SHAPES[4:]] == [(1024, 16), (2048, 8)] and 1024 * 16 == 16384
    for name in R.FWD_NAMES + R.BWD_NAMES:
        c = R.fwd_case(name) if name in R.FWD_NAMES else R.bwd_case(name)
        assert c.codes.shape[1] > c.n_sites and c.k > 1 and (c.nq == 1 or ((c.inv >= 0).sum(1) == 0).any())
