"""kNN parity at the launch shapes the benchmark and large batches actually run.

The bench (configs[2]) searches 512 query haplotypes against a 1,000,000-haplotype,
1024-site panel: 32 query tiles -> G = 4 co-scheduled query groups sharing each panel
range (csrc/knn.hip scan2_kernel slot/group/part mapping), the n_parts >= 256 branch of
``scan_parts`` and the threshold pre-pass over a 1/64 panel prefix.  Every case here
compares the device top-k keys with the ORACLE run end to end on the host copy of the same
panel: Delta in the device's f32 arithmetic (``knn_np.lut_delta_f32``, oracle/lut_f32.c) ->
``quantize_lut`` (asserted equal to the device's LUT bit for bit) -> ``knn_np.knn``
(float64-exact (distance, index) order); sampled queries cover every query group.

Cases:
  * bench shape:   N = 1,000,000, 1024 sites, 512 queries (G = 4), aligned masks (the
                   one-limb reduced scan), the bench's own workload generator;
  * ragged:        N = 600,000, 1000 sites, 200 queries (G = 2, last tile half full),
                   misaligned query masks (two-limb scan);
  * Aq != Ar:      N = 200,000, 96 queries whose AF embedding differs from the panel's
                   (the exact-LUT path of embedding_rag_dataset.py:193-196), checked LUT
                   and keys;
  * 8-way shards:  the per-rank launch shape of configs[3] on one GPU: 4096 all-gathered
                   queries (G = 32 query groups) against panel shards with a non-zero
                   ref_offset and a part count that is no multiple of 8 (160,000 rows in 8
                   shards, one limb; 40,000 rows in 3 unequal shards, 3000 ragged queries, two
                   limbs; rank 3's 125,000 rows of the 1M panel), the shards' merge against the
                   whole-panel search, and neighbor_counts at the same shape.
Reference behaviour: src/dataset/embedding_rag_dataset.py:390-402 (cdist + topk).
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from knn_helpers import decode_lut, lut_wide_flag
from oracle import knn_np

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sample_queries(nq, per_group=8, seed=0):
    """Queries spread over every 128-query group (and both ends of the last tile)."""
    rng = np.random.default_rng(seed)
    out = []
    for g0 in range(0, nq, 128):
        g1 = min(nq, g0 + 128)
        pick = rng.choice(np.arange(g0, g1), size=min(per_group, g1 - g0), replace=False)
        out += sorted(set(pick.tolist()) | {g0, g1 - 1})
    return np.array(sorted(set(out)))


def _oracle_lut(tok, W, site_mask, exps, lut, nq, n_sites_pad, sample, limbs=2, **offsets):
    """The oracle's LUT of the sampled queries (f32 Delta in the device's order -> quantised),
    asserted equal to the device's LUT and exponents."""
    n_sites = site_mask.shape[0]
    dq_o, e_o = knn_np.quantize_lut(knn_np.lut_delta_f32(W, tok[sample], site_mask, **offsets), limbs)
    np.testing.assert_array_equal(exps.cpu().numpy()[sample], e_o)
    np.testing.assert_array_equal(decode_lut(lut, nq, n_sites_pad, limbs)[sample, :n_sites], dq_o)
    return dq_o


def _check_sampled(index, dq_o, keys, idx, sample, k):
    """Device keys/indices of the sampled queries == the oracle's top-k (from the oracle's own
    LUT ``dq_o``) on the host panel copy (a shard's rows: indices offset by its ``ref_offset``)."""
    codes = index.codes.cpu().numpy()[:, :index.n_sites]
    oi, od = knn_np.knn(codes, dq_o, k)
    oi = np.where(oi >= 0, oi + index.ref_offset, -1)
    np.testing.assert_array_equal(idx.cpu().numpy()[sample], oi)
    kk = keys.cpu().numpy().view(np.uint64)[sample]
    np.testing.assert_array_equal(kk, knn_np.pack_key(od, oi))
    return oi, od


def test_knn_bench_launch_shape_1m_512q():
    import bench
    from src.dataset import synthetic
    from src.dataset.vocab import WordVocab
    from src.engine import engine_for
    from src.model import build_model
    args = SimpleNamespace(batch=256, n_ref=1_000_000, window=1024, level=4)
    vocab = WordVocab(synthetic.POPS)
    torch.manual_seed(0)
    m = build_model(len(vocab), 384, 1, 12).to(DEV).eval()
    P = engine_for(m).packed()
    wl = bench.build_workload(args, torch.device(DEV), vocab)
    nq, k = wl.tok.shape[0], 32
    assert nq == 512 and ((nq + 15) // 16 + 7) // 8 == 4          # four co-scheduled query groups
    idx, dist, keys, lut, exps = wl.index.search(wl.tok, P.W, wl.site_mask, k, return_keys=True)
    # aligned masks + equal AF: binary Delta -> the device took the reduced one-limb scan
    assert lut_wide_flag(lut, nq, wl.index.n_sites_pad) == 0
    sample = _sample_queries(nq)
    assert len(sample) >= 32 and len({q // 128 for q in sample}) == 4
    dq_o = _oracle_lut(wl.tok.cpu().numpy(), P.W.cpu().numpy(), wl.raw_mask.astype(np.uint8), exps, lut, nq,
                       wl.index.n_sites_pad, sample)
    oi, od = _check_sampled(wl.index, dq_o, keys, idx, sample, k)
    # each query's own source haplotype (2 % flips) is among its nearest neighbours
    src = np.concatenate([wl.src[:, 0], wl.src[:, 1]])[sample]
    assert np.mean([s in row for s, row in zip(src, oi)]) > 0.9
    # the search is deterministic across launches
    idx2, _ = wl.index.search(wl.tok, P.W, wl.site_mask, k)
    torch.testing.assert_close(idx2, idx, rtol=0, atol=0)


def test_knn_ragged_600k_200q_two_limb():
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k = 600_000, 1000, 200, 32
    rng = np.random.default_rng(21)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    index = PanelIndex.synthetic(n_ref, n_sites, af, torch.zeros(1030, device=DEV), seed=5)
    assert index.n_sites_pad == 1024
    codes_h = index.codes[:, :n_sites].cpu().numpy()
    W = torch.from_numpy(rng.standard_normal((12, 64)).astype(np.float32)).to(DEV)
    site_mask = (rng.random(n_sites) < 0.4).astype(np.uint8)
    q_alle = codes_h[rng.integers(0, n_ref, nq)] ^ (rng.random((nq, n_sites)) < 0.03)
    tok = np.zeros((nq, 1030), np.int64)
    tok[:, 0] = 2
    tok[:, 1:1 + n_sites] = np.where(site_mask[None] == 1, 4, 5 + q_alle)
    tok[:, 1 + n_sites] = 3
    tok[:, 1:1 + n_sites][:, rng.random(n_sites) < 0.05] = 4     # query-only masked sites
    smask = torch.from_numpy(site_mask).to(DEV)
    idx, dist, keys, lut, exps = index.search(torch.from_numpy(tok).to(DEV), W, smask, k, return_keys=True)
    assert ((nq + 15) // 16 + 7) // 8 == 2 and nq % 16 == 8
    # the device LUT equals the oracle's (f32 Delta in the device's order) for EVERY query, and
    # is within one quantum of the fp64 Delta's quantisation
    allq = np.arange(nq)
    dq_o = _oracle_lut(tok, W.cpu().numpy(), site_mask, exps, lut, nq, index.n_sites_pad, allq)
    dq_64, _ = knn_np.quantize_lut(knn_np.lut_delta(W.cpu().numpy(), tok, None, site_mask), 2)
    assert np.abs(dq_64 - dq_o).max() <= 1
    sample = _sample_queries(nq, per_group=12, seed=1)
    assert {q // 128 for q in sample} == {0, 1} and nq - 1 in sample
    _check_sampled(index, dq_o[sample], keys, idx, sample, k)


def test_knn_aq_ne_ar_exact_lut():
    """Query AF embedding != panel AF embedding: u = W[tok] + A_q - A_r per position."""
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k, D, L = 200_000, 512, 96, 16, 64, 1030
    rng = np.random.default_rng(4)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    index = PanelIndex.synthetic(n_ref, n_sites, af, torch.zeros(L, device=DEV), seed=9)
    codes_h = index.codes[:, :n_sites].cpu().numpy()
    W = rng.standard_normal((12, D)).astype(np.float32)
    period = nq // 2                                               # A_q rows repeat (h1 | h2 of a sample)
    Aq = (0.3 * rng.standard_normal((period, L, D))).astype(np.float32)
    Ar = (0.3 * rng.standard_normal((L, D))).astype(np.float32)
    site_mask = (rng.random(n_sites) < 0.3).astype(np.uint8)
    q_alle = codes_h[rng.integers(0, n_ref, nq)] ^ (rng.random((nq, n_sites)) < 0.05)
    tok = np.zeros((nq, L), np.int64)
    tok[:, 0], tok[:, 1 + n_sites] = 2, 3
    tok[:, 1:1 + n_sites] = np.where(site_mask[None] == 1, 4, 5 + q_alle)
    T = lambda a: torch.from_numpy(a).to(DEV)
    idx, dist, keys, lut, exps = index.search(T(tok), T(W), T(site_mask), k, Aq=T(Aq), aq_period=period, Ar=T(Ar),
                                              return_keys=True)
    sample = np.arange(nq)
    # real-valued Delta: the oracle's f32 restatement of lut_delta_kernel (u = (W + A_q) - A_r)
    # gives the device's LUT bit for bit, and its top-k the device's indices
    dq_o = _oracle_lut(tok, W, site_mask, exps, lut, nq, index.n_sites_pad, sample, Aq=Aq, aq_period=period, Ar=Ar)
    dA = Aq[np.arange(nq) % period] - Ar[None]
    dq_64, _ = knn_np.quantize_lut(knn_np.lut_delta(W, tok, dA, site_mask), 2)
    assert np.abs(dq_64 - dq_o).max() <= 1
    assert lut_wide_flag(lut, nq, index.n_sites_pad) == 1           # real-valued Delta: two limbs
    _check_sampled(index, dq_o, keys, idx, sample, k)


def test_knn_quantised_lut_vs_exact_fp64_l2_reorder_bound():
    """What the 14-bit LUT quantisation costs against the reference's real-valued distances,
    with real-valued Delta (A_q != A_r, as for train-mode dropped-out queries or a stale panel
    snapshot) at N = 200 000: for every query the exact float64 distance
    dist(q, r) = C_q + sum_s Delta_q[s] a_r[s] (the reference's cdist^2 up to C_q,
    embedding_rag_dataset.py:390-402) is recomputed over the WHOLE panel and its true top-k
    taken.  Guarantee (rigorous): the device's picks are the exact top-k of the quantised
    distances, which differ from the exact ones by at most eps_q = sum_s |Delta_q[s] -
    dq[s] 2^-e| — so every device pick lies within eps_q of the true k-th distance and every
    true neighbour closer than the k-th by more than 2 eps_q is picked.  Reported: how many
    picks differ from the exact fp64 order (near-ties inside the bound); bounded at 1 %."""
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k, D, L = 200_000, 512, 96, 16, 64, 1030
    rng = np.random.default_rng(40)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    index = PanelIndex.synthetic(n_ref, n_sites, af, torch.zeros(L, device=DEV), seed=19)
    codes = index.codes[:, :n_sites]
    codes_h = codes.cpu().numpy()
    W = rng.standard_normal((12, D)).astype(np.float32)
    Aq = (0.3 * rng.standard_normal((nq, L, D))).astype(np.float32)
    Ar = (0.3 * rng.standard_normal((L, D))).astype(np.float32)
    site_mask = (rng.random(n_sites) < 0.3).astype(np.uint8)
    q_alle = codes_h[rng.integers(0, n_ref, nq)] ^ (rng.random((nq, n_sites)) < 0.05)
    tok = np.zeros((nq, L), np.int64)
    tok[:, 0], tok[:, 1 + n_sites] = 2, 3
    tok[:, 1:1 + n_sites] = np.where(site_mask[None] == 1, 4, 5 + q_alle)
    T = lambda a: torch.from_numpy(a).to(DEV)
    idx, _, keys, lut, exps = index.search(T(tok), T(W), T(site_mask), k, Aq=T(Aq), aq_period=nq, Ar=T(Ar),
                                           return_keys=True)
    delta = knn_np.lut_delta(W, tok, Aq - Ar[None], site_mask)                    # float64 [nq, S]
    dq = decode_lut(lut, nq, index.n_sites_pad, 2)[:, :n_sites].astype(np.float64)
    scale = np.exp2(-exps.cpu().numpy().astype(np.float64))
    eps = np.abs(delta - dq * scale[:, None]).sum(1)                              # per-query bound
    # exact float64 distances over the whole panel (the C_q constant cancels in every order)
    exact = torch.from_numpy(delta).to(DEV) @ codes.to(torch.float64).t()          # [nq, N]
    ex_sorted = torch.sort(exact, 1).values
    kth = ex_sorted[:, k - 1].cpu().numpy()
    picks = torch.gather(exact, 1, idx).cpu().numpy()
    assert (picks <= kth[:, None] + eps[:, None] + 1e-9).all()
    # every neighbour closer than the k-th by more than 2 eps is picked
    true_sets = torch.topk(exact, k, 1, largest=False).indices.cpu().numpy()
    ex_np = exact.cpu().numpy()
    idx_np = idx.cpu().numpy()
    missed_clear = 0
    for q in range(nq):
        must = true_sets[q][ex_np[q, true_sets[q]] < kth[q] - 2 * eps[q]]
        missed_clear += len(set(must.tolist()) - set(idx_np[q].tolist()))
    assert missed_clear == 0
    # how often the quantised order differs from the exact one (near-ties inside the bound)
    diff = sum(len(set(true_sets[q].tolist()) ^ set(idx_np[q].tolist())) // 2 for q in range(nq))
    dist_diff = np.abs(np.sort(picks, 1) - ex_sorted[:, :k].cpu().numpy())
    print(f"quantised vs exact fp64 top-{k}: {diff} of {nq * k} picks differ "
          f"({100.0 * diff / (nq * k):.3f} %), max |distance gap| {dist_diff.max():.3e}, "
          f"median bound eps {np.median(eps):.3e}, median k-th distance gap to k+1 "
          f"{np.median((ex_sorted[:, k] - ex_sorted[:, k - 1]).cpu().numpy()):.3e}")
    assert diff <= 0.01 * nq * k
    assert (dist_diff <= 2 * eps[:, None] + 1e-9).all()


# ----------------------------------------------- 8-way-sharded launch shape (configs[3]) --
# Each of 8 ranks searches the all-gathered 8 x 512 = 4096 query haplotypes against its own
# 125 000-haplotype shard: G = 32 co-scheduled query groups (csrc/knn.hip launch_scan2) over a
# small-panel part count from scan_parts that is no multiple of 8, so scan2_kernel's
# `part >= n_parts` early return is live in the last slot row of every group.
def _groups(nq):
    return ((nq + 15) // 16 + 7) // 8


def _query_tokens(rows, site_mask, rng, flips, query_masked=0.0, L=1030):
    """Query tokens [nq, L] copied from panel ``rows`` with a fraction ``flips`` of the alleles
    flipped, masked where the panel is; ``query_masked``: a further fraction of the sites masked
    in the queries only (misaligned masks: real-valued Delta, the two-limb scan)."""
    nq, n_sites = rows.shape
    alle = rows ^ (rng.random((nq, n_sites)) < flips)
    tok = np.zeros((nq, L), np.int64)
    tok[:, 0], tok[:, 1 + n_sites] = 2, 3
    tok[:, 1:1 + n_sites] = np.where(site_mask[None] == 1, 4, 5 + alle)
    if query_masked:
        tok[:, 1:1 + n_sites][:, rng.random(n_sites) < query_masked] = 4
    return tok


def _check_shards(index, bounds, lut, nq, k, dq_o, sample):
    """Every shard [a, b) of ``index`` (row slices of the same codes tensor, ref_offset = a): the
    scan's part count is no multiple of 8 and the sampled queries' keys equal the oracle's on the
    shard's host rows.  Returns the shards' merged keys [n_shards, nq, k]."""
    from src import kernels as K
    from src.retrieval import PanelIndex
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        sh = PanelIndex(index.codes[a:b], index.n_sites, index.ref_af, ref_offset=a, n_total=index.n_ref)
        parts = K.knn_scan(sh.codes, sh.n_sites_pad, lut, nq, 2, k, sh.ref_offset)
        assert parts.shape[0] % 8 != 0, parts.shape
        keys = K.topk_merge(parts, k)
        _check_sampled(sh, dq_o, keys, K.knn_decode(keys)[0], sample, k)
        out.append(keys)
    return torch.stack(out)


def _check_merge(index, shard_keys, lut, nq, k):
    """topk_merge of the shards' keys == one scan_keys over the whole panel == a plain NumPy
    merge of the lists (keys are unique: each carries its index), bit for bit."""
    from src import kernels as K
    from src import native
    assert native.lib().snvrag_knn_scan_parts(index.n_ref, nq) % 8 != 0
    merged = K.topk_merge(shard_keys, k)
    assert torch.equal(merged, index.scan_keys(lut, nq, 2, k))
    np.testing.assert_array_equal(merged.cpu().numpy().view(np.uint64),
                                  knn_np.merge_partials(shard_keys.cpu().numpy().view(np.uint64), k))


def test_knn_32_query_groups_8_shards_one_limb():
    """4096 queries = G = 32 query groups (launch_scan2: G = ceil(nq / 128)) over 8 contiguous
    20 000-row shards of a 160 000 x 1020 panel, each with its own ref_offset: 10 parts per shard
    (scan_parts' small-panel branch; asserted n_parts % 8 != 0), aligned masks = the reduced
    one-limb scan.  Sampled queries of all 32 groups == the oracle on every shard; the merged
    shards == the whole-panel search (>= SAMPLE_MIN: threshold pre-pass at G = 32, 79 parts)."""
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k = 160_000, 1020, 4096, 32
    rng = np.random.default_rng(61)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    index = PanelIndex.synthetic(n_ref, n_sites, af, torch.zeros(1030, device=DEV), seed=23)
    assert index.n_sites_pad == 1024 and n_ref >= index.SAMPLE_MIN
    W = rng.standard_normal((12, 64)).astype(np.float32)
    site_mask = (rng.random(n_sites) < 0.4).astype(np.uint8)
    rows = index.codes[torch.from_numpy(rng.integers(0, n_ref, nq)).to(DEV), :n_sites].cpu().numpy()
    tok = _query_tokens(rows, site_mask, rng, 0.03)
    lut, exps, _ = index.lut(torch.from_numpy(tok).to(DEV), torch.from_numpy(W).to(DEV),
                             torch.from_numpy(site_mask).to(DEV), 2)
    assert _groups(nq) == 32 and lut_wide_flag(lut, nq, index.n_sites_pad) == 0
    sample = _sample_queries(nq, per_group=2, seed=2)
    assert {q // 128 for q in sample} == set(range(32))
    dq_o = _oracle_lut(tok, W, site_mask, exps, lut, nq, index.n_sites_pad, sample)
    shard_keys = _check_shards(index, list(range(0, n_ref + 1, 20_000)), lut, nq, k, dq_o, sample)
    assert shard_keys.shape == (8, nq, k)
    _check_merge(index, shard_keys, lut, nq, k)


def test_knn_ragged_3000q_24_groups_3_shards_two_limb():
    """3000 queries = 24 query groups, the last tile half full (nq % 16 == 8) and the last group
    partly empty (4 of 8 tiles), misaligned query masks (two-limb scan) over 3 unequal shards of a
    40 000 x 500 panel (KS = 8), part counts no multiple of 8; k = 5 (merge_group pads k to 8)."""
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k = 40_000, 500, 3000, 5
    rng = np.random.default_rng(62)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    index = PanelIndex.synthetic(n_ref, n_sites, af, torch.zeros(1030, device=DEV), seed=29)
    assert index.n_sites_pad == 512
    W = rng.standard_normal((12, 64)).astype(np.float32)
    site_mask = (rng.random(n_sites) < 0.4).astype(np.uint8)
    rows = index.codes[torch.from_numpy(rng.integers(0, n_ref, nq)).to(DEV), :n_sites].cpu().numpy()
    tok = _query_tokens(rows, site_mask, rng, 0.03, query_masked=0.05)
    lut, exps, _ = index.lut(torch.from_numpy(tok).to(DEV), torch.from_numpy(W).to(DEV),
                             torch.from_numpy(site_mask).to(DEV), 2)
    assert _groups(nq) == 24 and nq % 16 == 8 and (nq + 15) // 16 % 8 == 4
    assert lut_wide_flag(lut, nq, index.n_sites_pad) == 1
    sample = _sample_queries(nq, per_group=3, seed=3)
    assert {q // 128 for q in sample} == set(range(24)) and nq - 1 in sample
    dq_o = _oracle_lut(tok, W, site_mask, exps, lut, nq, index.n_sites_pad, sample)
    shard_keys = _check_shards(index, [0, 9_000, 27_016, n_ref], lut, nq, k, dq_o, sample)
    _check_merge(index, shard_keys, lut, nq, k)


def test_knn_per_rank_shard_125k_4096q():
    """The true per-rank shape of the 8-way-sharded bench panel, once: rank 3's rows
    [375 000, 500 000) of the 1M x 1024 panel (generated in place with row0), 4096 queries
    (G = 32), ref_offset = 375 000: 62 parts (asserted n_parts % 8 != 0).  Sampled queries of all
    32 groups == the oracle on the host copy; a second launch returns identical keys."""
    from src import kernels as K
    from src.retrieval import PanelIndex
    n_total, row0, n_rows, n_sites, nq, k = 1_000_000, 375_000, 125_000, 1024, 4096, 32
    rng = np.random.default_rng(63)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    codes = K.panel_synth(n_rows, n_sites, af, seed=7, row0=row0)
    sh = PanelIndex(codes, n_sites, torch.zeros(1030, device=DEV), ref_offset=row0, n_total=n_total)
    assert sh.n_sites_pad == 1024 == codes.shape[1]
    W = rng.standard_normal((12, 64)).astype(np.float32)
    site_mask = (rng.random(n_sites) < 0.4).astype(np.uint8)
    rows = codes[torch.from_numpy(rng.integers(0, n_rows, nq)).to(DEV)].cpu().numpy()
    tok = _query_tokens(rows, site_mask, rng, 0.02)
    lut, exps, _ = sh.lut(torch.from_numpy(tok).to(DEV), torch.from_numpy(W).to(DEV),
                          torch.from_numpy(site_mask).to(DEV), 2)
    assert _groups(nq) == 32
    parts = K.knn_scan(codes, sh.n_sites_pad, lut, nq, 2, k, row0)
    assert parts.shape[0] % 8 != 0, parts.shape
    keys = K.topk_merge(parts, k)
    sample = _sample_queries(nq, per_group=2, seed=4)
    assert {q // 128 for q in sample} == set(range(32))
    dq_o = _oracle_lut(tok, W, site_mask, exps, lut, nq, sh.n_sites_pad, sample)
    oi, _ = _check_sampled(sh, dq_o, keys, K.knn_decode(keys)[0], sample, k)
    assert oi.min() >= row0 and oi.max() < row0 + n_rows
    assert torch.equal(sh.scan_keys(lut, nq, 2, k), keys)


def test_neighbor_counts_4096q_on_offset_shard():
    """neighbor_counts at the sharded step's shape (nq = 4096, k = 32) on a shard with row0 != 0:
    global indices inside the shard, outside it on both sides and -1, vs a NumPy gather-and-sum
    over the shard's rows, bit for bit; a counts row longer than the codes row is zero past it."""
    from src import kernels as K
    nq, k, n_sites, row0, n_rows, n_total = 4096, 32, 1020, 15_000, 5_000, 40_000
    rng = np.random.default_rng(64)
    af = torch.from_numpy(rng.beta(0.3, 3.0, n_sites).astype(np.float32)).to(DEV)
    codes = K.panel_synth(n_rows, n_sites, af, seed=3, row0=row0)
    idx = rng.integers(0, n_total, (nq, k))
    idx[rng.random((nq, k)) < 0.1] = -1
    idx[7] = -1                                                    # no neighbour at all
    idx[9] = rng.integers(row0, row0 + n_rows, k)                  # all k in this shard
    idx[11, :2] = [row0, row0 + n_rows - 1]                        # the shard's first and last row
    idx[12, :2] = [row0 - 1, row0 + n_rows]                        # just outside on both sides
    own = (idx >= row0) & (idx < row0 + n_rows)
    assert own.any() and ((idx >= 0) & (idx < row0)).any() and (idx >= row0 + n_rows).any() and (idx < 0).any()
    codes_h = codes.cpu().numpy()
    ref = (codes_h[np.where(own, idx - row0, 0)] * own[..., None]).sum(1).astype(np.uint8)
    idx_d = torch.from_numpy(idx).to(DEV)
    np.testing.assert_array_equal(K.neighbor_counts(idx_d, codes, row0).cpu().numpy(), ref)
    wide = K.neighbor_counts(idx_d, codes, row0, ld_out=codes.shape[1] + 16).cpu().numpy()
    np.testing.assert_array_equal(wide[:, :codes.shape[1]], ref)
    assert (wide[:, codes.shape[1]:] == 0).all()
