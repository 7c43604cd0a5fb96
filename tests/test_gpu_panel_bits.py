"""Bit-packed panel index on the GPU (csrc/knn.hip, src/retrieval/panel_index.py).

The yardsticks are the host packing (numpy), the u8 index's kernels and ``oracle/knn_np``; every
comparison is bit for bit, since the packed index holds exactly the u8 index's 0/1 alleles:

  * pack / unpack / synth kernels against ``np.packbits(bitorder="little")``;
  * ``knn_scan_bits`` part keys against ``knn_scan``'s with the same ``n_parts``, the merged top-k
    against the oracle's canonical (distance, index) order;
  * ``rag_mean`` / ``neighbor_counts`` reading bit rows against the u8 index's outputs;
  * the product path (eval and train retrieval, one deterministic train step, the inference
    entry point, a 2-way sharded panel over gloo) under ``panel_codes="bits"`` against ``"u8"``.
"""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for _p in (ROOT, os.path.join(ROOT, "rag-snvbert_amd")):       # also when run as the train-step child
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import knn_np  # noqa: E402
from knn_helpers import decode_lut, lut_wide_flag, rand_case  # noqa: E402


def K():
    from src import kernels
    return kernels


def _pad(panel: np.ndarray) -> np.ndarray:
    from src.retrieval import pad_sites
    out = np.zeros((panel.shape[0], pad_sites(panel.shape[1])), np.uint8)
    out[:, :panel.shape[1]] = panel
    return out


def _same(a: torch.Tensor, b: torch.Tensor) -> None:
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# --------------------------------------------------------------------- pack / unpack --
@pytest.mark.parametrize("n,n_sites", [(1, 40), (37, 300), (1000, 1030)])
def test_pack_bits_and_unpack_rows_round_trip(n, n_sites):
    rng = np.random.default_rng(n + n_sites)
    codes = _pad((rng.random((n, n_sites)) < 0.4).astype(np.uint8))
    want = np.packbits(codes, axis=1, bitorder="little")
    dev_codes = torch.from_numpy(codes).to(DEV)
    bits = K().panel_pack_bits(dev_codes)
    np.testing.assert_array_equal(bits.cpu().numpy(), want)
    # every row back, in order
    back = K().panel_unpack_rows(bits, torch.arange(n, device=DEV))
    _same(back, dev_codes)
    # shuffled, repeated, negative and out-of-range entries: those give zero rows
    rows = np.concatenate([rng.permutation(n), [-1, n, n + 5, -7, 0, n - 1]]).astype(np.int64)
    rng.shuffle(rows)
    got = K().panel_unpack_rows(bits, torch.from_numpy(rows).to(DEV)).cpu().numpy()
    ok = (rows >= 0) & (rows < n)
    np.testing.assert_array_equal(got[ok], codes[rows[ok]])
    assert (got[~ok] == 0).all() and (~ok).sum() == 4
    assert K().panel_unpack_rows(bits, torch.zeros(0, dtype=torch.long, device=DEV)).shape == (0, codes.shape[1])


def test_index_pack_and_rows():
    from src.retrieval import PanelIndex
    _, panel, _, _ = rand_case(200, 300, 1, 4)
    u8 = PanelIndex.from_alleles(panel, np.zeros(1030, np.float32), DEV, ref_offset=7, n_total=500)
    host = PanelIndex.from_alleles(panel, np.zeros(1030, np.float32), DEV, ref_offset=7, n_total=500, packed=True)
    pk = u8.pack()
    _same(pk.bits, host.bits)
    assert pk.packed and pk.pack() is pk and (pk.ref_offset, pk.n_total, pk.n_sites) == (7, 500, 300)
    assert pk.nbytes * 8 == u8.nbytes and pk.device == u8.device
    i = torch.tensor([3, 199, 0, 3], device=DEV)
    _same(pk.rows(i), u8.rows(i))
    _same(u8.rows(i), u8.codes[i])


@pytest.mark.parametrize("n_sites", [40, 300, 1030])
def test_panel_synth_bits_equals_packed_panel_synth(n_sites):
    af = torch.rand(n_sites, device=DEV) * 0.6
    for n, row0 in ((257, 0), (100, 1733)):
        codes = K().panel_synth(n, n_sites, af, 11, row0=row0)
        _same(K().panel_synth_bits(n, n_sites, af, 11, row0=row0), K().panel_pack_bits(codes))
    from src.retrieval import PanelIndex
    ref_af = torch.zeros(1030, device=DEV)
    a = PanelIndex.synthetic(300, n_sites, af, ref_af, 5)
    b = PanelIndex.synthetic(300, n_sites, af, ref_af, 5, packed=True)
    _same(b.bits, a.pack().bits)


# ------------------------------------------------------------------------------ scan --
def _scan_case(n_ref, n_sites, nq, limbs, tie, seed, real_delta=False):
    """(u8 index, packed index, lut, oracle LUT integers) of a rand_case."""
    from src.retrieval import PanelIndex
    W, panel, site_mask, tok = rand_case(n_ref, n_sites, nq, seed, tie, L=n_sites + 4)
    u8 = PanelIndex.from_alleles(panel, np.zeros(n_sites + 4, np.float32), DEV)
    pk = PanelIndex.from_alleles(panel, np.zeros(n_sites + 4, np.float32), DEV, packed=True)
    Wt, sm, tq = torch.from_numpy(W).to(DEV), torch.from_numpy(site_mask).to(DEV), torch.from_numpy(tok).to(DEV)
    Aq = Ar = None
    if real_delta:       # A_q != A_r: real-valued Delta, no common divisor
        g = torch.Generator(device="cpu").manual_seed(seed)
        Aq = (0.3 * torch.randn(nq, n_sites + 4, W.shape[1], generator=g)).to(DEV)
        Ar = (0.3 * torch.randn(n_sites + 4, W.shape[1], generator=g)).to(DEV)
    lut, _, _ = u8.lut(tq, Wt, sm, limbs, Aq, nq if real_delta else 0, Ar)
    dq = decode_lut(lut, nq, u8.n_sites_pad, limbs)[:, :n_sites]
    return u8, pk, lut, dq, panel


SCAN_CASES = [
    # n_ref, n_sites, nq, k, limbs, tie
    (1, 40, 1, 1, 1, False), (15, 1024, 17, 32, 2, False), (33, 1030, 200, 1, 2, True),
    (1000, 40, 200, 32, 1, False), (2500, 1024, 17, 32, 2, True), (2500, 1030, 1, 32, 1, True),
    (1000, 1030, 17, 32, 2, False), (2500, 40, 200, 1, 2, False), (15, 40, 200, 32, 2, True),
    (33, 1024, 1, 32, 1, False), (1, 1030, 17, 1, 2, False), (1000, 1024, 200, 1, 1, True),
    (2500, 1024, 200, 32, 2, False), (33, 40, 17, 32, 1, True), (15, 1030, 1, 1, 1, False),
]


@pytest.mark.parametrize("n_ref,n_sites,nq,k,limbs,tie", SCAN_CASES)
def test_scan_bits_keys_equal_u8_scan_and_oracle(n_ref, n_sites, nq, k, limbs, tie):
    """Fewer rows than one 32-row stage, ragged last stages, several ranges; windows padded to
    256 / 1024 / 1280 sites; ragged query tiles and two query groups; k = 1 and 32 (k > n_ref
    gives KEY_MAX pads); both limb counts; the tie-heavy generator, whose binary Delta lets the
    device-decided one-limb reduction fire."""
    u8, pk, lut, dq, panel = _scan_case(n_ref, n_sites, nq, limbs, tie, n_ref + n_sites + nq + k)
    if limbs == 2 and (tie or n_sites >= 1024):      # (a 40-site window may draw no misaligned site)
        assert lut_wide_flag(lut, nq, u8.n_sites_pad) == (0 if tie else 1)
    oi, od = knn_np.knn(panel, dq, k)
    want = knn_np.pack_key(od, oi)
    for n_parts in (None, 3):        # the library's ranges, and three ragged ones
        a = K().knn_scan(u8.codes, u8.n_sites_pad, lut, nq, limbs, k, n_parts=n_parts)
        b = K().knn_scan_bits(pk.bits, pk.n_sites_pad, lut, nq, limbs, k, n_parts=n_parts)
        _same(b, a)
        merged = K().topk_merge(b, k).cpu().numpy().view(np.uint64)
        valid = oi >= 0
        np.testing.assert_array_equal(merged[valid], want[valid])
        assert (merged[~valid] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        assert (~valid).sum() == nq * max(0, k - n_ref)
    _same(pk.scan_keys(lut, nq, limbs, k), u8.scan_keys(lut, nq, limbs, k))


def test_scan_bits_two_limbs_when_the_reduction_cannot_fire():
    """Real-valued Delta (A_q != A_r): the LUT keeps two limbs; also the forced two-limb scan of a
    reducible LUT gives the reduced scan's keys."""
    n_ref, n_sites, nq, k = 1000, 300, 40, 16
    u8, pk, lut, dq, panel = _scan_case(n_ref, n_sites, nq, 2, False, 91, real_delta=True)
    assert lut_wide_flag(lut, nq, u8.n_sites_pad) == 1
    oi, od = knn_np.knn(panel, dq, k)
    keys = pk.scan_keys(lut, nq, 2, k)
    np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), knn_np.pack_key(od, oi))
    _same(keys, u8.scan_keys(lut, nq, 2, k))
    u8, pk, lut, dq, panel = _scan_case(n_ref, n_sites, nq, 2, True, 92)
    assert lut_wide_flag(lut, nq, u8.n_sites_pad) == 0
    reduced = pk.scan_keys(lut, nq, 2, k)
    with K().option("knn_no_reduce", 1):
        _same(pk.scan_keys(lut, nq, 2, k), reduced)


def test_scan_bits_ref_offset_and_shard_merge():
    from src.retrieval import PanelIndex
    n_ref, n_sites, nq, k = 2500, 400, 24, 16
    u8, pk, lut, dq, panel = _scan_case(n_ref, n_sites, nq, 2, True, 5)
    full = u8.scan_keys(lut, nq, 2, k)
    parts = []
    for a, b in ((0, 1000), (1000, 2100), (2100, 2500)):
        sh = PanelIndex.from_alleles(panel[a:b], np.zeros(n_sites + 4, np.float32), DEV, ref_offset=a, packed=True)
        parts.append(sh.scan_keys(lut, nq, 2, k))
        u8s = PanelIndex.from_alleles(panel[a:b], np.zeros(n_sites + 4, np.float32), DEV, ref_offset=a)
        _same(K().knn_scan_bits(sh.bits, sh.n_sites_pad, lut, nq, 2, k, ref_offset=a),
              K().knn_scan(u8s.codes, u8s.n_sites_pad, lut, nq, 2, k, ref_offset=a))
    _same(K().topk_merge(torch.stack(parts), k), full)


@pytest.mark.parametrize("tie", [False, True])
def test_scan_bits_presample_threshold(tie):
    """The threshold pre-pass forced on a 2 500-row panel: th_init reaches the bit scan."""
    n_ref, n_sites, nq, k = 2500, 300, 40, 32
    u8, pk, lut, dq, panel = _scan_case(n_ref, n_sites, nq, 2, tie, 77)
    plain = pk.scan_keys(lut, nq, 2, k, presample=False)
    pre = pk.scan_keys(lut, nq, 2, k, presample=True)
    _same(pre, plain)
    _same(pre, u8.scan_keys(lut, nq, 2, k, presample=True))
    oi, od = knn_np.knn(panel, dq, k)
    np.testing.assert_array_equal(pre.cpu().numpy().view(np.uint64), knn_np.pack_key(od, oi))
    # and the raw entry point with an explicit threshold
    th = K().knn_threshold(plain, k)
    _same(K().knn_scan_bits(pk.bits, pk.n_sites_pad, lut, nq, 2, k, th_init=th),
          K().knn_scan(u8.codes, u8.n_sites_pad, lut, nq, 2, k, th_init=th))


def test_search_on_a_packed_index_equals_u8_search():
    from src.retrieval import PanelIndex
    W, panel, site_mask, tok = rand_case(1500, 500, 30, 8)
    args = (torch.from_numpy(tok).to(DEV), torch.from_numpy(W).to(DEV), torch.from_numpy(site_mask).to(DEV), 8)
    a = PanelIndex.from_alleles(panel, np.zeros(1030, np.float32), DEV).search(*args)
    b = PanelIndex.from_alleles(panel, np.zeros(1030, np.float32), DEV, packed=True).search(*args)
    _same(b[0], a[0])
    _same(b[1], a[1])


# ------------------------------------------------------------------------- consumers --
@pytest.mark.parametrize("n_sites", [300, 1030])
def test_rag_mean_and_neighbor_counts_read_bit_rows(n_sites):
    from src.retrieval import PanelIndex
    rng = np.random.default_rng(9)
    D, L, n_ref, nq, k = 64, 1036, 200, 37, 32
    panel = rng.integers(0, 2, (n_ref, n_sites)).astype(np.uint8)
    u8 = PanelIndex.from_alleles(panel, np.zeros(L, np.float32), DEV, ref_offset=50)
    pk = PanelIndex.from_alleles(panel, np.zeros(L, np.float32), DEV, ref_offset=50, packed=True)
    W, pe, Ar = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
                 for s in ((12, D), (L, D), (L, D)))
    idx = rng.integers(0, n_ref, (nq, k))
    idx[5, 3:] = -1
    idx[nq - 1, :] = -1
    idx = torch.from_numpy(idx).to(DEV)
    for dt in (torch.float32, torch.bfloat16):
        want = u8.rag_mean(idx, W, pe, Ar, L, dt)
        _same(pk.rag_mean(idx, W, pe, Ar, L, dt), want)
        _same(K().rag_mean(idx, u8.codes, n_sites, W, pe, Ar, L, dt), want)
        out = torch.full((nq, L, D), 7.0, device=DEV, dtype=dt)
        assert pk.rag_mean(idx, W, pe, None, L, dt, out=out) is out
        _same(out, u8.rag_mean(idx, W, pe, None, L, dt))
        # the dense one-neighbour form
        one = idx.reshape(-1, 1)
        _same(pk.rag_mean(one, W, pe, Ar, L, dt), u8.rag_mean(one, W, pe, Ar, L, dt))
    # neighbour counts of a shard: global indices, rows outside the shard do not count
    gidx = idx + 50
    gidx[idx < 0] = -1
    gidx[0, :4] = torch.tensor([0, 49, 250, 10 ** 6], device=DEV)
    want = u8.neighbor_counts(gidx)
    _same(pk.neighbor_counts(gidx), want)
    _same(want, K().neighbor_counts(gidx, u8.codes, 50))
    # a counts row wider than the panel row stays zero past it
    wide = K().neighbor_counts(gidx, pk.bits, 50, ld_out=pk.ld + 32, bits=True)
    _same(wide[:, :pk.ld].contiguous(), want)
    assert int(wide[:, pk.ld:].max()) == 0


# ------------------------------------------------------------------------ end to end --
def _tiny(panel_codes, seed=2):
    from src.dataset.synthetic import make_rag_dataset
    from src.model import build_model
    np.random.seed(0)        # the construction-time window masks draw from the global RNG
    ds, vocab = make_rag_dataset(n_samples=6, n_sites=300, n_windows=2, n_ref_samples=40, seed=seed,
                                 panel_codes=panel_codes)
    torch.manual_seed(0)
    m = build_model(len(vocab), 64, 1, 4).to(DEV)
    return ds, m


def _batch(ds, items=(0, 1, 2, 3, 5)):
    from src.dataset.embedding_rag_dataset import embedding_rag_collate_fn
    return embedding_rag_collate_fn([ds[i] for i in items])


def test_process_batch_retrieval_bits_equals_u8():
    """Eval, train mode without dropout, and train mode with dropout under one seed (the gathered
    rows are equal, so the fused neighbour-mean launch sees identical inputs); also the dense form."""
    got = {}
    for pc in ("u8", "bits"):
        ds, m = _tiny(pc)
        emb = m.bert.embedding
        m.eval()
        b = ds.process_batch_retrieval(_batch(ds), emb, DEV, k_retrieve=4)
        assert ds.panel_index(0, DEV).packed == (pc == "bits")
        d = ds.process_batch_retrieval(_batch(ds), emb, DEV, k_retrieve=4, dense=True)
        out = dict(ev_idx1=b["rag_idx_h1"], ev_idx2=b["rag_idx_h2"], ev_mean=b["rag_mean"].clone(),
                   ev_dense=d["rag_emb_h1"].clone())
        m.train()
        for p in (0.0, 0.1):
            emb.dropout.p = p
            torch.manual_seed(123)
            t = ds.process_batch_retrieval(_batch(ds), emb, DEV, k_retrieve=4)
            out.update({f"tr{p}_idx1": t["rag_idx_h1"], f"tr{p}_idx2": t["rag_idx_h2"],
                        f"tr{p}_e1": t["rag_emb_h1"].detach().clone(), f"tr{p}_e2": t["rag_emb_h2"].detach().clone()})
            with K().option("deterministic", 1):      # fixed-order backward: the gradient is comparable
                g, = torch.autograd.grad(t["rag_emb_h1"].float().sum() + t["rag_emb_h2"].float().pow(2).sum(),
                                         emb.tokenizer.weight)
            out[f"tr{p}_gW"] = g.clone()
        got[pc] = out
    assert (got["u8"]["ev_idx1"] >= 0).all()
    for key, want in got["u8"].items():
        _same(got["bits"][key], want)


def _step_child(panel_codes: str) -> None:
    """One deterministic train_step on the tiny setup; prints the loss bits and a weights hash."""
    import faulthandler
    import hashlib
    faulthandler.dump_traceback_later(150, exit=True)
    from src.dataset.synthetic import make_rag_dataset
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized
    from src.model import build_model
    torch.manual_seed(0)
    np.random.seed(0)
    ds, vocab = make_rag_dataset(n_samples=8, n_sites=300, n_windows=2, n_ref_samples=40, seed=5, name="train",
                                 panel_codes=panel_codes)
    m = build_model(len(vocab), 64, 2, 2, dropout=0.1).to(DEV)
    tr = BERTTrainerWithValidationOptimized(m, None, None, vocab, lr=1e-3, warmup_steps=1, grad_accum_steps=1,
                                            log_freq=0, deterministic=True)
    tr.rag_train_dataset = ds
    tr.rag_k = 4
    loss = tr.train_step(_batch(ds, (0, 2, 4, 6, 1)))
    assert ds.panel_index(0, DEV).packed == (panel_codes == "bits")
    sha = hashlib.sha1(tr.flat.flat.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
    print(f"STEP loss {loss.float().view(torch.int32).item()} params {sha}")
    print("DONE", flush=True)


def test_deterministic_train_step_bits_equals_u8():
    outs = []
    for pc in ("u8", "bits"):     # fresh processes, one after the other, each under its own limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "step", pc], capture_output=True, text=True,
                           timeout=170)
        assert r.returncode == 0 and "DONE" in r.stdout, (pc, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("STEP")])
    assert len(outs[0]) == 1 and outs[0] == outs[1], outs


def test_infer_entry_bits_equals_u8(tmp_path):
    from src.infer_embedding_rag import infer
    res = {}
    for pc in ("u8", "bits"):
        res[pc] = infer(["--synthetic", "4", "--synthetic_sites", "1020", "--synthetic_ref", "24", "-d", "64", "-l", "1",
                         "-a", "2", "-b", "4", "--k_retrieve", "3", "--index_window_len", "510", "--panel_codes", pc,
                         "-o", str(tmp_path / pc)])
    for key in ("h1", "gt", "mask"):
        np.testing.assert_array_equal(res["bits"][key], res["u8"][key])
    assert (tmp_path / "bits" / "imputed.vcf").read_text() == (tmp_path / "u8" / "imputed.vcf").read_text()


# --------------------------------------------------------------- sharded, two gloo ranks --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_setup(panel_codes):
    from src.dataset.synthetic import make_rag_dataset
    from src.engine import engine_for
    from src.model import build_model
    torch.manual_seed(0)
    np.random.seed(0)
    ds, vocab = make_rag_dataset(n_samples=7, n_sites=300, n_windows=2, n_ref_samples=40, seed=3,
                                 panel_codes=panel_codes)
    m = build_model(len(vocab), 64, 1, 4).to(DEV).eval()
    engine_for(m).set_dtype(torch.float32)
    return ds, m


SHARD_ITEMS = ([0, 1, 2, 3, 5], [7, 9])          # ragged: both windows on rank 0, window 1 on rank 1
SHARD_TRAIN_ITEMS = ([0, 1, 2, 3, 5], [7, 9, 4])  # train mode: every rank has queries in both windows


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "rag-snvbert_amd")]
        from src.retrieval.shards import PanelShard
        ds, m = _shard_setup("bits")
        ds.set_panel_shard(PanelShard.current())
        b = ds.process_batch_retrieval(_batch(ds, SHARD_ITEMS[rank]), m.bert.embedding, DEV, k_retrieve=6)
        assert ds.panel_index(1, DEV).packed and ds.panel_index(1, DEV).n_ref < 80
        res = dict(idx1=b["rag_idx_h1"].cpu().numpy(), idx2=b["rag_idx_h2"].cpu().numpy(),
                   mean=b["rag_mean"].float().cpu().numpy())
        # train mode with dropout: the ranks exchange the unique neighbours' rows (unpack_rows)
        m.train()
        m.bert.embedding.dropout.p = 0.1
        t = ds.process_batch_retrieval(_batch(ds, SHARD_TRAIN_ITEMS[rank]), m.bert.embedding, DEV, k_retrieve=6)
        res["uniq"] = [(g.uniq.cpu().numpy(), g.uniq_codes.cpu().numpy()) for g in t["rag_groups"]]
        q.put((rank, res))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_bits_two_ranks_match_single_process_u8():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=280) for _ in ps)
    for p in ps:
        p.join(60)
    assert all(isinstance(got[r], dict) for r in range(2)), "\n".join(str(got[r]) for r in range(2))
    assert all(p.exitcode == 0 for p in ps)
    ds, m = _shard_setup("u8")
    for r in range(2):
        b = ds.process_batch_retrieval(_batch(ds, SHARD_ITEMS[r]), m.bert.embedding, DEV, k_retrieve=6)
        np.testing.assert_array_equal(got[r]["idx1"], b["rag_idx_h1"].cpu().numpy())
        np.testing.assert_array_equal(got[r]["idx2"], b["rag_idx_h2"].cpu().numpy())
        np.testing.assert_array_equal(got[r]["mean"], b["rag_mean"].float().cpu().numpy())
        # the exchanged rows are the whole panel's rows of the unique neighbours, one group per window
        assert len(got[r]["uniq"]) == 2
        hit = set()
        for uniq, codes in got[r]["uniq"]:
            assert len(uniq) > 0 and codes.dtype == np.uint8
            hit |= {w for w in range(2)
                    if np.array_equal(codes, _pad(np.asarray(ds.ref_alleles[w], np.uint8))[uniq])}
        assert hit == {0, 1}


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "step":
    _step_child(sys.argv[2])
