"""Device-resident featurisation (src/dataset/device_features.py, csrc/features.hip
``snvrag_batch_features``, csrc/embed.hip ``snvrag_infer_scatter``): every tensor of a device-built
batch equals the collated host items bit for bit (floats compared as their 32-bit patterns), the
scattered inference outputs equal ``infer_post`` + the host ``geometry``, and the two entry points
give identical results with the option on and off."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOMASK = ("hap1_nomask", "hap2_nomask")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _host_batch(ds, items):
    from src.dataset.embedding_rag_dataset import embedding_rag_collate_fn
    return embedding_rag_collate_fn([ds[i] for i in items])


def _assert_batch_equal(got, want, L=None):
    assert set(got) == set(want) - set(NOMASK), set(got) ^ set(want)
    for k, v in want.items():
        if k in NOMASK:
            continue
        if k == "window_idx":
            assert type(got[k]) is type(v) and len(got[k]) == len(v)
            assert all(type(a) is type(b) and int(a) == int(b) for a, b in zip(got[k], v))
            assert not any(torch.is_tensor(a) and a.is_cuda for a in got[k])
            continue
        g = got[k]
        if L is not None and v.dim() == 2 and v.shape[1] > 1:
            v = v[:, :L]
        assert g.is_cuda and g.dtype == v.dtype and g.shape == v.shape, (k, g.dtype, g.shape, v.shape)
        assert torch.equal(_bits(g), _bits(v)), k


def _infer_ds(a, panel_codes="u8", **kw):
    from src.dataset.embedding_rag_infer_dataset import EmbeddingRAGInferDataset
    from src.dataset.synthetic import POPS
    from src.dataset.vocab import WordVocab
    vocab = WordVocab(POPS)
    ds = EmbeddingRAGInferDataset.from_arrays(vocab, a["vcf"], a["pos"], a["pops"], a["freq"], a["pop_to_idx"],
                                              a["pos_to_idx"], a["ref_gt"], a["ref_pos"], panel_codes=panel_codes,
                                              **kw)
    return ds, vocab


@pytest.fixture(scope="module")
def infer_arrays():
    from src.dataset.synthetic import make_infer_arrays
    return make_infer_arrays(n_sites=1300, n_samples=5, missing_rate=0.3)


# --------------------------------------------------------------------- kernel vs host, infer --
@pytest.mark.parametrize("window_len", [1020, 510])
def test_infer_batches_equal_host_items(infer_arrays, window_len):
    """1300 sites: a full 1020-site window plus a ragged 280-site one (eos and pads inside the
    row; the 510-site index windows put mask bits past the 280 sites), and the same data in 510-site
    windows (510, 510, 280).  All items in sampler-sized chunks, then a batch that mixes windows and
    repeats a sample."""
    from src.dataset.device_features import DeviceFeatures
    ds, _ = _infer_ds(infer_arrays, window_len=window_len)
    assert ds.window_count == (2 if window_len == 1020 else 3)
    if window_len == 1020:
        assert np.asarray(ds.infer_masks[1])[282:].any()            # bits set past n = 280
    df = DeviceFeatures(ds, DEV)
    n = len(ds)
    chunks = [list(range(i, min(i + 4, n))) for i in range(0, n, 4)] + [[0, 1, 0, n - 1, 3, 2, 1]]
    for items in chunks:
        _assert_batch_equal(df.batch(items), _host_batch(ds, items))
    b = df.batch([0, 1, 2])
    assert b["hap_1"]._base is b["hap_2"]._base                      # one [2B, L] buffer: retrieval's cat([h1, h2])
    with pytest.raises(IndexError):
        df.batch([n])


@pytest.mark.parametrize("n_sites", [1028, 1029])
def test_infer_eos_edge(n_sites):
    """One window of 1028 sites: eos lands in the last slot; 1029 sites: no eos.  The window's mask
    gets a bit on that last slot (past n for 1028), which must turn it into the mask token."""
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_infer_arrays
    a = make_infer_arrays(n_sites=n_sites, n_samples=3, missing_rate=0.3, seed=2)
    ds, vocab = _infer_ds(a, window_len=n_sites)
    assert ds.window_count == 1
    want = _host_batch(ds, [0, 1, 2])
    last = want["hap_1"][:, -1]
    assert (last == vocab.eos_index).all() if n_sites == 1028 else (last >= vocab.stoi[0]).all() or \
        (last == vocab.mask_index).any()
    _assert_batch_equal(DeviceFeatures(ds, DEV).batch([0, 1, 2]), want)
    m = np.asarray(ds.infer_masks[0]).copy()
    m[1029] = 1
    ds.infer_masks[0] = m
    want = _host_batch(ds, [2, 0])
    assert (want["hap_1"][:, -1] == vocab.mask_index).all()
    _assert_batch_equal(DeviceFeatures(ds, DEV).batch([2, 0]), want)


# --------------------------------------------------------------------- kernel vs host, train --
def _unmatched_dataset(name):
    """make_rag_dataset's data with 37 sites of window 1 dropped from the panel: window_valid_indices
    is non-empty and the window's items hold the matched sites only."""
    from src.dataset.embedding_rag_dataset import EmbeddingRAGDataset
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    ds0, vocab = make_rag_dataset(n_samples=6, n_sites=512, n_windows=2, n_ref_samples=16, name=name)
    ref_gt = np.concatenate([ra.T.reshape(ra.shape[1], -1, 2) for ra in ds0.ref_alleles])
    keep = np.ones(len(ds0.pos), bool)
    keep[np.random.default_rng(1).choice(np.arange(512, 1024), 37, replace=False)] = False
    ds = EmbeddingRAGDataset.from_arrays(vocab, ds0.vcf, ds0.pos, ds0.panel.pop_list, ds0.freq,
                                         ds0.window.window_info, ds0.pop_to_idx, ds0.pos_to_idx, ref_gt[keep],
                                         ds0.pos[keep], name=name)
    assert list(ds.window_valid_indices) == [1] and ds.window_actual_lens == [512, 475]
    return ds


@pytest.mark.parametrize("name", ["train", "val"])
@pytest.mark.parametrize("unmatched", [False, True])
def test_train_batches_equal_host_items(name, unmatched):
    """All keys (the three labels included) for every item, the DistributedWindowSampler padding
    duplicates (item >= len(ds): same tokens, zero mask), and the mask following the dataset after
    current_epoch += 1, add_level() and regenerate_masks()."""
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_rag_dataset
    if unmatched:
        ds = _unmatched_dataset(name)
    else:
        np.random.seed(0)
        ds, _ = make_rag_dataset(n_samples=6, n_sites=512, n_windows=2, n_ref_samples=16, name=name)
    df = DeviceFeatures(ds, DEV)
    n = len(ds)
    for items in (list(range(0, 7)), list(range(7, n)), [1, n + 1, 0, n + 4, 1]):
        got, want = df.batch(items), _host_batch(ds, items)
        _assert_batch_equal(got, want)
    assert not got["mask"][1].any() and got["mask"][0].any()
    assert torch.equal(got["hap_1"][0], got["hap_1"][1])            # the duplicate keeps its masked tokens
    before = df.batch([0, 1])["mask"].clone()
    ds.current_epoch += 1
    _assert_batch_equal(df.batch([0, 1, 5]), _host_batch(ds, [0, 1, 5]))
    assert torch.equal(df.batch([0, 1])["mask"], before) == (name == "val")   # val masks: seed 2024 always
    ds.add_level()
    _assert_batch_equal(df.batch([3, 2]), _host_batch(ds, [3, 2]))
    ds.regenerate_masks(seed=3)
    _assert_batch_equal(df.batch([4, 3]), _host_batch(ds, [4, 3]))
    ds.current_epoch -= 1                                            # back to a cached (seed, level)
    _assert_batch_equal(df.batch([4, 3]), _host_batch(ds, [4, 3]))


def test_odd_row_length_scalar_stores():
    """L = 515 (odd: rows are not 16-byte aligned, the kernel stores element by element) against
    the host items cut to 515 columns — 512 sites, so sos, eos and pads all fall inside."""
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    ds, _ = make_rag_dataset(n_samples=3, n_sites=512, n_windows=2, n_ref_samples=16, name="val")
    df = DeviceFeatures(ds, DEV, L=515)
    items = [5, 0, 3, 9]
    _assert_batch_equal(df.batch(items), _host_batch(ds, items), L=515)


# -------------------------------------------------------------------------------- refusals --
def test_refusals():
    from src import kernels as K
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    ds, _ = make_rag_dataset(n_samples=3, n_sites=512, n_windows=2, n_ref_samples=16, name="val")
    df = DeviceFeatures(ds, DEV)
    rows = torch.tensor([[0, 1], [0, 1], [0, 0]], dtype=torch.int32)
    call = lambda r, L: K.batch_features(df.tables, r.to(DEV), r, 2, L, df.token_ids, labels=True)
    call(rows, 1030)
    with pytest.raises(RuntimeError, match=r"L must be in \[2, 1030\]"):
        call(rows, 1031)
    with pytest.raises(RuntimeError, match="n \\+ 1 > L"):
        call(rows, 512)
    bad = rows.clone()
    bad[1, 1] = 2
    with pytest.raises(RuntimeError, match="window index out of range"):
        call(bad, 1030)
    bad = rows.clone()
    bad[0, 0] = 3
    with pytest.raises(RuntimeError, match="sample index out of range"):
        call(bad, 1030)
    ds.vcf = ds.vcf.copy()
    ds.vcf[5, 1, 0] = -1
    with pytest.raises(ValueError, match="0/1 genotypes"):
        DeviceFeatures(ds, DEV)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- infer_scatter --
@pytest.mark.parametrize("L,window_len,n_variants", [(130, 100, 250), (130, 100, 300), (130, 100, 317),
                                                     (1030, 1020, 3060)])
def test_infer_scatter_equals_post_plus_geometry(L, window_len, n_variants):
    """W = 3, S = 4: the 12 sample-windows in a shuffled order, in batches of 7 and 5 (ragged
    row tiles), n_variants below, equal to and above W * window_len."""
    from src import kernels as K
    from src.infer_embedding_rag import geometry
    W, S = 3, 4
    g = torch.Generator().manual_seed(L + n_variants)
    pr = torch.rand(2, W * S, L, 2, generator=g)
    pr = (pr / pr.sum(-1, keepdim=True)).to(DEV)
    mask = torch.randint(0, 2, (W * S, L), generator=g).to(DEV)
    p1, p2, gt = K.infer_post(pr[0], pr[1])                          # rows in window-major order: r = w S + s
    want = geometry(p1.cpu().numpy(), p2.cpu().numpy(), gt.cpu().numpy(), mask.cpu().numpy(), W, n_variants,
                    window_len)
    out = [torch.zeros(n_variants, S, device=DEV), torch.zeros(n_variants, S, device=DEV),
           torch.zeros(n_variants, S, 4, device=DEV), torch.zeros(n_variants, S, device=DEV, dtype=torch.long)]
    order = torch.randperm(W * S, generator=g)
    for rows in (order[:7], order[7:]):
        B = len(rows)
        table = torch.stack([rows % S, rows // S, torch.zeros_like(rows)]).to(torch.int32).contiguous()
        r = rows.to(DEV)
        K.infer_scatter(pr[0][r].contiguous(), pr[1][r].contiguous(), mask[r].contiguous(), table.to(DEV), table,
                        window_len, *out)
    for got, ref in zip(out, want):
        assert got.shape == ref.shape
        assert torch.equal(_bits(got), _bits(torch.from_numpy(np.ascontiguousarray(ref))))
    bad = table.clone()
    bad[0, 0] = S
    with pytest.raises(RuntimeError, match="sample index out of range"):
        K.infer_scatter(pr[0][r].contiguous(), pr[1][r].contiguous(), mask[r].contiguous(), bad.to(DEV), bad,
                        window_len, *out)


# ------------------------------------------------------------------------------ end to end --
def _model(vocab, dropout=0.1):
    from src.model import build_model
    torch.manual_seed(0)
    return build_model(len(vocab), 64, 2, 2, dropout=dropout).to(DEV)


@pytest.mark.parametrize("panel_codes,budget", [("u8", None), ("bits", None), ("u8", 0)])
def test_infer_run_identical_with_device_features(infer_arrays, panel_codes, budget, capsys):
    from src.infer_embedding_rag import OUTPUT_BUDGET_BYTES, run
    ds, vocab = _infer_ds(infer_arrays, panel_codes=panel_codes)
    m = _model(vocab).eval()
    off = run(ds, m, torch.device(DEV), 4, 3)
    on = run(ds, m, torch.device(DEV), 4, 3, device_features=True,
             output_budget_bytes=OUTPUT_BUDGET_BYTES if budget is None else budget)
    assert ("output_budget_bytes" in capsys.readouterr().out) == (budget is not None)
    assert (on["batch_h1"] is None) == (budget is None)            # the scatter path keeps no per-row outputs
    for k in ("h1", "h2", "gt", "mask", "idx1", "idx2"):
        assert on[k].dtype == off[k].dtype and on[k].shape == off[k].shape, k
        assert np.array_equal(on[k].view(np.int32) if on[k].dtype == np.float32 else on[k],
                              off[k].view(np.int32) if off[k].dtype == np.float32 else off[k]), k
    assert on["masked_snvs"] == off["masked_snvs"] > 0


def test_train_steps_identical_from_device_loader():
    """Two deterministic training steps fed by DeviceBatchLoader and by the DataLoader over the same
    sampler: bitwise-equal losses and weights."""
    from src.dataset.device_features import DeviceBatchLoader
    from src.dataset.embedding_rag_dataset import embedding_rag_collate_fn
    from src.dataset.sampler import WindowGroupedSampler
    from src.dataset.synthetic import make_rag_dataset
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized

    def steps(device_loader):
        np.random.seed(0)
        ds, vocab = make_rag_dataset(n_samples=6, n_sites=512, n_windows=2, n_ref_samples=16, seed=5, name="train")
        sampler = WindowGroupedSampler(ds, shuffle=True, seed=42)
        if device_loader:
            loader = DeviceBatchLoader(ds, sampler, 4, DEV)
        else:
            loader = torch.utils.data.DataLoader(ds, batch_size=4, sampler=sampler,
                                                 collate_fn=embedding_rag_collate_fn)
        assert len(loader) == 3 and loader.dataset is ds and loader.sampler is sampler and loader.batch_size == 4
        tr = BERTTrainerWithValidationOptimized(_model(vocab), loader, None, vocab, lr=1e-3, warmup_steps=1,
                                                grad_accum_steps=1, log_freq=0, deterministic=True)
        tr.rag_k = 4
        losses = []
        for i, batch in enumerate(loader):
            if i == 2:
                break
            torch.manual_seed(100 + i)
            losses.append(tr.train_step(batch).float())
        return torch.stack(losses), tr.flat.flat.detach().clone()

    la, wa = steps(False)
    lb, wb = steps(True)
    assert torch.isfinite(la).all()
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(wa), _bits(wb))
