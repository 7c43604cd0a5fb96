"""Host side of the device-resident featurisation (src/dataset/device_features.py), no GPU: the
tables built on the host reproduce each dataset's own per-item arrays (gathered here in numpy the
way csrc/features.hip gathers them), the flags parse, the exports are declared, and ``nbytes``
follows the documented formula."""

import re

import numpy as np
import pytest
import torch

from conftest import REPO

L = 1030
FLOATS = ("pos", "af", "af_p", "ref", "het", "hom")


def _gather(ds, t, item):
    """One item from the host tables, as the kernel builds it (numpy restatement of the semantics in
    include/snvrag.h: snvrag_batch_features)."""
    from src.dataset.dataset import GLOBAL
    v = ds.vocab
    W = ds.window_count
    dup = item >= len(ds)
    s, w = (item - len(ds) if dup else item) // W, (item - len(ds) if dup else item) % W
    lo, hi = t["win_off"][w], t["win_off"][w + 1]
    n = hi - lo
    rows, cols = t["site_row"][lo:hi], t["freq_col"][lo:hi]
    out = {}
    alle = []
    for h in (0, 1):
        bits = np.unpackbits(t["gt_bits"][2 * s + h], bitorder="little")
        a = np.where(rows < 0, 0, bits[np.maximum(rows, 0)]).astype(np.int64)
        tok = np.full(L, v.pad_index, np.int64)
        tok[0] = v.sos_index
        tok[1:1 + n] = np.where(a == 1, v.stoi[1], v.stoi[0])
        if n + 1 < L:
            tok[n + 1] = v.eos_index
        tok[t["win_mask"][w] != 0] = v.mask_index
        out[f"hap_{h + 1}"] = tok
        lab = np.zeros(L, np.int64)
        lab[1:1 + n] = a
        out[f"hap_{h + 1}_label"] = lab
        alle.append(a)
    out["gt_label"] = np.zeros(L, np.int64)
    out["gt_label"][1:1 + n] = (alle[0] << 1) + alle[1]
    out["mask"] = np.zeros(L, np.int64) if dup else t["win_mask"][w].astype(np.int64)
    pop = t["pop_of_sample"][s]
    src = dict(pos=t["pos_norm"][lo:hi], af=t["freq"][3][GLOBAL][cols], af_p=t["freq"][3][pop][cols],
               ref=t["freq"][0][pop][cols], het=t["freq"][1][pop][cols], hom=t["freq"][2][pop][cols])
    for k in FLOATS:
        out[k] = np.zeros(L, np.float32)
        out[k][1:1 + n] = src[k]
    return out


def _check_items(ds, t, items):
    for item in items:
        want, got = ds[item], _gather(ds, t, item)
        for k, g in got.items():
            if k not in want:
                assert k.endswith("label")                  # the infer items carry no labels
                continue
            w = want[k].numpy()
            assert w.dtype == g.dtype and w.shape == g.shape, (k, w.dtype, g.dtype)
            assert np.array_equal(w.view(np.int32) if w.dtype == np.float32 else w,
                                  g.view(np.int32) if g.dtype == np.float32 else g), (item, k)


def _infer_ds(window_len, n_sites=1300, **kw):
    from src.dataset.embedding_rag_infer_dataset import EmbeddingRAGInferDataset
    from src.dataset.synthetic import POPS, make_infer_arrays
    from src.dataset.vocab import WordVocab
    a = make_infer_arrays(n_sites=n_sites, n_samples=5, missing_rate=0.3, **kw)
    return EmbeddingRAGInferDataset.from_arrays(WordVocab(POPS), a["vcf"], a["pos"], a["pops"], a["freq"],
                                                a["pop_to_idx"], a["pos_to_idx"], a["ref_gt"], a["ref_pos"],
                                                window_len=window_len)


@pytest.mark.parametrize("window_len,n_sites", [(1020, 1300), (510, 1300), (1028, 1028), (1029, 1029)])
def test_infer_tables_reproduce_items(window_len, n_sites):
    from src.dataset import device_features as DF
    ds = _infer_ds(window_len, n_sites)
    t = DF.host_tables(ds)
    counts = np.diff(t["win_off"])
    assert counts.tolist() == [ds.window_bounds(w)[1] - ds.window_bounds(w)[0] for w in range(ds.window_count)]
    assert (t["site_row"] < 0).any() and t["site_row"].dtype == np.int32 and t["pos_norm"].dtype == np.float32
    assert t["win_mask"].shape == (ds.window_count, L) and t["win_mask"].dtype == np.uint8
    _check_items(ds, t, range(len(ds)))


@pytest.mark.parametrize("name", ["train", "val"])
def test_train_tables_reproduce_items(name):
    from src.dataset import device_features as DF
    from src.dataset.embedding_rag_dataset import EmbeddingRAGDataset
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    ds0, vocab = make_rag_dataset(n_samples=6, n_sites=512, n_windows=2, n_ref_samples=16, name=name)
    _check_items(ds0, DF.host_tables(ds0), list(range(len(ds0))) + [len(ds0) + 3])
    # a panel lacking 37 sites of window 1: window_valid_indices filters the window's items
    ref_gt = np.concatenate([ra.T.reshape(ra.shape[1], -1, 2) for ra in ds0.ref_alleles])
    keep = np.ones(len(ds0.pos), bool)
    keep[np.random.default_rng(1).choice(np.arange(512, 1024), 37, replace=False)] = False
    ds = EmbeddingRAGDataset.from_arrays(vocab, ds0.vcf, ds0.pos, ds0.panel.pop_list, ds0.freq,
                                         ds0.window.window_info, ds0.pop_to_idx, ds0.pos_to_idx, ref_gt[keep],
                                         ds0.pos[keep], name=name)
    assert list(ds.window_valid_indices) == [1]
    t = DF.host_tables(ds)
    assert np.diff(t["win_off"]).tolist() == [512, 475]
    _check_items(ds, t, range(len(ds)))
    # the masks follow the epoch (train only), the level and the key that triggers a re-upload
    k0 = DF.mask_key(ds)
    ds.current_epoch += 1
    ds.add_level()
    assert DF.mask_key(ds) != k0
    t["win_mask"] = DF.window_masks(ds)
    _check_items(ds, t, [0, 1, len(ds) - 1])


def test_one_site_window_keeps_the_nan():
    """position_normalize of a one-site window is 0 / 0: the table holds the same NaN the item has."""
    from src.dataset import device_features as DF
    ds = _infer_ds(1020, 1021)
    assert ds.window_bounds(1) == (1020, 1021)
    with np.errstate(invalid="ignore"):
        t = DF.host_tables(ds)
        assert np.isnan(t["pos_norm"][-1]) and np.isnan(ds[1]["pos"][1].item())
        _check_items(ds, t, [0, 1])


def test_refuses_what_it_cannot_reproduce():
    from src.dataset import device_features as DF
    from src.dataset.dataset import TrainDataset
    ds = _infer_ds(1020)
    ds.vcf = ds.vcf.copy()
    ds.vcf[3, 2, 1] = -1
    with pytest.raises(ValueError, match="0/1 genotypes"):
        DF.host_tables(ds)
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    rag, vocab = make_rag_dataset(n_samples=2, n_sites=64, n_windows=1, n_ref_samples=8)
    plain = TrainDataset(vocab, rag.vcf, rag.pos, rag.panel, rag.freq, rag.window, {}, rag.pop_to_idx, rag.pos_to_idx)
    with pytest.raises(ValueError, match="EmbeddingRAGDataset"):
        DF.host_tables(plain)


def test_nbytes_formula():
    from src.dataset import device_features as DF
    ds = _infer_ds(510)
    t = DF.host_tables(ds)
    held = sum(v.nbytes for v in t.values())
    n_rows, S = ds.vcf.shape[0], ds.vcf.shape[1]
    assert held == DF.table_nbytes(n_rows, S, np.diff(t["win_off"]), ds.freq.shape[1], ds.freq.shape[2])
    assert held == 2 * S * ((n_rows + 7) // 8) + 12 * 1300 + 4 * 4 + 3 * 1030 + 16 * 6 * 1300 + 4 * S
    # DeviceFeatures.nbytes sums the same arrays after upload (same dtypes and shapes)
    assert {k: v.dtype for k, v in t.items()} == dict(
        gt_bits=np.uint8, win_off=np.int32, site_row=np.int32, freq_col=np.int32, pos_norm=np.float32,
        win_mask=np.uint8, freq=np.float32, pop_of_sample=np.int32)


def test_flags_parse_and_default_off():
    import inspect
    from src import infer_embedding_rag as I, train_embedding_rag as T
    assert I.parse_args([]).device_features is False and I.parse_args(["--device_features"]).device_features is True
    assert T.parse_args([]).device_features is False and T.parse_args(["--device_features"]).device_features is True
    sig = inspect.signature(I.run).parameters
    assert sig["device_features"].default is False and sig["output_budget_bytes"].default == I.OUTPUT_BUDGET_BYTES


def test_exports_declared_and_bound():
    from src import native
    header = (REPO / "include" / "snvrag.h").read_text()
    declared = set(re.findall(r"\b(snvrag_[a-z0-9_]+)\s*\(", header))
    new = {"snvrag_batch_features", "snvrag_infer_scatter"}
    assert new <= declared and new <= set(native.EXPORTED)
    assert native.ABI_VERSION == 31 and "#define SNVRAG_ABI_VERSION 31" in header
    # the ctypes struct mirrors the header's field order
    body = header[header.index("typedef struct {\n  const uint8_t* gt_bits;"):header.index("} snvrag_feature_tables_t;")]
    fields = re.findall(r"(\w+);", body)
    assert fields == [n for n, _ in native.FeatureTables._fields_]


def test_loader_chunks_and_length():
    """DeviceBatchLoader's chunking of the sampler stream (no device: a stub in place of the features)."""
    from src.dataset.device_features import DeviceBatchLoader

    class Stub:
        def batch(self, items):
            return list(items)

    ld = DeviceBatchLoader(object(), list(range(10)), 4, "cpu", features=Stub())
    assert len(ld) == 3 and list(ld) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert ld.batch_size == 4 and ld.sampler == list(range(10))
    assert list(DeviceBatchLoader(object(), [], 4, "cpu", features=Stub())) == []
