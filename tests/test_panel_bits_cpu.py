"""Bit-packed panel index, host side (src/retrieval/panel_index.py): the layout is
``np.packbits(bitorder="little")`` of the zero-padded rows, an eighth of the u8 index, and the
datasets validate their ``panel_codes`` switch.  No GPU: the tensors stay on the CPU."""

import numpy as np
import pytest
import torch


def _case():
    rng = np.random.default_rng(3)
    return (rng.random((37, 300)) < 0.3).astype(np.int64)


def test_layout_is_little_endian_packbits_with_zero_padding():
    from src.retrieval import PanelIndex, pad_sites
    a = _case()
    pk = PanelIndex.from_alleles(a, np.zeros(1030, np.float32), "cpu", packed=True)
    u8 = PanelIndex.from_alleles(a, np.zeros(1030, np.float32), "cpu")
    ld = pad_sites(300)
    assert ld == 512 and pk.packed and not u8.packed
    assert pk.bits.dtype == torch.uint8 and tuple(pk.bits.shape) == (37, ld // 8)
    padded = np.zeros((37, ld), np.uint8)
    padded[:, :300] = a
    bits = pk.bits.numpy()
    np.testing.assert_array_equal(bits, np.packbits(padded, axis=1, bitorder="little"))
    # site s of row r is bit s & 7 of byte s >> 3
    s = np.arange(ld)
    np.testing.assert_array_equal((bits[:, s >> 3] >> (s & 7)) & 1, padded)
    assert (np.unpackbits(bits, axis=1, bitorder="little")[:, 300:] == 0).all()
    assert (bits[:, (300 + 7) // 8:] == 0).all()
    # the same geometry as the u8 index, an eighth of its bytes
    assert (pk.n_ref, pk.ld, pk.n_sites, pk.n_sites_pad) == (u8.n_ref, u8.ld, u8.n_sites, u8.n_sites_pad)
    assert u8.nbytes == 37 * ld and pk.nbytes * 8 == u8.nbytes
    assert pk.device == u8.device == torch.device("cpu")
    torch.testing.assert_close(u8.rows(torch.tensor([5, 0, 36])), u8.codes[[5, 0, 36]], rtol=0, atol=0)


def test_shard_arguments_carry_over():
    from src.retrieval import PanelIndex
    pk = PanelIndex.from_alleles(_case()[10:20], np.zeros(1030, np.float32), "cpu", ref_offset=10, n_total=37,
                                 packed=True)
    assert (pk.n_ref, pk.ref_offset, pk.n_total) == (10, 10, 37)


def test_codes_of_a_packed_index_raises_naming_unpack_rows():
    from src.retrieval import PanelIndex
    pk = PanelIndex.from_alleles(_case(), np.zeros(1030, np.float32), "cpu", packed=True)
    with pytest.raises(AttributeError, match="unpack_rows"):
        pk.codes
    assert PanelIndex.from_alleles(_case(), np.zeros(1030, np.float32), "cpu").bits is None


@pytest.mark.parametrize("packed", [False, True])
def test_non_binary_alleles_are_refused(packed):
    from src.retrieval import PanelIndex
    a = _case()
    a[3, 7] = 2
    with pytest.raises(ValueError, match="biallelic"):
        PanelIndex.from_alleles(a, np.zeros(1030, np.float32), "cpu", packed=packed)
    a[3, 7] = -1
    with pytest.raises(ValueError, match="biallelic"):
        PanelIndex.from_alleles(a, np.zeros(1030, np.float32), "cpu", packed=packed)


def test_panel_codes_validation_in_both_datasets():
    from src.dataset.embedding_rag_dataset import panel_index_of
    from src.dataset.synthetic import make_infer_dataset, make_rag_dataset
    ds, _ = make_rag_dataset(n_samples=2, n_sites=40, n_windows=1, n_ref_samples=4)
    assert ds.panel_codes == "u8"
    with pytest.raises(ValueError, match="panel_codes"):
        make_rag_dataset(n_samples=2, n_sites=40, n_windows=1, n_ref_samples=4, panel_codes="u4")
    assert make_rag_dataset(n_samples=2, n_sites=40, n_windows=1, n_ref_samples=4,
                            panel_codes="bits")[0].panel_codes == "bits"
    with pytest.raises(ValueError, match="panel_codes"):
        ds.set_panel_codes("packed")
    ds.set_panel_codes("bits")
    idx = ds.panel_index(0, "cpu")
    assert idx.packed and idx.nbytes == idx.n_ref * idx.n_sites_pad // 8
    ds.set_panel_codes("u8")                                   # the setter drops the cached indexes
    assert not ds.panel_index(0, "cpu").packed
    inf, _ = make_infer_dataset(n_sites=600, n_samples=2, n_ref_samples=4, index_window_len=510)
    assert inf.panel_codes == "u8"
    with pytest.raises(ValueError, match="panel_codes"):
        make_infer_dataset(n_sites=600, n_samples=2, n_ref_samples=4, index_window_len=510, panel_codes="bit")
    inf.set_panel_codes("bits")
    assert inf.panel_index(0, "cpu").packed
    with pytest.raises(ValueError, match="panel_codes"):
        panel_index_of(_case(), np.zeros(1030, np.float32), "cpu", panel_codes="nibbles")
