"""GPU tests of the device VCF reader (src/dataset/vcf_reader.py read_vcf, csrc/vcfread.hip) against its
specification parse_vcf_host: exact equality of samples, pos and gt() over the shapes at which the
kernels change path (one lane group, one tile, a partial tile, a partial 64-record group, chunk and
record carries), the fixed-width and the general parse path, and the wiring behind it (PanelIndex
from bit rows, device features from the file's bit rows, the file path of the entry points)."""

import gzip
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from knn_helpers import rand_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 1 << 20
COUNTS = (1, 7, 8, 9, 63, 64, 65, 130)


def V():
    from src.dataset import vcf_reader
    return vcf_reader


def same_as_host(path, **kw):
    """read_vcf(path) == parse_vcf_host(path); returns (VcfGenotypes, host gt)."""
    samples, pos, gt = V().parse_vcf_host(path)
    vg = V().read_vcf(path, DEV, **{"chunk_bytes": CHUNK, **kw})
    assert vg.samples == samples and vg.n_sites == len(pos)
    assert vg.pos.dtype == np.int32
    np.testing.assert_array_equal(vg.pos, pos)
    want = gt.copy()
    want[want > 0] = 1
    got = vg.gt()
    assert got.dtype == np.int8 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert vg.any_missing == bool((gt < 0).any())
    with V()._open(path) as fh:
        body = fh.read().split(b"#CHROM", 1)[1].split(b"\n")[1:]
    slash = any(b"/" in cell.split(b":")[0] for line in body for cell in line.split(b"\t")[9:])
    assert vg.phased == (not slash)
    assert vg.alt_bits.shape == vg.miss_bits.shape == (2 * len(samples), (len(pos) + 7) // 8)
    return vg, want


def same_bits(a, b):
    assert torch.equal(a.alt_bits, b.alt_bits) and torch.equal(a.miss_bits, b.miss_bits)
    np.testing.assert_array_equal(a.pos, b.pos)
    assert (a.any_missing, a.phased) == (b.any_missing, b.phased)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_fixed_width_files_both_paths(tmp_path, S):
    from src.dataset.device_features import pack_genotypes
    rng = np.random.default_rng(S)
    names = [f"S{i}" for i in range(S)]
    for n in COUNTS:
        gt = (rng.random((n, S, 2)) < 0.3).astype(np.int8)
        pos = np.cumsum(rng.integers(1, 10 ** 6, n)).astype(np.int32)
        pos[-1] = 2 ** 31 - 1                                 # ten digits, the largest POS
        path = tmp_path / f"f{n}.vcf"
        V().write_gt_vcf(path, names, pos, gt)
        fixed, want = same_as_host(path)
        general, _ = same_as_host(path, force_general=True)
        same_bits(fixed, general)
        assert fixed.phased and not fixed.any_missing
        np.testing.assert_array_equal(fixed.alt_bits.cpu().numpy(), pack_genotypes(want))
        assert not fixed.miss_bits.any()


CELLS = ["0|1", "1/0", ".|.", "./.", ".", "1", "10|2", "0|1:35:0.1,0.2,0.7", "0|0", "1|1", "0/00", "2|.", ".|3"]


def mixed_text(n, S, seed, crlf=False, final_newline=True):
    """Lines of three kinds: fixed-width GT-only, GT-only with odd cells, and GT:DS:GP."""
    rng = np.random.default_rng(seed)
    out = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
           "\t".join(f"N{i}" for i in range(S))]
    for i in range(n):
        kind = rng.integers(0, 3)
        if kind == 0:
            cells = [f"{a}|{b}" for a, b in rng.integers(0, 2, (S, 2))]
            fmt = "GT"
        elif kind == 1:
            cells = [CELLS[j] if ":" not in CELLS[j] else "1|0" for j in rng.integers(0, len(CELLS), S)]
            fmt = "GT"
        else:
            cells = [CELLS[j].split(":")[0] + f":{rng.integers(0, 99)}:0.1,0.2,0.7" for j in rng.integers(0, len(CELLS), S)]
            fmt = "GT:DS:GP"
        out.append(f"1\t{100 + 3 * i}\t.\tA\tC\t.\tPASS\t.\t{fmt}\t" + "\t".join(cells))
        if i % 11 == 5:
            out.append("")                                   # an empty line inside the body
    nl = "\r\n" if crlf else "\n"
    text = nl.join(out) + (nl if final_newline else "")
    return text.encode()


@pytest.mark.parametrize("S,n", [(1, 9), (63, 65), (64, 64), (65, 130), (257, 63)])
def test_mixed_files_fall_back_per_line(tmp_path, S, n):
    path = tmp_path / "m.vcf"
    path.write_bytes(mixed_text(n, S, seed=S + n))
    a, _ = same_as_host(path)
    b, _ = same_as_host(path, force_general=True)
    same_bits(a, b)


@pytest.mark.parametrize("crlf,final_newline", [(True, True), (True, False), (False, False)])
def test_line_endings(tmp_path, crlf, final_newline):
    path = tmp_path / "e.vcf"
    path.write_bytes(mixed_text(70, 5, seed=3, crlf=crlf, final_newline=final_newline))
    same_bits(same_as_host(path)[0], same_as_host(path, force_general=True)[0])


def test_long_info_and_every_prefix_alignment(tmp_path):
    """INFO of about 5 000 bytes, and 16 consecutive prefix lengths: the ninth tab and the line starts
    fall on every offset modulo 16, and across the 64-byte step edge."""
    S, rng = 65, np.random.default_rng(8)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + \
        "\t".join(f"N{i}" for i in range(S)) + "\n"
    lines = []
    for i in range(48):
        info = "." if i % 3 else "AC=" + "7" * (4990 + i)
        ident = "r" * (1 + i % 16)
        fixed = i % 2 == 0
        cells = [f"{a}|{b}" for a, b in rng.integers(0, 2, (S, 2))]
        if not fixed:
            cells[i % S] = "1|0:9"
        lines.append(f"1\t{10 + i}\t{ident}\tA\tC\t.\tPASS\t{info}\t{'GT' if fixed else 'GT:DS'}\t" + "\t".join(cells) + "\n")
    path = tmp_path / "long.vcf"
    path.write_text(head + "".join(lines))
    a, _ = same_as_host(path)
    same_bits(a, same_as_host(path, force_general=True)[0])
    longest = max(len(l) for l in lines)
    same_bits(a, same_as_host(path, chunk_bytes=longest + 1)[0])


def test_chunk_boundaries_tail_and_record_carry(tmp_path):
    """chunk_bytes just above the longest line: one or two records per chunk, so every chunk cuts a tail
    and the 64-record carry runs across many chunks; the .gz twin reads the same."""
    S, n = 65, 130
    rng = np.random.default_rng(4)
    gt = (rng.random((n, S, 2)) < 0.4).astype(np.int8)
    pos = np.arange(1000, 1000 + 7 * n, 7, dtype=np.int32)
    names = [f"S{i}" for i in range(S)]
    V().write_gt_vcf(tmp_path / "c.vcf", names, pos, gt)
    V().write_gt_vcf(tmp_path / "c.vcf.gz", names, pos, gt)
    body = (tmp_path / "c.vcf").read_bytes().split(b"#CHROM", 1)[1].split(b"\n")[1:]
    longest = max(len(l) for l in body) + 1                   # with its newline
    whole, _ = same_as_host(tmp_path / "c.vcf")
    for chunk in (longest + 1, 2 * longest + 3, 64 * longest + 5):
        same_bits(whole, same_as_host(tmp_path / "c.vcf", chunk_bytes=chunk)[0])
        same_bits(whole, same_as_host(tmp_path / "c.vcf", chunk_bytes=chunk, force_general=True)[0])
    same_bits(whole, same_as_host(tmp_path / "c.vcf.gz")[0])
    same_bits(whole, same_as_host(tmp_path / "c.vcf.gz", chunk_bytes=longest + 1)[0])
    with pytest.raises(ValueError, match="longer than chunk_bytes"):
        V().read_vcf(tmp_path / "c.vcf", DEV, chunk_bytes=longest - 1)


GOOD = "1\t{pos}\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|0\t0|0\t1|1\n"
BAD = {1: "1\t200\t.\tA\tC\t.\tPASS\t.\tDS:GT\t0|1\t1|0\t0|0\t1|1\n",
       2: "1\t200\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|0\t0|0\n",
       4: "1\t200\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|0|1\t0|0\t1|1\n",
       8: "1\t2147483648\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|0\t0|0\t1|1\n",
       16: "1\t200\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|x\t0|0\t1|1\n",
       3: "1\t200\t.\tA\tC\t.\tPASS\t.\n",
       18: "1\t200\t.\tA\tC\t.\tPASS\t.\tGT\t0|1\t1|0\t0|0\t1|1\t\n"}


@pytest.mark.parametrize("flag", sorted(BAD))
@pytest.mark.parametrize("force_general", [False, True])
def test_each_flag_raises_the_host_error(tmp_path, flag, force_general):
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC\tD\n"
    body = "".join(GOOD.format(pos=10 + i) for i in range(70)) + "\n" + BAD[flag] + GOOD.format(pos=999)
    path = tmp_path / "bad.vcf"
    path.write_text(head + body)
    with pytest.raises(ValueError) as host:
        V().parse_vcf_host(path)
    assert f"line 74: " in str(host.value)
    with pytest.raises(ValueError) as dev:
        V().read_vcf(path, DEV, chunk_bytes=CHUNK, force_general=force_general)
    assert str(dev.value) == str(host.value)


def test_kernel_outputs_fixed_equals_general():
    """The raw kernels on one chunk: line offsets against numpy, and codes / pos / flags of the two parse
    paths byte for byte (flags bits 8-12 included)."""
    from src import kernels as K
    S = 1030                                                  # two fixed-path tiles, the second partial
    text = mixed_text(40, S, seed=1).split(b"\n", 2)[2]
    nbytes = len(text)
    buf = np.full((nbytes + 15) // 16 * 16, 10, np.uint8)
    buf[:nbytes] = np.frombuffer(text, np.uint8)
    t = torch.from_numpy(buf).to(DEV)
    line_off, n_lines = K.vcf_line_index(t, nbytes, 64)
    starts = [i for i in range(nbytes) if text[i] != 10 and (i == 0 or text[i - 1] == 10)]
    assert int(n_lines) == len(starts)
    np.testing.assert_array_equal(line_off[:len(starts) + 1].cpu().numpy(), starts + [nbytes])
    out = []
    for force in (False, True):
        codes = torch.zeros(len(starts), 1032, device=DEV, dtype=torch.uint8)
        pos, flags = K.vcf_parse_gt(t, nbytes, line_off, len(starts), S, codes, force)
        out.append((codes[:, :S].cpu().numpy(), pos.cpu().numpy(), flags.cpu().numpy()))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    assert not (out[0][2] & 0x1f).any()


def test_panel_index_from_bit_rows():
    """A non-contiguous site list: the gathered index equals from_alleles of the same columns in both
    layouts, and searches to the same neighbours."""
    from src import kernels as K
    from src.retrieval import PanelIndex
    n_sites, n_src = 500, 1500
    W, panel, site_mask, tok = rand_case(300, n_sites, 12, 7)
    rng = np.random.default_rng(2)
    site_idx = np.sort(rng.choice(n_src, n_sites, replace=False)).astype(np.int32)
    full = (rng.random((300, n_src)) < 0.5).astype(np.uint8)
    full[:, site_idx] = panel
    bits = torch.from_numpy(np.packbits(full, axis=1, bitorder="little")).to(DEV)       # [n_haps, ceil(n_src / 8)]
    af = np.zeros(1030, np.float32)
    args = (torch.from_numpy(tok).to(DEV), torch.from_numpy(W).to(DEV), torch.from_numpy(site_mask).to(DEV), 8)
    for packed in (False, True):
        want = PanelIndex.from_alleles(panel, af, DEV, packed=packed)
        got = PanelIndex.from_bit_rows(bits, site_idx, af, packed=packed, n_src_sites=n_src)
        assert got.packed == packed and got.n_sites == n_sites and got.n_ref == 300
        assert torch.equal(got.data, want.data)
        (gi, gd), (wi, wd) = got.search(*args), want.search(*args)
        assert torch.equal(gi, wi) and torch.equal(gd, wd)
    # a shard's row range, and -1 / out-of-range sites give 0
    part = PanelIndex.from_bit_rows(bits[100:200], site_idx, af, packed=True, ref_offset=100, n_total=300,
                                    n_src_sites=n_src)
    assert torch.equal(part.data, PanelIndex.from_alleles(panel[100:200], af, DEV, packed=True).data)
    holes = site_idx.copy()
    holes[::7] = -1
    holes[3] = n_src
    got = K.panel_gather_bits(bits, n_src, torch.from_numpy(holes).to(DEV), 512, False).cpu().numpy()
    want = np.zeros((300, 512), np.uint8)
    ok = (holes >= 0) & (holes < n_src)
    want[:, :n_sites][:, ok] = full[:, holes[ok]]
    np.testing.assert_array_equal(got, want)


def write_common_files(d, a, samples):
    with open(d / "panel.txt", "w") as f:
        f.write("sample\tpop\tsuper_pop\n")
        for s, p in zip(samples, a["pops"]):
            f.write(f"{s}\tX\t{p}\n")
    np.save(d / "freq.npy", a["freq"])
    for name, obj in (("type.pkl", {}), ("pop.pkl", a["pop_to_idx"]), ("pos.pkl", a["pos_to_idx"])):
        with open(d / name, "wb") as f:
            pickle.dump(obj, f)


def test_infer_entry_through_files_equals_arrays(tmp_path):
    """target.vcf + panel.vcf.gz through build_dataset's file path against make_infer_dataset on the same
    arrays: bitwise equal run() outputs, with and without device features, for both panel layouts."""
    from src.dataset.synthetic import make_infer_arrays, make_infer_dataset
    from src.engine import engine_for
    from src.infer_embedding_rag import build_dataset, parse_args, run
    from src.model import build_model
    a = make_infer_arrays(1300, 6, 24, missing_rate=0.3, ref_missing=5, seed=11)
    samples = [f"S{i}" for i in range(6)]
    V().write_gt_vcf(tmp_path / "target.vcf", samples, a["pos"], a["vcf"])
    V().write_gt_vcf(tmp_path / "panel.vcf.gz", [f"R{i}" for i in range(24)], a["ref_pos"], a["ref_gt"])
    write_common_files(tmp_path, a, samples)
    dev = torch.device("cuda", torch.cuda.current_device())
    for codes in ("u8", "bits"):
        args = parse_args(["--infer_dataset", str(tmp_path / "target.vcf"), "--infer_panel", str(tmp_path / "panel.txt"),
                           "--freq_path", str(tmp_path / "freq.npy"), "--type_path", str(tmp_path / "type.pkl"),
                           "--pop_path", str(tmp_path / "pop.pkl"), "--pos_path", str(tmp_path / "pos.pkl"),
                           "--ref_panel", str(tmp_path / "panel.vcf.gz"), "--panel_codes", codes,
                           "-d", "64", "-l", "2", "-a", "2", "-b", "4", "--k_retrieve", "3"])
        ds_file, vocab = build_dataset(args)
        ds_mem, _ = make_infer_dataset(a, panel_codes=codes)
        assert ds_file.vcf_genotypes is not None and ds_file.ref_panel_vcf is not None
        np.testing.assert_array_equal(ds_file.vcf, a["vcf"])
        assert ds_file.panel_index(0, dev).packed == (codes == "bits")
        assert torch.equal(ds_file.panel_index(1, dev).data, ds_mem.panel_index(1, dev).data)
        torch.manual_seed(0)
        model = build_model(len(vocab), 64, 2, 2).to(dev).eval()
        engine_for(model).set_dtype(torch.float32)
        for feats in (False, True):
            want = run(ds_mem, model, dev, 4, 3, device_features=feats)
            got = run(ds_file, model, dev, 4, 3, device_features=feats)
            for k in ("h1", "h2", "gt", "mask"):
                np.testing.assert_array_equal(got[k], want[k])


def test_device_features_take_the_files_bit_rows(tmp_path):
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_infer_arrays, make_infer_dataset
    a = make_infer_arrays(300, 5, 8, seed=2)
    ds, _ = make_infer_dataset(a)
    V().write_gt_vcf(tmp_path / "t.vcf", [f"S{i}" for i in range(5)], a["pos"], a["vcf"])
    ds.vcf_genotypes = V().read_vcf(tmp_path / "t.vcf", DEV, chunk_bytes=CHUNK)
    f = DeviceFeatures(ds, DEV)
    assert f.dev["gt_bits"].data_ptr() == ds.vcf_genotypes.alt_bits.data_ptr()
    miss = a["vcf"].copy()
    miss[3, 2, 1] = -1
    V().write_gt_vcf(tmp_path / "m.vcf", [f"S{i}" for i in range(5)], a["pos"], miss)
    ds.vcf_genotypes = V().read_vcf(tmp_path / "m.vcf", DEV, chunk_bytes=CHUNK)
    with pytest.raises(ValueError, match="device features need 0/1 genotypes"):
        DeviceFeatures(ds, DEV)


def test_train_dataset_from_file_equals_from_arrays(tmp_path):
    from src.dataset.embedding_rag_dataset import EmbeddingRAGDataset
    from src.dataset.synthetic import POPS
    from src.dataset.vocab import WordVocab
    rng = np.random.default_rng(6)
    n_sites, n_win, S, R = 120, 2, 5, 12
    n = n_sites * n_win
    af = rng.beta(0.3, 3.0, n).astype(np.float32)
    pos = np.sort(rng.choice(np.arange(1, 50 * n), n, replace=False)).astype(np.int64)
    ref = (rng.random((n, R, 2)) < af[:, None, None]).astype(np.int8)
    vcf = (rng.random((n, S, 2)) < af[:, None, None]).astype(np.int8)
    keep = np.ones(n, bool)
    keep[[5, 130, 131]] = False                               # panel sites missing: window_valid_indices
    freq = rng.random((4, 6, n)).astype(np.float32)
    freq[3, 5] = af
    a = dict(pops=[POPS[i % 5] for i in range(S)], freq=freq, pop_to_idx={p: i for i, p in enumerate(POPS)},
             pos_to_idx={int(p): i for i, p in enumerate(pos)})
    samples = [f"S{i}" for i in range(S)]
    write_common_files(tmp_path, a, samples)
    V().write_gt_vcf(tmp_path / "train.vcf.gz", samples, pos, vcf)
    V().write_gt_vcf(tmp_path / "ref.vcf", [f"R{i}" for i in range(R)], pos[keep], ref[keep])
    bounds = np.array([[w * n_sites, (w + 1) * n_sites] for w in range(n_win)])
    (tmp_path / "win.csv").write_text("start,end\n" + "".join(f"{s},{e}\n" for s, e in bounds))
    vocab = WordVocab(POPS)
    np.random.seed(1)
    mem = EmbeddingRAGDataset.from_arrays(vocab, vcf, pos, a["pops"], freq, bounds, a["pop_to_idx"], a["pos_to_idx"],
                                          ref[keep], pos[keep], name="val", panel_codes="bits")
    np.random.seed(1)
    fil = EmbeddingRAGDataset.from_file(vocab, str(tmp_path / "train.vcf.gz"), tmp_path / "panel.txt",
                                        tmp_path / "freq.npy", tmp_path / "win.csv", tmp_path / "type.pkl",
                                        tmp_path / "pop.pkl", tmp_path / "pos.pkl", ref_vcf_path=str(tmp_path / "ref.vcf"),
                                        name="val", panel_codes="bits")
    assert len(fil) == len(mem) and fil.ref_panel_vcf is not None and fil.vcf_genotypes is not None
    for item in (0, 1, n_win * S - 1):
        x, y = fil[item], mem[item]
        assert x.keys() == y.keys()
        for k in x:
            if torch.is_tensor(x[k]):
                assert torch.equal(x[k], y[k]), k
            else:
                np.testing.assert_array_equal(np.asarray(x[k]), np.asarray(y[k]))
    for w in range(n_win):
        assert torch.equal(fil.panel_index(w, DEV).data, mem.panel_index(w, DEV).data)
