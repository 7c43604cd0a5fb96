"""GPU tests of the panel tables: the counting kernel (csrc/panel_stats.hip) against its specification
``panel_counts_host`` bit for bit over the sizes at which it changes path (one lane, a partial dword, the tile
of 64 dword columns = 2048 sites, more than one sample group per wave, empty and one-sample populations) with
every row stride and row alignment, from a file through ``read_vcf`` -> ``build_tables``, its refused calls,
and imputation from VCFs alone (``--ref_panel_pops``) against the same run through ``build_panel_stats``' files."""
import gzip
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_panel_stats_cpu import random_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_SITES = 64 * 32                     # PS_COLS dword columns of 32 sites per workgroup
N_SITES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, TILE_SITES - 1, TILE_SITES, TILE_SITES + 1)
GARBAGE, SENTINEL = 0x5A5A5A5A, -7


def PS():
    from src.dataset import panel_stats
    return panel_stats


def bit_rows(gt):
    """(alt, miss) u8 [2 S, ceil(n / 8)] of gt [n, S, 2]: row 2 s + h, site r at bit r & 7 of byte r >> 3, the
    bits of the last byte past n set to 1."""
    n, S = gt.shape[:2]
    rows = gt.transpose(1, 2, 0).reshape(2 * S, n)
    out = []
    for bits in ((rows > 0), (rows < 0)):
        b = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little"))
        if n % 8:
            b[:, -1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
        out.append(b)
    return out


def strided(rows, ld, offset):
    """The rows as a device view of row stride ``ld`` that begins ``offset`` bytes into an allocation and ends
    with the last row's last byte; every byte between the rows is 0xFF."""
    R, nb = rows.shape
    flat = np.full(offset + (R - 1) * ld + nb, 0xFF, np.uint8)
    for r in range(R):
        flat[offset + r * ld:offset + r * ld + nb] = rows[r]
    buf = torch.from_numpy(flat).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return torch.as_strided(buf, (R, nb), (ld, 1), storage_offset=offset)


def launch(alt, miss, n, order, pop_start):
    """Counts through sentinel rows and a garbage pre-fill; two launches."""
    from src import kernels as K
    big = torch.full((8, 5, n), GARBAGE, device=DEV, dtype=torch.int32)
    big[0], big[7] = SENTINEL, SENTINEL
    o, ps = torch.from_numpy(order).to(DEV), torch.from_numpy(pop_start).to(DEV)
    first = K.panel_counts(alt, miss, n, o, ps, out=big[1:7]).clone()
    big[1:7] = GARBAGE + 1
    second = K.panel_counts(alt, miss, n, o, ps, out=big[1:7])
    assert torch.equal(first, second)
    assert bool((big[0] == SENTINEL).all()) and bool((big[7] == SENTINEL).all())
    return first.cpu().numpy()


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 130])
def test_kernel_equals_the_host_specification(S):
    combos = 0
    for n in N_SITES:
        nb = (n + 7) // 8
        lds = (nb, nb + 1, nb + 3, (nb + 63) // 64 * 64)
        for P in (1, 2, 5):
            gt, order, pop_start = random_case(n, S, P, seed=1000 * S + 10 * n + P, missing=0.1)
            if S > P > 1:
                assert pop_start[1] == 1 and (order != np.arange(S)).any()      # a population of one sample
            want = PS().panel_counts_host(gt, order, pop_start, P)
            alt, miss = bit_rows(gt)
            for ld in lds:
                for offset in (0, 1, 3):
                    got = launch(strided(alt, ld, offset), strided(miss, ld, offset), n, order, pop_start)
                    np.testing.assert_array_equal(got, want, err_msg=f"n={n} P={P} ld={ld} offset={offset}")
                    assert not got[P:5].any()
                    combos += 1
    assert combos == len(N_SITES) * 3 * 4 * 3


def test_more_samples_than_one_flush_holds():
    """2100 samples in one population: a wave's share (263) is more than the 248 samples a bit-sliced counter
    holds between two flushes, and the counts pass 255."""
    S, n = 2100, 70
    gt, order, pop_start = random_case(n, S, 2, seed=3, missing=0.05)
    want = PS().panel_counts_host(gt, order, pop_start, 2)
    assert want[1].max() > 2000
    alt, miss = bit_rows(gt)
    got = launch(strided(alt, 9, 1), strided(miss, 9, 1), n, order, pop_start)
    np.testing.assert_array_equal(got, want)


def test_alt_bit_under_a_missing_bit_and_a_bad_sample_number():
    from src import kernels as K
    gt, order, pop_start = random_case(40, 6, 2, seed=8, missing=0.3)
    want = PS().panel_counts_host(gt, order, pop_start, 2)
    alt, miss = bit_rows(gt)
    a, m = torch.from_numpy(alt | miss).to(DEV), torch.from_numpy(miss).to(DEV)     # ALT set wherever missing
    o, ps = torch.from_numpy(order).to(DEV), torch.from_numpy(pop_start).to(DEV)
    np.testing.assert_array_equal(K.panel_counts(a, m, 40, o, ps).cpu().numpy(), want)
    bad = order.copy()
    drop = int(bad[2])
    bad[2] = 6                                                # outside [0, S): loads nothing, counts nothing
    keep = np.array([s for s in order if s != drop], np.int32)
    starts = np.array([0, pop_start[1], 5], np.int32)
    want = PS().panel_counts_host(gt, keep, starts, 2)
    got = K.panel_counts(a, m, 40, torch.from_numpy(bad).to(DEV), ps).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def panel_arrays(n, S, seed):
    """(gt, pos, names) of a panel with allele numbers 0..2 and 12 % of the alleles missing."""
    rng = np.random.default_rng(seed)
    gt = rng.choice(np.array([0, 0, 1, 1, 2], np.int8), (n, S, 2))
    gt[rng.random((n, S, 2)) < 0.12] = -1
    pos = np.cumsum(rng.integers(1, 50, n)).astype(np.int32)
    return gt, pos, [f"R{i}" for i in range(S)]


def write_panel(path, names, pos, gt):
    """write_gt_vcf's file with '/' in every second record's cells and the haploid call 'a' in place of 'a|.'."""
    from src.dataset import vcf_reader as V
    plain = str(path)[:-3] if str(path).endswith(".gz") else str(path)
    V.write_gt_vcf(plain, names, pos, gt)
    with open(plain) as f:
        lines = f.read().split("\n")[:-1]
    out = []
    for i, line in enumerate(lines):
        if not line.startswith("#"):
            cols = line.split("\t")
            cells = cols[9:]
            if i % 2:
                cells = [c.replace("|", "/") for c in cells]
            cells = [re.sub(r"^([0-9]+)[|/]\.$", r"\1", c) for c in cells]
            line = "\t".join(cols[:9] + cells)
        out.append(line)
    data = ("\n".join(out) + "\n").encode()
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)


def write_panel_file(path, names, pops, extra=()):
    with open(path, "w") as f:
        f.write("sample\tpop\tsuper_pop\tgender\n")
        for s, p in list(zip(names, pops)) + list(extra):
            f.write(f"{s}\tX\t{p}\tmale\n")


@pytest.mark.parametrize("name", ["panel.vcf", "panel.vcf.gz"])
def test_tables_from_a_file(tmp_path, name):
    from src.dataset import vcf_reader as V
    gt, pos, names = panel_arrays(300, 21, seed=4)
    path = tmp_path / name
    write_panel(path, names, pos, gt)
    with V._open(path) as fh:
        cells = {c for line in fh.read().split(b"#CHROM")[1].split(b"\n")[1:] for c in line.split(b"\t")[9:]}
    assert {b"1", b"0", b"./.", b".|.", b"1/0", b"0|1", b".|2", b"./1"} <= cells      # haploid, missing, '/' calls
    pops = [("EUR", "AFR", "EAS")[(i + i // 5) % 3] for i in range(21)]
    write_panel_file(tmp_path / "p.panel", names[::-1], pops[::-1], extra=[("NOT_IN_VCF", "SAS")])
    samples, hpos, hgt = V.parse_vcf_host(path)
    assert samples == names and (hgt[:, :, 1] < 0).any() and (hgt > 1).any()
    pop_list, order, pop_start = PS().population_order(samples, names, pops)
    assert pop_list == ["AFR", "EAS", "EUR"]
    want = PS().panel_counts_host(hgt, order, pop_start, 3)
    vg = V.read_vcf(path, DEV)
    assert vg.any_missing and not vg.phased
    t = PS().build_tables(vg, tmp_path / "p.panel", DEV)
    assert t["counts"].dtype == np.int32 and t["freq"].dtype == np.float32
    np.testing.assert_array_equal(t["counts"], want)
    np.testing.assert_array_equal(t["freq"], PS().freq_from_counts(want))
    assert (t["pop_to_idx"], t["pos_to_idx"]) == PS().maps(pop_list, hpos)
    assert t["type_to_idx"] == {} and list(t["pos_to_idx"]) == [int(p) for p in hpos]


def test_refused_calls():
    from src import native
    lib = native.load()
    S, n, P = 3, 20, 2
    guard = torch.full((4096,), 0xA5, device=DEV, dtype=torch.uint8)
    ref = guard.clone()
    at = lambda i: guard[256 * i:].data_ptr()
    good = dict(alt=at(0), miss=at(1), ld=3, S=S, n=n, order=at(2), pop_start=at(3), P=P, counts=at(4))

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.snvrag_panel_counts(a["alt"], a["miss"], a["ld"], a["S"], a["n"], a["order"], a["pop_start"], a["P"],
                                     a["counts"], None)
        return rc, lib.snvrag_last_error().decode()

    cases = [dict(alt=None), dict(miss=None), dict(order=None), dict(pop_start=None), dict(counts=None), dict(S=0),
             dict(S=-1), dict(P=0), dict(P=6), dict(ld=2), dict(n=-1), dict(n=-1, ld=0)]
    for kw in cases:
        rc, text = call(**kw)
        assert rc != 0 and text.startswith("panel_counts_args: ") and len(text) > 25, (kw, rc, text)
    assert call(alt=None)[1] == "panel_counts_args: null pointer"
    assert "P must be in [1, 5]" in call(P=6)[1] and "ld_bits" in call(ld=2)[1] and "n_sites" in call(n=-1)[1]
    assert call(n=0, ld=0)[0] == 0                            # nothing to count: no launch
    torch.cuda.synchronize()
    assert torch.equal(guard, ref), "a refused call wrote to a buffer it was passed"


def test_imputation_from_vcfs_alone_equals_the_tool_files(tmp_path, monkeypatch):
    """target.vcf, panel.vcf.gz and their .panel files, nothing else: build_dataset with --ref_panel_pops against
    build_panel_stats' four files through the old flags; the panel file is read once on the flag path."""
    from src import build_panel_stats
    from src.dataset import vcf_reader as V
    from src.dataset.synthetic import POPS, make_infer_arrays
    from src.engine import engine_for
    from src.infer_embedding_rag import build_dataset, parse_args, run
    from src.model import build_model
    a = make_infer_arrays(1300, 6, 24, missing_rate=0.3, ref_missing=0, seed=11)
    samples, refs = [f"S{i}" for i in range(6)], [f"R{i}" for i in range(24)]
    target, panel = str(tmp_path / "target.vcf"), str(tmp_path / "panel.vcf.gz")
    V.write_gt_vcf(target, samples, a["pos"], a["vcf"])
    V.write_gt_vcf(panel, refs, a["ref_pos"], a["ref_gt"])
    write_panel_file(tmp_path / "target.panel", samples, a["pops"])
    write_panel_file(tmp_path / "panel.panel", refs, [POPS[(3 * i) % 5] for i in range(24)])
    common = ["--infer_dataset", target, "--infer_panel", str(tmp_path / "target.panel"), "--ref_panel", panel,
              "-d", "64", "-l", "2", "-a", "2", "-b", "4", "--k_retrieve", "3"]
    reads = []
    real = V.read_vcf
    monkeypatch.setattr(V, "read_vcf", lambda path, *args, **kw: (reads.append(str(path)), real(path, *args, **kw))[1])

    ds_flag, vocab = build_dataset(parse_args(common + ["--ref_panel_pops", str(tmp_path / "panel.panel")]))
    assert reads.count(panel) == 1 and reads.count(target) == 1
    assert ds_flag.ref_panel_vcf is not None and ds_flag.vcf_genotypes is not None
    np.testing.assert_array_equal(ds_flag.ori_pos, a["ref_pos"])

    out = tmp_path / "tables"
    paths = build_panel_stats.main(["--ref_panel", panel, "--ref_panel_pops", str(tmp_path / "panel.panel"),
                                    "-o", str(out)])
    np.testing.assert_array_equal(np.load(paths["freq"]), ds_flag.freq)
    assert np.load(paths["freq"]).dtype == np.float32 and ds_flag.freq.shape == (4, 6, len(a["ref_pos"]))
    ds_files, _ = build_dataset(parse_args(common + ["--freq_path", paths["freq"], "--type_path", paths["type_to_idx"],
                                                     "--pop_path", paths["pop_to_idx"],
                                                     "--pos_path", paths["pos_to_idx"]]))
    assert ds_files.pop_to_idx == ds_flag.pop_to_idx and ds_files.pos_to_idx == ds_flag.pos_to_idx
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = build_model(len(vocab), 64, 2, 2).to(dev).eval()
    engine_for(model).set_dtype(torch.float32)
    got = run(ds_flag, model, dev, 4, 3)
    want = run(ds_files, model, dev, 4, 3)
    for k in ("h1", "h2", "gt", "mask", "idx1", "idx2"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["mask"].any() and np.isfinite(got["gt"]).all()


def test_a_target_population_the_panel_lacks_is_named(tmp_path):
    from src.dataset import vcf_reader as V
    from src.dataset.synthetic import make_infer_arrays
    from src.infer_embedding_rag import build_dataset, parse_args
    a = make_infer_arrays(200, 3, 8, seed=2)
    samples, refs = ["S0", "S1", "S2"], [f"R{i}" for i in range(8)]
    V.write_gt_vcf(tmp_path / "t.vcf", samples, a["pos"], a["vcf"])
    V.write_gt_vcf(tmp_path / "p.vcf", refs, a["ref_pos"], a["ref_gt"])
    write_panel_file(tmp_path / "t.panel", samples, ["AFR", "OCE", "EUR"])
    write_panel_file(tmp_path / "p.panel", refs, ["AFR", "EUR"] * 4)
    args = parse_args(["--infer_dataset", str(tmp_path / "t.vcf"), "--infer_panel", str(tmp_path / "t.panel"),
                       "--ref_panel", str(tmp_path / "p.vcf"), "--ref_panel_pops", str(tmp_path / "p.panel")])
    with pytest.raises(ValueError, match="'OCE'"):
        build_dataset(args)
