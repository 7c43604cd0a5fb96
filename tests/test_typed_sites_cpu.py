"""Typed sites in the imputed VCF without a GPU: the numpy specification of the overlay kernel
(``typed_sites.typed_overlay_host``) against a cell-by-cell loop, the packing of a genotype array into the target's
bit rows, the INFO strings and header line of ``--vcf_sites all``, the host writer's text over overlaid arrays, the
command line's precondition, and the new prototype in the header against ``native._SIGS``.
"""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
from src import native  # noqa: E402
from src import quality as Q  # noqa: E402
from src import typed_sites as T  # noqa: E402
from src import vcf_device as VD  # noqa: E402
from src.infer_embedding_rag import parse_args, write_vcf  # noqa: E402

NAN_PATTERN = np.uint32(0x7fc0a5a5)             # a NaN with a payload: equal only bit for bit


def nan_fill(shape):
    return np.full(shape, NAN_PATTERN, np.uint32).view(np.float32).copy()


def bit_of(bits, row, r):
    return (int(bits[row, r >> 3]) >> (r & 7)) & 1


def overlay_loop(h1, h2, gt, alt, miss, n_target, site_row, col):
    """The rule of the issue, one cell at a time."""
    n, S = h1.shape
    missing = np.zeros(n, np.int32)
    for i in range(n):
        r = int(site_row[i])
        if not 0 <= r < n_target:
            continue
        for s in range(S):
            c = int(col[s])
            if not 0 <= c < alt.shape[0] // 2:
                continue
            a1, a2 = bit_of(alt, 2 * c, r), bit_of(alt, 2 * c + 1, r)
            if bit_of(miss, 2 * c, r) | bit_of(miss, 2 * c + 1, r):
                missing[i] += 1
                continue
            h1[i, s], h2[i, s] = a1, a2
            gt[i, s] = 0.0
            gt[i, s, 2 * a1 + a2] = 1.0
    return missing


def random_bits(rng, S_target, n_target, ld, miss_rate=0.1):
    """(alt, miss) u8 [2 S_target, ld]: missing on one haplotype, on both, and none; bits past n_target random."""
    alt = rng.integers(0, 256, (2 * S_target, ld), dtype=np.uint8)
    one = np.packbits(rng.random((2 * S_target, 8 * ld)) < miss_rate, axis=1, bitorder="little")
    both = np.packbits(rng.random((S_target, 8 * ld)) < miss_rate / 2, axis=1, bitorder="little")
    miss = one | np.repeat(both, 2, axis=0)
    return alt, miss


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlay_host_equals_the_cell_loop(seed):
    rng = np.random.default_rng(seed)
    n, S, S_target, n_target, ld = 23, 7, 9, 29, 5
    alt, miss = random_bits(rng, S_target, n_target, ld)
    site_row = rng.integers(0, n_target, n).astype(np.int32)
    site_row[[1, 5]] = -1
    site_row[2], site_row[3] = n_target, 8 * ld + 3             # out of range, and past the bit rows
    site_row[6] = site_row[7] = n_target - 1                    # repeated; the last record
    site_row[8:12] = [20, 13, 13, 2]                            # decreasing
    col = rng.permutation(S_target)[:S].astype(np.int32)
    col[2], col[4] = -1, S_target
    got, want = [nan_fill((n, S)), nan_fill((n, S)), nan_fill((n, S, 4))], None
    want = [a.copy() for a in got]
    m_want = overlay_loop(*want, alt, miss, n_target, site_row, col)
    m_got = T.typed_overlay_host(*got, alt, miss, n_target, site_row, col)
    assert m_got.dtype == np.int32 and np.array_equal(m_got, m_want) and m_want.sum() > 0
    for g, w in zip(got, want):
        assert same_bits(g, w)
    # the untouched cells are the fill, bit for bit: unmapped rows and columns, and the missing calls
    keep = got[0].view(np.uint32) == NAN_PATTERN
    assert keep[[1, 2, 3, 5]].all() and keep[:, [2, 4]].all()
    valid_rows = np.flatnonzero((site_row >= 0) & (site_row < n_target))
    assert int(keep[valid_rows][:, [0, 1, 3, 5, 6]].sum()) == int(m_want.sum())
    assert (got[2].view(np.uint32)[keep] == NAN_PATTERN).all() and (got[1].view(np.uint32)[keep] == NAN_PATTERN).all()
    written = got[2][~keep]
    assert set(np.unique(written)) <= {0.0, 1.0} and (written.sum(1) == 1).all()


def test_overlay_host_nothing_mapped_and_refusals():
    alt, miss = np.zeros((4, 2), np.uint8), np.zeros((4, 2), np.uint8)
    h1, h2, gt = nan_fill((3, 2)), nan_fill((3, 2)), nan_fill((3, 2, 4))
    m = T.typed_overlay_host(h1, h2, gt, alt, miss, 10, [-1, -1, 99], [0, 1])
    assert not m.any() and (h1.view(np.uint32) == NAN_PATTERN).all() and (gt.view(np.uint32) == NAN_PATTERN).all()
    m = T.typed_overlay_host(h1, h2, gt, alt, miss, 10, [0, 1, 2], [-1, 7])
    assert not m.any() and (h2.view(np.uint32) == NAN_PATTERN).all()
    with pytest.raises(ValueError):
        T.typed_overlay_host(h1, h2, gt, alt, miss, 17, [0, 1, 2], [0, 1])      # 8 ld_bits < n_target
    with pytest.raises(ValueError):
        T.typed_overlay_host(h1, h2, gt, alt, miss, 10, [0, 1], [0, 1])
    with pytest.raises(TypeError):
        T.typed_overlay_host(h1.astype(np.float64), h2, gt, alt, miss, 10, [0, 1, 2], [0, 1])


def unpack_gt_numpy(alt, miss, n_sites):
    """``vcf_unpack_gt_kernel`` restated: i8 [n_sites, S, 2], 0 / 1 from the ALT bits, -1 where missing."""
    a = np.unpackbits(alt, axis=1, bitorder="little")[:, :n_sites].astype(np.int8)
    m = np.unpackbits(miss, axis=1, bitorder="little")[:, :n_sites].astype(bool)
    g = np.where(m, np.int8(-1), a)                                             # [2 S, n]
    return np.ascontiguousarray(g.reshape(-1, 2, n_sites).transpose(2, 0, 1))


class _Target:
    vcf_genotypes = None

    def __init__(self, vcf):
        self.vcf = vcf


@pytest.mark.parametrize("n_target,S", [(1, 1), (8, 3), (9, 2), (63, 5), (64, 1), (65, 4), (300, 6)])
def test_target_bit_rows_round_trip(n_target, S):
    rng = np.random.default_rng(n_target)
    vcf = rng.choice(np.array([-1, 0, 1, 2], np.int8), (n_target, S, 2), p=[0.1, 0.5, 0.3, 0.1])
    alt, miss, n, s = T.target_bit_rows(_Target(vcf))
    assert (n, s) == (n_target, S) and alt.dtype == miss.dtype == np.uint8
    assert alt.shape == miss.shape == (2 * S, alt.shape[1]) and alt.shape[1] % 8 == 0 and 8 * alt.shape[1] >= n_target
    assert alt.flags.c_contiguous and alt.ctypes.data % 8 == 0 and miss.ctypes.data % 8 == 0
    assert not (alt & miss).any()                                               # an ALT bit is 0 where missing
    want = np.where(vcf < 0, -1, (vcf > 0).astype(np.int8)).astype(np.int8)
    assert np.array_equal(unpack_gt_numpy(alt, miss, n_target), want)
    # bits past the last record are 0
    assert not np.unpackbits(alt | miss, axis=1, bitorder="little")[:, n_target:].any()


def test_info_strings_imputed_flag():
    af, r2, dr2 = np.array([0.25, 0.0, 1.0]), np.array([0.5, 0.0, 1.0]), np.array([0.125, 1.0, 0.0])
    today = ["AF=%.4f;DR2=%.3f;R2=%.3f;IMP" % (a, d, r) for a, r, d in zip(af, r2, dr2)]
    assert Q.info_strings(af, r2, dr2) == today == Q.info_strings(af, r2, dr2, imputed=None)
    assert today[0] == "AF=0.2500;DR2=0.125;R2=0.500;IMP"
    assert Q.info_strings(af, r2, dr2, imputed=np.array([True, False, True])) == [
        "AF=0.2500;DR2=0.125;R2=0.500;IMP", "AF=0.0000;DR2=1.000;R2=0.000;TYPED", "AF=1.0000;DR2=0.000;R2=1.000;IMP"]
    with pytest.raises(ValueError):
        Q.info_strings(af, r2, dr2, imputed=[True])


TYPED_LINE = '##INFO=<ID=TYPED,Number=0,Type=Flag,Description="Site genotyped in the target">\n'


def six_sites():
    """6 sites x 3 samples of model output, a target of 4 records x 3 samples typed at sites 0, 2, 3, 5."""
    n, S = 6, 3
    h1 = np.full((n, S), 0.25, np.float32)
    h2 = np.full((n, S), 0.75, np.float32)
    gt = np.tile(np.array([0.125, 0.25, 0.5, 0.125], np.float32), (n, S, 1))
    vcf = np.array([[[0, 0], [0, 1], [1, 0]],
                    [[1, 1], [-1, 0], [0, 0]],                                  # a half-missing call
                    [[1, 0], [1, 1], [-1, -1]],                                 # a missing call
                    [[0, 1], [0, 0], [1, 1]]], np.int8)
    site_row = np.array([0, -1, 1, 3, -1, 2], np.int32)                         # not increasing
    return h1, h2, gt, vcf, site_row


MODEL_CELL = "1|0:0.250,0.750:0.125,0.750,0.125:1.000"
CELL = {(0, 0): "0|0:0.000,0.000:1.000,0.000,0.000:0.000", (0, 1): "0|1:0.000,1.000:0.000,1.000,0.000:1.000",
        (1, 0): "1|0:1.000,0.000:0.000,1.000,0.000:1.000", (1, 1): "1|1:1.000,1.000:0.000,0.000,1.000:2.000"}


def test_write_vcf_after_the_host_overlay(tmp_path):
    h1, h2, gt, vcf, site_row = six_sites()
    alt, miss, n_target, S = T.target_bit_rows(_Target(vcf))
    missing = T.typed_overlay_host(h1, h2, gt, alt, miss, n_target, site_row, np.arange(S))
    assert missing.tolist() == [0, 0, 1, 0, 0, 1]
    pos, samples = [100, 200, 300, 400, 500, 600], ["A", "B", "C"]
    imputed = site_row < 0
    info = Q.info_strings(np.zeros(6), np.zeros(6), np.zeros(6), imputed=imputed)
    write_vcf(tmp_path / "all.vcf", "7", pos, h1, h2, gt, samples, pos_flag=None, info=info, typed=True)
    rows = []
    for i, p in enumerate(pos):
        r = int(site_row[i])
        cells = [MODEL_CELL if r < 0 or (vcf[r, s] < 0).any() else CELL[tuple(vcf[r, s].tolist())] for s in range(3)]
        flag = "IMP" if r < 0 else "TYPED"
        rows.append(f"7\t{p}\t.\t.\t.\t0.0\tPASS\tAF=0.0000;DR2=0.000;R2=0.000;{flag}\tGT:HDS:GP:DS\t" + "\t".join(cells) + "\n")
    assert (tmp_path / "all.vcf").read_text() == VD.header_lines(samples, info=True, typed=True) + "".join(rows)
    assert rows[0].endswith("\t".join([CELL[0, 0], CELL[0, 1], CELL[1, 0]]) + "\n")
    assert rows[2].endswith("\t".join([CELL[1, 1], MODEL_CELL, CELL[0, 0]]) + "\n")


def test_typed_header_line_only_when_asked(tmp_path):
    assert VD.TYPED_HEADER == TYPED_LINE
    h1, h2, gt, _, _ = six_sites()
    samples, pos = ["A", "B", "C"], list(range(1, 7))
    info = ["X=1"] * 6
    for kw_info in (None, info):
        plain = VD.header_lines(samples, info=kw_info is not None)
        asked = VD.header_lines(samples, info=kw_info is not None, typed=True)
        assert TYPED_LINE not in plain and asked.count(TYPED_LINE) == 1 and asked.replace(TYPED_LINE, "") == plain
        assert asked.index(TYPED_LINE) < asked.index("##FORMAT")
        if kw_info is not None:
            assert asked.index("ID=IMP") < asked.index(TYPED_LINE)
        write_vcf(tmp_path / "p.vcf", "1", pos, h1, h2, gt, samples, info=kw_info)
        write_vcf(tmp_path / "t.vcf", "1", pos, h1, h2, gt, samples, info=kw_info, typed=True)
        p, t = (tmp_path / "p.vcf").read_text(), (tmp_path / "t.vcf").read_text()
        assert p.startswith(plain) and t.startswith(asked) and t.replace(TYPED_LINE, "") == p


def test_parse_args_vcf_sites(capsys):
    base = ["--synthetic", "2"]
    assert parse_args(base).vcf_sites == "imputed"
    assert parse_args(base + ["--vcf_sites", "all", "--index_window_len", "1020"]).vcf_sites == "all"
    assert parse_args(base + ["--vcf_sites", "all", "--window_len", "510"]).vcf_sites == "all"
    for extra in (["--index_window_len", "510"], []):                           # 510 is also the default
        with pytest.raises(SystemExit):
            parse_args(base + ["--vcf_sites", "all"] + extra)
        assert "--vcf_sites all needs --index_window_len equal to --window_len" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(base + ["--vcf_sites", "typed"])


def test_prototype_and_abi_version():
    assert native.ABI_VERSION == 31
    header = (REPO / "include" / "snvrag.h").read_text()
    assert re.search(r"#define SNVRAG_ABI_VERSION 31\b", header)
    m = re.search(r"int snvrag_typed_overlay\(([^)]*)\);", header)
    args = [a.strip() for a in m.group(1).split(",")]
    kinds = [C.c_void_p if "*" in a else {"int64_t": C.c_int64}[a.split()[0]] for a in args]
    assert native._SIGS["snvrag_typed_overlay"] == (kinds, C.c_int) and len(kinds) == 14
    names = [re.split(r"[\s\*]+", a)[-1] for a in args]
    assert names == ["alt_bits", "miss_bits", "ld_bits", "n_target", "S_target", "site_row", "col", "n", "S", "h1", "h2",
                     "gt", "missing", "stream"]
