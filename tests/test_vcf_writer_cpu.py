"""The host side of the opt-in device VCF writer (src/vcf_device.py), without a GPU: the integer
'%.3f' rounding the kernel uses (``milli_f32``, csrc/vcf.hip ``milli``) against Python's own
formatting, the flag, the bindings, and the prefix / offset / chunk builder against the lines the
unchanged host ``write_vcf`` writes."""
import re

import numpy as np
import pytest

from conftest import REPO


def _py_milli(v):
    """Python's own formatting of the exact value of the float32, digits without the point."""
    return int(f"{float(np.float32(v)):.3f}".replace(".", ""))


def _near(x):
    v = np.float32(x)
    return [np.nextafter(v, np.float32(-1)), v, np.nextafter(v, np.float32(20))]


def boundary_values():
    vals = []
    for q in range(2001):                                  # rounding boundaries (q + 0.5) / 1000 and neighbours
        vals += _near((q + 0.5) / 1000)
    vals += [np.float32(j / 16) for j in range(1, 33, 2)]  # exact ties: odd sixteenths up to 2
    vals += [np.float32(0), np.float32(1e-45), np.float32(1e-30), np.float32(1.0), np.float32(2.0),
             np.nextafter(np.float32(2), np.float32(3)), np.float32(9.9994)]
    vals += _near(0.0005)
    return np.asarray(vals, np.float32)


def test_milli_f32_matches_python_format_on_boundaries():
    from src.infer_embedding_rag import milli_f32
    v = boundary_values()
    assert v[v > 0].min() == np.float32(1e-45) and np.float32(1e-45) > 0     # the smallest subnormal is in
    got = milli_f32(v)
    want = np.asarray([_py_milli(x) for x in v], np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:10]]
    # the ties of the issue, spelled out: round-half-even on the exact binary value
    assert milli_f32(np.float32([0.0625, 0.1875, 0.3125, 0.4375])).tolist() == [62, 188, 312, 438]


def test_milli_f32_matches_python_format_on_random_bit_patterns():
    from src.infer_embedding_rag import milli_f32
    rng = np.random.default_rng(20240611)
    two = int(np.float32(2.0).view(np.uint32))
    v = rng.integers(0, two + 1, size=200_000, dtype=np.uint32).view(np.float32)   # every f32 in [0, 2] equally likely
    assert v.min() >= 0 and v.max() <= 2
    got = milli_f32(v)
    want = np.asarray([_py_milli(x) for x in v], np.int64)
    assert np.array_equal(got, want)
    # values spread evenly over [0, 2] as well (the bit patterns above crowd towards 0)
    w = (rng.random(20_000) * 2).astype(np.float32)
    assert np.array_equal(milli_f32(w), np.asarray([_py_milli(x) for x in w], np.int64))


def test_milli_f32_marks_what_does_not_fit():
    from src.infer_embedding_rag import milli_f32
    bad = np.float32([np.nan, np.inf, -0.0, -1.0, -1e-30, 9.9995, 10.0, 16.0, 1e30])
    assert (milli_f32(bad) == -1).all()
    assert milli_f32(np.float32([9.9994]))[0] == 9999
    assert milli_f32(np.zeros((3, 2), np.float32)).shape == (3, 2)


def test_flag_parses_and_defaults_to_host():
    from src import infer_embedding_rag as I
    assert I.parse_args([]).vcf_writer == "host"
    assert I.parse_args(["--vcf_writer", "device"]).vcf_writer == "device"
    assert I.parse_args(["--vcf_writer", "host"]).vcf_writer == "host"
    with pytest.raises(SystemExit):
        I.parse_args(["--vcf_writer", "gpu"])
    assert callable(I.write_vcf_device)


def test_export_declared_and_bound_abi_unchanged():
    from src import kernels, native
    header = (REPO / "include" / "snvrag.h").read_text()
    declared = set(re.findall(r"\b(snvrag_[a-z0-9_]+)\s*\(", header))
    assert "snvrag_vcf_format" in declared and "snvrag_vcf_format" in native.EXPORTED
    assert native.ABI_VERSION == 31 and "#define SNVRAG_ABI_VERSION 31" in header
    # one ctypes argument per parameter of the declaration
    decl = header[header.index("int snvrag_vcf_format("):]
    decl = decl[:decl.index(");")]
    assert len(decl.split(",")) == len(native._SIGS["snvrag_vcf_format"][0])
    assert callable(kernels.vcf_format)
    assert (REPO / "rag-snvbert_amd" / "csrc" / "vcf.hip").exists()


def _host_lines(tmp_path, chrom, pos, S, ref, alt, pos_flag=None):
    from src.infer_embedding_rag import write_vcf
    n = len(pos)
    rng = np.random.default_rng(1)
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    gt = rng.random((n, S, 4), dtype=np.float32)
    samples = [f"S{i}" for i in range(S)]
    write_vcf(tmp_path / "host.vcf", chrom, pos, h1, h2, gt, samples, pos_flag=pos_flag, ref=ref, alt=alt)
    lines = (tmp_path / "host.vcf").read_bytes().split(b"\n")
    assert lines[-1] == b""
    lines = [ln + b"\n" for ln in lines[:-1]]
    head = [ln for ln in lines if ln.startswith(b"#")]
    return b"".join(head), lines[len(head):], samples


def test_prefixes_and_offsets_equal_the_host_writer_lines(tmp_path):
    from src import vcf_device as V
    pos = np.asarray([7, 31, 48213, 5, 123456789], np.int64)
    flag = np.asarray([True, False, True, False, True])
    ref, alt = ["A", "C", "GATTACA", "T", "G"], ["T", "G", "G", "TTTT", "ACGTACGTAC"]
    S = 3
    head, body, samples = _host_lines(tmp_path, "chr21", pos, S, ref, alt, flag)
    assert len(body) == 3
    assert V.header_lines(samples).encode() == head
    rows, blob, p_off = V.site_prefixes("chr21", pos, flag, ref, alt)
    assert rows.tolist() == [0, 2, 4] and rows.dtype == np.int32 and p_off.dtype == np.int32
    assert p_off[0] == 0 and p_off[-1] == len(blob)
    length = V.line_lengths(p_off, S)
    assert length.tolist() == [len(ln) for ln in body]
    for i, ln in enumerate(body):
        assert ln.startswith(blob[p_off[i]:p_off[i + 1]])
        assert len(ln) - (p_off[i + 1] - p_off[i]) == V.CELL_BYTES * S       # every cell is 39 bytes + separator
    # chunk plans over these very lines: the third is the longest, and no two fit in its length
    l0, l1, l2 = (int(x) for x in length)
    assert l2 == max(l0, l1, l2) and l0 + l1 > l2 + 1
    assert V.plan_chunks(length, l2) == [(0, 1), (1, 2), (2, 3)]
    assert V.plan_chunks(length, l2 + 1) == [(0, 1), (1, 2), (2, 3)]
    assert V.plan_chunks(length, l0 + l1 - 1) == [(0, 1), (1, 2), (2, 3)]
    assert V.plan_chunks(length, l0 + l1) == [(0, 2), (2, 3)]
    assert V.plan_chunks(length, l0 + l1 + l2) == [(0, 3)]
    with pytest.raises(ValueError, match="does not fit"):
        V.plan_chunks(length, l2 - 1)
    # no ref / alt and no flag: every site, '.' alleles
    _, body, _ = _host_lines(tmp_path, "21", pos, S, None, None)
    rows, blob, p_off = V.site_prefixes("21", pos)
    assert rows.tolist() == [0, 1, 2, 3, 4]
    assert V.line_lengths(p_off, S).tolist() == [len(ln) for ln in body]


def test_chunk_plan_splits_where_expected():
    from src import vcf_device as V
    length = np.asarray([100, 100, 100, 100, 100], np.int64)
    assert V.plan_chunks(length, 100) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]      # exactly one line
    assert V.plan_chunks(length, 101) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]      # one line plus 1
    assert V.plan_chunks(length, 200) == [(0, 2), (2, 4), (4, 5)]
    assert V.plan_chunks(length, 299) == [(0, 2), (2, 4), (4, 5)]
    assert V.plan_chunks(length, 300) == [(0, 3), (3, 5)]
    assert V.plan_chunks(length, 1 << 20) == [(0, 5)]
    assert V.plan_chunks(np.zeros(0, np.int64), 100) == []
    ragged = np.asarray([60, 50, 70, 120, 10], np.int64)
    assert V.plan_chunks(ragged, 120) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert V.plan_chunks(ragged, 121) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert V.plan_chunks(ragged, 130) == [(0, 2), (2, 3), (3, 5)]
    with pytest.raises(ValueError, match="does not fit"):
        V.plan_chunks(ragged, 119)                                                    # the over-long line
    with pytest.raises(ValueError, match="1 GiB"):
        V.plan_chunks(ragged, (1 << 30) + 1)
    assert V.plan_chunks(ragged, 1 << 30) == [(0, 5)]
