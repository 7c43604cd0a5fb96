"""The site columns (CHROM, ID, REF, ALT) without a GPU: the host specification ``site_columns_host`` on
hand-written bytes, the writers' ``ids`` / ``ref`` / ``alt`` columns byte for byte, and the refusals of
``--vcf_site_columns``."""
import gzip

import numpy as np
import pytest

HEAD = b"##fileformat=VCFv4.2\n##x=<a\tb>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\n"


def V():
    from src.dataset import vcf_reader
    return vcf_reader


def rec(chrom, pos, id_, ref, alt, tail=b".\tPASS\t.\tGT\t0|1\t1|1"):
    return b"\t".join([chrom, str(pos).encode(), id_, ref, alt, tail])


def test_lf_crlf_blank_lines_empty_columns_and_a_last_line_without_newline():
    body = (rec(b"chr21", 5, b"rs1", b"A", b"C,T") + b"\n" +
            b"\n" +                                                    # a blank line vanishes
            rec(b"chr21", 6, b"rs2;x", b"GATTACA", b"G") + b"\r\n" +   # CRLF
            b"\r\n" +                                                  # a blank CRLF line vanishes
            rec(b"1", 7, b"", b"", b"") + b"\n" +                      # empty ID, REF and ALT
            rec(b"", 8, b".", b"N", b"<DEL>") + b"\r\n" +              # empty CHROM
            rec(b"chrX", 9, b"last", b"T", b"TT"))                     # no newline at the end
    c = V().site_columns_host(HEAD + body)
    assert len(c) == 5
    assert c.column("chrom") == [b"chr21", b"chr21", b"1", b"", b"chrX"]
    assert c.column("id") == [b"rs1", b"rs2;x", b"", b".", b"last"]
    assert c.column("ref") == [b"A", b"GATTACA", b"", b"N", b"T"]
    assert c.column("alt") == [b"C,T", b"G", b"", b"<DEL>", b"TT"]
    assert c.ref_len.tolist() == [1, 7, 0, 1, 1] and c.ref_len.dtype == np.int64
    assert c.lengths("alt").tolist() == [3, 1, 0, 5, 2]
    assert (c.chrom(4), c.id(1), c.ref(1), c.alt(3)) == (b"chrX", b"rs2;x", b"GATTACA", b"<DEL>")
    for name in V().COLUMN_NAMES:
        off, blob = getattr(c, name + "_off"), getattr(c, name + "_blob")
        assert off.dtype == np.int64 and off.shape == (6,) and blob.dtype == np.uint8 and off[-1] == blob.size
    with pytest.raises(IndexError):
        c.ref(5)
    # the same records as parse_vcf_host sees them
    samples, pos, gt = V().parse_vcf_host(HEAD + body)
    assert samples == ["A", "B"] and pos.tolist() == [5, 6, 7, 8, 9]


def test_short_lines_and_a_last_line_ending_in_cr():
    body = b"chr1\t5\trs7\tACGT\r\n" + b"chr1\t5\n" + b"chr1\t5\trs7\tAC\tT\r"
    c = V().site_columns_host(HEAD + body)
    assert c.column("chrom") == [b"chr1"] * 3 and c.column("id") == [b"rs7", b"", b"rs7"]
    assert c.column("ref") == [b"ACGT", b"", b"AC"] and c.column("alt") == [b"", b"", b"T"]
    assert V().record_columns(b"a\tb\tc\td\te\tf\r") == (b"a", b"c", b"d", b"e")


def test_gz_input_empty_body_and_missing_header(tmp_path):
    data = HEAD + rec(b"chr2", 11, b"a", b"C", b"G") + b"\n" + rec(b"chr2", 12, b"b", b"CC", b"G,GA") + b"\n"
    want = V().site_columns_host(data)
    assert V().site_columns_host(gzip.compress(data)).column("alt") == [b"G", b"G,GA"]
    (tmp_path / "a.vcf.gz").write_bytes(gzip.compress(data))
    (tmp_path / "a.vcf").write_bytes(data)
    for name in ("a.vcf.gz", "a.vcf"):
        got = V().site_columns_host(tmp_path / name)
        for col in V().COLUMN_NAMES:
            assert got.column(col) == want.column(col)
    empty = V().site_columns_host(HEAD)
    assert len(empty) == 0 and empty.ref_len.size == 0 and empty.column("id") == []
    with pytest.raises(ValueError, match="no #CHROM header"):
        V().site_columns_host(b"##fileformat=VCFv4.2\n")
    assert V().VcfGenotypes(["A"], np.zeros(0, np.int32), None, None, 0, False, True).columns is None


def _arrays(n, S):
    rng = np.random.default_rng(1)
    return (rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32),
            rng.random((n, S, 4), dtype=np.float32))


def test_writer_columns_equal_the_prefixes_byte_for_byte(tmp_path):
    from src import vcf_device as D
    from src.infer_embedding_rag import write_vcf
    pos = np.asarray([7, 31, 48213, 50000, 123456789], np.int64)
    flag = np.asarray([True, False, True, True, True])
    ids = ["rs1", "skipped", ".", "rs77;esv3", "chr21:123456789:G:A"]
    ref, alt = ["A", "C", "ACGT" * 10, "T", "G"], ["T", "G", "A", "TA,TAA", "<DEL>"]
    S = 3
    samples = ["HG00096", "NA12878", "s 3"]
    h1, h2, gt = _arrays(len(pos), S)
    write_vcf(tmp_path / "cols.vcf", "chr21", pos, h1, h2, gt, samples, pos_flag=flag, ref=ref, alt=alt, ids=ids)
    data = (tmp_path / "cols.vcf").read_bytes()
    head = D.header_lines(samples).encode()
    assert data.startswith(head) and head.endswith(b"\tFORMAT\tHG00096\tNA12878\ts 3\n")
    body = data[len(head):].split(b"\n")[:-1]
    rows, blob, off = D.site_prefixes("chr21", pos, flag, ref, alt, ids=ids)
    assert rows.tolist() == [0, 2, 3, 4] and len(body) == 4
    for i, ln in enumerate(body):
        prefix = blob[off[i]:off[i + 1]]
        assert ln.startswith(prefix) and len(ln) + 1 - len(prefix) == D.CELL_BYTES * S
        r = rows[i]
        assert prefix == f"chr21\t{pos[r]}\t{ids[r]}\t{ref[r]}\t{alt[r]}\t0.0\tPASS\t.\tGT:HDS:GP:DS\t".encode()
    assert D.line_lengths(off, S).tolist() == [len(ln) + 1 for ln in body]
    # the specification reads back what was written
    c = V().site_columns_host(data)
    assert c.column("id") == [ids[r].encode() for r in rows] and c.ref_len.tolist() == [1, 40, 1, 1]


def test_ids_none_gives_todays_bytes(tmp_path):
    from src import vcf_device as D
    from src.infer_embedding_rag import write_vcf
    pos = np.asarray([3, 9, 27], np.int64)
    samples = ["S0", "S1"]
    h1, h2, gt = _arrays(3, 2)
    write_vcf(tmp_path / "a.vcf", "21", pos, h1, h2, gt, samples)
    write_vcf(tmp_path / "b.vcf", "21", pos, h1, h2, gt, samples, ids=None, ref=None, alt=None)
    write_vcf(tmp_path / "c.vcf", "21", pos, h1, h2, gt, samples, ids=["."] * 3, ref=["."] * 3, alt=["."] * 3)
    a = (tmp_path / "a.vcf").read_bytes()
    assert a == (tmp_path / "b.vcf").read_bytes() == (tmp_path / "c.vcf").read_bytes()
    assert [ln.split(b"\t")[:5] for ln in a.split(b"\n")[-4:-1]] == [[b"21", str(p).encode(), b".", b".", b"."] for p in pos]
    assert D.site_prefixes("21", pos)[1] == D.site_prefixes("21", pos, ids=None)[1] == D.site_prefixes("21", pos, ids=["."] * 3)[1]
    assert D.site_prefixes("21", pos)[1] == b"".join(f"21\t{p}\t.\t.\t.\t0.0\tPASS\t.\tGT:HDS:GP:DS\t".encode() for p in pos)


FILES_ARGS = ["--infer_dataset", "t.vcf", "--infer_panel", "t.panel"]


@pytest.mark.parametrize("extra", [
    ["--vcf_site_columns", "--synthetic", "4"],
    ["--vcf_site_columns", "--synthetic", "4", "--ref_panel", "p.vcf"],
    FILES_ARGS + ["--vcf_site_columns"],
    FILES_ARGS + ["--vcf_site_columns", "--ref_panel", "p.h5"],
])
def test_parse_args_refuses(extra, capsys):
    from src.infer_embedding_rag import parse_args
    with pytest.raises(SystemExit):
        parse_args(extra)
    assert "--vcf_site_columns" in capsys.readouterr().err


def test_parse_args_accepts():
    from src.infer_embedding_rag import parse_args
    assert parse_args(FILES_ARGS).vcf_site_columns is False
    for panel in ("p.vcf", "p.vcf.gz"):
        a = parse_args(FILES_ARGS + ["--vcf_site_columns", "--ref_panel", panel, "--vcf_writer", "device",
                                     "--vcf_bgzf", "--vcf_index"])
        assert a.vcf_site_columns and a.chrom == "21"
    assert parse_args(FILES_ARGS + ["--vcf_site_columns", "--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel"]).ref_panel_pops


def test_entry_points_declared_and_bound():
    from conftest import REPO
    from src import kernels, native
    header = (REPO / "include" / "snvrag.h").read_text()
    for name in ("snvrag_vcf_cols_span", "snvrag_vcf_cols_gather"):
        assert f"int {name}(" in header and name in native.EXPORTED
    assert callable(kernels.vcf_cols_span) and callable(kernels.vcf_cols_gather)
    assert native.ABI_VERSION == 31
