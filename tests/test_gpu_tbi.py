"""GPU tests of the tabix index (``write_vcf_device(bgzf=True, index=True)``, ``read_vcf(region=...)``,
``--vcf_index`` / ``--truth_region``): the device writer's index against the specification ``index_vcf_bgzf`` of
the file it wrote and against the independent validator of test_tbi_cpu.py, at the shapes where a record begins
on a member boundary, straddles members, and where chunks leave short members in the middle of the file; region
reads in both inflate modes against ``parse_vcf_host`` of the filtered text; and the entry point."""
import gzip
import os

import numpy as np
import pytest
import torch

from test_tbi_cpu import check_written, file_records, vcf_text, writer_case

from src.dataset import bgzf as B
from src.dataset import tbi as T
from src.dataset import vcf_reader as V

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


# ---------------------------------------------------------------------------------------- the device writer --
def write_device(tmp_path, c, chrom, expect=True, **kw):
    from src.infer_embedding_rag import write_vcf_device
    up = lambda a: torch.from_numpy(a.copy()).to(DEV)
    for name, index in (("a", True), ("b", False)):
        ok = write_vcf_device(tmp_path / f"{name}.vcf.gz", chrom, c["pos"], up(c["h1"]), up(c["h2"]), up(c["gt"]),
                              c["samples"], pos_flag=c["flag"], device=DEV, bgzf=True, index=index, **kw)
        assert ok is expect
    assert sorted(os.listdir(tmp_path)) == ["a.vcf.gz", "a.vcf.gz.tbi", "b.vcf.gz"]
    return check_written(tmp_path / "a.vcf.gz", tmp_path / "b.vcf.gz")


def test_device_writer_index_record_on_a_member_boundary(tmp_path):
    """S = 4 and a 44-byte prefix (chr1, 8-digit positions): lines of 204 bytes, 320 of them fill a member of
    0xff00 bytes exactly, so every 320th record begins a member."""
    c = writer_case(4, 702)
    recs, members = write_device(tmp_path, c, "chr1")
    assert len(recs) == 700 and [i for i, r in enumerate(recs) if r[3] & 0xffff == 0] == [0, 320, 640]
    assert [size for _, size in members[1:]] == [0xff00, 0xff00, 60 * 204, 0]
    assert recs[319][4] == recs[320][3] == members[2][0] << 16          # offset 0 of the later member, not ISIZE
    assert recs[-1][4] == members[-1][0] << 16                          # the EOF block


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_device_writer_index_straddling_records_and_chunks(tmp_path, n_chunks):
    """S = 257: lines of about 10 KB straddle the members; three chunks leave short members inside the file."""
    from src import vcf_device as D
    c = writer_case(257, 700)
    _, _, p_off = D.site_prefixes("21", c["pos"], c["flag"])
    length = D.line_lengths(p_off, 257)
    kw = {} if n_chunks == 1 else dict(chunk_bytes=int(length.sum()) // 3 + int(length.max()))
    recs, members = write_device(tmp_path, c, "21", **kw)
    assert len(recs) == 698 and len(D.plan_chunks(length, kw.get("chunk_bytes", D.DEFAULT_CHUNK_BYTES))) == n_chunks
    short = [i for i, (_, size) in enumerate(members[1:-1]) if size != 0xff00]
    assert len(short) == n_chunks and (n_chunks == 1 or short[0] < len(members) // 2)
    assert sum(r[3] >> 16 != r[4] >> 16 and r[4] & 0xffff != 0 for r in recs) > 50      # records across two members


@pytest.mark.parametrize("form", ["device", "numpy"])
def test_device_writer_index_fallback(tmp_path, capsys, form):
    from src.infer_embedding_rag import write_vcf, write_vcf_device
    c = writer_case(70, 100)
    c["h1"][50, 40] = 10.0
    conv = (lambda a: torch.from_numpy(a.copy()).to(DEV)) if form == "device" else (lambda a: a)
    args = ("7", c["pos"], conv(c["h1"]), conv(c["h2"]), conv(c["gt"]), c["samples"])
    assert write_vcf_device(tmp_path / "a.vcf.gz", *args, pos_flag=c["flag"], device=DEV, bgzf=True, index=True) is False
    assert "host writer" in capsys.readouterr().out
    write_vcf(tmp_path / "b.vcf.gz", "7", c["pos"], c["h1"], c["h2"], c["gt"], c["samples"], pos_flag=c["flag"], bgzf=True)
    assert sorted(os.listdir(tmp_path)) == ["a.vcf.gz", "a.vcf.gz.tbi", "b.vcf.gz"]
    check_written(tmp_path / "a.vcf.gz", tmp_path / "b.vcf.gz")


def test_device_writer_refusals(tmp_path):
    from src.infer_embedding_rag import write_vcf_device
    c = writer_case(3, 8)
    up = lambda a: torch.from_numpy(a.copy()).to(DEV)
    args = lambda pos: ("1", pos, up(c["h1"]), up(c["h2"]), up(c["gt"]), c["samples"])
    with pytest.raises(ValueError, match="bgzf"):
        write_vcf_device(tmp_path / "a.vcf", *args(c["pos"]), device=DEV, index=True)
    far = c["pos"].copy()
    far[7] = (1 << 29) + 5
    with pytest.raises(ValueError, match="record 7: POS 536870917"):
        write_vcf_device(tmp_path / "a.vcf.gz", *args(far), device=DEV, bgzf=True, index=True)
    assert os.listdir(tmp_path) == []
    none = np.zeros(8, bool)
    assert write_vcf_device(tmp_path / "n.vcf.gz", *args(c["pos"]), pos_flag=none, device=DEV, bgzf=True, index=True)
    assert T.read(tmp_path / "n.vcf.gz.tbi") == T.index_vcf_bgzf(tmp_path / "n.vcf.gz")


# --------------------------------------------------------------------------------------------- region reads --
@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """A three-sequence BGZF file of 2 000 records x 8 samples in members of 4 096 bytes, with missing and
    unphased calls, its index, and its records by sequence."""
    rng = np.random.default_rng(9)
    d = tmp_path_factory.mktemp("region")
    S, parts, names = 8, [], [f"S{i}" for i in range(8)]
    for k, (chrom, n, phased) in enumerate((("chr1", 600, True), ("chr2", 900, False), ("X", 500, True))):
        pos = np.cumsum(rng.integers(2, 300, n)) + 1000
        gt = rng.integers(0, 2, (n, S, 2)).astype(np.int8)
        gt[rng.random((n, S, 2)) < (0.02 if chrom != "X" else 0)] = -1
        V.write_gt_vcf(d / "part.vcf", names, pos, gt, chrom=chrom, phased=phased)
        text = (d / "part.vcf").read_bytes()
        parts.append(text if k == 0 else text[text.index(b"\n", text.index(b"#CHROM")) + 1:])
    text = b"".join(parts)
    path = d / "three.vcf.gz"
    B.write_bgzf(path, text, block_size=4096)
    T.index_vcf_bgzf(path).write(str(path) + ".tbi")
    recs, members = file_records(path)
    return dict(path=path, text=text, recs=recs, members=members, names=names)


def expected(text, name, first, last):
    """``parse_vcf_host`` of the header and the lines of ``name`` with first <= POS <= last."""
    lines = text.split(b"\n")
    keep = [l for l in lines if l.startswith(b"#") or
            (l and l.split(b"\t", 2)[0].decode() == name and first <= int(l.split(b"\t", 2)[1]) <= last)]
    body = [l for l in keep if not l.startswith(b"#")]
    samples, pos, gt = V.parse_vcf_host(b"\n".join(keep) + b"\n")
    return samples, pos, (gt > 0).astype(np.int8) - (gt < 0), not any(b"/" in l for l in body), bool((gt < 0).any())


def regions(t):
    by = lambda name: [r for r in t["recs"] if r[0] == name]
    two, member_of = by("chr2"), lambda r: r[3] >> 16
    pos = lambda r: r[1] + 1
    inside = [r for r in two if member_of(r) == member_of(two[300]) and r[4] >> 16 == member_of(two[300])]
    offs = sorted({member_of(r) for r in two})
    m0 = offs.index(member_of(two[400]))
    four = [r for r in two if offs[m0] <= member_of(r) <= offs[m0 + 3]]
    assert len(inside) > 5 and len({member_of(r) for r in four}) == 4
    return {"single_record": ("chr2", pos(two[123]), pos(two[123])),
            "inside_one_member": ("chr2", pos(inside[1]), pos(inside[-2])),
            "across_four_members": ("chr2", pos(four[0]), pos(four[-1])),
            "bounds_in_gaps": ("chr2", pos(two[200]) + 1, pos(two[260]) - 1),
            "first_record": ("chr2", 1, pos(two[0])),
            "last_record": ("chr2", pos(two[-1]), (1 << 29) - 1),
            "first_of_the_file": ("chr1", 1, pos(by("chr1")[2])),
            "last_of_the_file": ("X", pos(by("X")[-3]), 1 << 29),
            "whole_sequence": ("X", 1, 1 << 29),
            "gap_without_a_record": ("chr2", pos(two[50]) + 1, pos(two[50]) + 1),
            "unknown_name": ("chr9", 1, 1 << 29),
            "empty_span": ("chr2", pos(two[60]), pos(two[60]) - 1),
            "behind_the_last_record": ("chr1", pos(by("chr1")[-1]) + 1, 1 << 29)}


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_region_reads_equal_the_filtered_whole_file(three, inflate):
    n_members, index = len(three["members"]), T.read(str(three["path"]) + ".tbi")
    for what, region in regions(three).items():
        got = V.read_vcf(three["path"], DEV, inflate=inflate, region=region)
        samples, pos, gt, phased, missing = expected(three["text"], *region)
        assert got.samples == samples == three["names"], what
        assert got.n_sites == len(pos) and np.array_equal(got.pos, pos) and got.pos.dtype == np.int32, what
        assert np.array_equal(got.gt(), gt), what
        assert (got.phased, got.any_missing) == (phased, missing), what
        assert got.alt_bits.shape == (16, (len(pos) + 7) // 8) == got.miss_bits.shape, what
        inflated = V.READ_STATS["members_inflated"]
        print(f"{inflate} {what}: {len(pos)} records, {inflated} of {n_members} members inflated")
        assert inflated < n_members, what                                   # the reader's own counter
        span = T.query(index, region[0], region[1] - 1, region[2]) if region[1] <= region[2] else None
        touched = 0 if span is None else sum(span[0] >> 16 <= off and off << 16 < span[1] for off, _ in three["members"])
        assert inflated == 1 + touched, what                                # the header's member and the span's
        if what == "single_record":
            assert touched <= 4, what                                       # one 16 kb window's records: about 6 KB
        if what == "across_four_members":
            assert touched >= 4, what
        if what in ("unknown_name", "empty_span", "behind_the_last_record", "gap_without_a_record"):
            assert len(pos) == 0, what
    assert len(expected(three["text"], *regions(three)["single_record"])[1]) == 1
    whole = V.read_vcf(three["path"], DEV, inflate=inflate)
    assert whole.n_sites == 2000 and not whole.phased and whole.any_missing
    if inflate == "device":
        assert V.READ_STATS["members_inflated"] >= n_members - 1            # every member with text


@pytest.mark.parametrize("small_span", [V.SMALL_SPAN, 0])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_region_read_chunked(three, monkeypatch, inflate, small_span):
    """Spans longer than ``chunk_bytes`` (one member of 4 096 bytes per chunk): the prefix is dropped in the first
    chunk and the suffix in the last, and the span's end is applied to its last member in whichever chunk that
    member falls.  chr1 and chr2 share a member and overlap in POS, so text left behind the end of chr1's span
    would come back as chr1's records; the whole of chr1, the tail of chr2 and the whole of X have their last
    record in the span's last member.  ``small_span`` 0: the raw bytes are streamed from the file itself, as for
    a span above ``SMALL_SPAN``; with it and a ``chunk_bytes`` of 1 MiB the span is one chunk of that path."""
    monkeypatch.setattr(V, "SMALL_SPAN", small_span)
    recs = three["recs"]
    one, two = [r for r in recs if r[0] == "chr1"], [r for r in recs if r[0] == "chr2"]
    assert one[-1][4] >> 16 == two[0][3] >> 16 and one[-1][4] & 0xffff                 # one member holds both
    assert two[0][1] < one[-1][1] and one[0][1] < two[-1][1]                           # and the positions overlap
    cases = dict(regions(three), whole_chr1=("chr1", 1, 1 << 29), tail_of_chr2=("chr2", two[-200][1] + 1, two[-1][1] + 1),
                 chr1_to_its_last=("chr1", one[300][1] + 1, one[-1][1] + 1))
    for what in ("across_four_members", "whole_chr1", "tail_of_chr2", "chr1_to_its_last", "whole_sequence", "single_record"):
        want = expected(three["text"], *cases[what])
        for chunk_bytes in (5000, 1 << 20) if small_span == 0 else (5000,):
            got = V.read_vcf(three["path"], DEV, chunk_bytes=chunk_bytes, inflate=inflate, region=cases[what])
            assert got.n_sites == len(want[1]) and np.array_equal(got.pos, want[1]), (what, chunk_bytes)
            assert np.array_equal(got.gt(), want[2]) and (got.phased, got.any_missing) == want[3:], (what, chunk_bytes)
    assert len(expected(three["text"], *cases["whole_chr1"])[1]) == 600


def test_region_read_refusals_and_error_text(three, tmp_path):
    text = three["text"]
    (tmp_path / "plain.vcf").write_bytes(text)
    with gzip.open(tmp_path / "one.vcf.gz", "wb") as f:
        f.write(text)
    B.write_bgzf(tmp_path / "noindex.vcf.gz", text)
    for name, match in (("plain.vcf", "BGZF"), ("one.vcf.gz", "BGZF"), ("noindex.vcf.gz", r"noindex.vcf.gz.tbi")):
        with pytest.raises(ValueError, match=match):
            V.read_vcf(tmp_path / name, DEV, region=("chr1", 1, 5000))
    # a malformed record inside the region: POS and the virtual offset, since the file line is not known
    two = [r for r in three["recs"] if r[0] == "chr2"]
    p = two[500][1] + 1
    old = next(l for l in text.split(b"\n") if l.startswith(f"chr2\t{p}\t".encode()))
    bad = text.replace(old, old[:-3] + b"0/1/1"[:3] + b"/1")
    assert bad != text
    B.write_bgzf(tmp_path / "bad.vcf.gz", bad, block_size=4096)
    T.index_vcf_bgzf(tmp_path / "bad.vcf.gz").write(str(tmp_path / "bad.vcf.gz.tbi"))
    v = next(r[3] for r in file_records(tmp_path / "bad.vcf.gz")[0] if r[0] == "chr2" and r[1] + 1 == p)
    for inflate in ("host", "device"):
        with pytest.raises(ValueError, match=f"bad.vcf.gz: record at POS {p} \\(virtual offset {v}: .*more than two alleles"):
            V.read_vcf(tmp_path / "bad.vcf.gz", DEV, inflate=inflate, region=("chr2", two[480][1], two[520][1]))
        got = V.read_vcf(tmp_path / "bad.vcf.gz", DEV, inflate=inflate, region=("chr2", 1, p - 1))   # not in the region
        assert got.n_sites == 500


# ------------------------------------------------------------------------------------------ the entry point --
def test_infer_cli_truth_region_and_vcf_index(tmp_path):
    """``--truth_region imputed`` reads the truth file through its index over the span of the imputed positions
    and scores the same: accuracy.tsv byte for byte, every array of quality.npz equal.  ``truth_row`` holds record
    numbers of what was read, so it is compared after adding the number of truth records in front of the span,
    which a region read cannot know without the full scan it avoids.  The truth file holds more of chromosome 21
    than the imputed sites span, and a second sequence."""
    from src import infer_embedding_rag as I
    from src.dataset.synthetic import make_infer_arrays
    n_sites, S = 2040, 6
    a = make_infer_arrays(n_sites, S, 24, missing_rate=0.5, seed=11)
    rng = np.random.default_rng(4)
    beyond = int(a["ori_pos"].max()) + np.cumsum(rng.integers(1, 400, 4000))
    other = np.cumsum(rng.integers(1, 200, 2000))
    text = vcf_text([("21", a["ori_pos"].tolist() + beyond.tolist()), ("22", other.tolist())], S=S)
    lines = text.split(b"\n")                                              # the true genotypes at the panel's sites
    V.write_gt_vcf(tmp_path / "t.vcf", [f"S{i}" for i in range(S)], a["ori_pos"], a["truth"], chrom="21")
    true = (tmp_path / "t.vcf").read_bytes().split(b"\n")
    lines[2:2 + n_sites] = true[2:2 + n_sites]
    truth = tmp_path / "truth.vcf.gz"
    B.write_bgzf(truth, b"\n".join(lines), block_size=8192)
    T.index_vcf_bgzf(truth).write(str(truth) + ".tbi")
    args = ["--synthetic", str(S), "--synthetic_sites", str(n_sites), "--synthetic_ref", "24", "-d", "64", "-l", "2",
            "-a", "2", "-b", "4", "--k_retrieve", "3", "--mask_rate", "0.5", "--index_window_len", "1020",
            "--truth_vcf", str(truth), "--vcf_inflate", "device"]
    try:
        I.infer(args + ["--no_vcf", "-o", str(tmp_path / "all")])
        whole = V.READ_STATS["members_inflated"]
        I.infer(args + ["--truth_region", "imputed", "--vcf_bgzf", "--vcf_index", "--vcf_writer", "device",
                        "-o", str(tmp_path / "imputed")])
        part = V.READ_STATS["members_inflated"]
    finally:
        V.set_default_inflate("host")                                       # the entry point's --vcf_inflate is process-wide
    assert part < whole / 2                                                 # a quarter of the records lie in the span
    assert (tmp_path / "all" / "accuracy.tsv").read_bytes() == (tmp_path / "imputed" / "accuracy.tsv").read_bytes()
    q, r = np.load(tmp_path / "all" / "quality.npz"), np.load(tmp_path / "imputed" / "quality.npz")
    assert q.files == r.files and int(q["flag"].sum()) > 500 and (q["acc_n"][q["flag"]] == S).all()
    for k in q.files:
        if k != "truth_row":
            assert np.array_equal(q[k], r[k], equal_nan=True), k
    in_front = int(np.argmax(q["flag"]))                                    # truth records in front of the first imputed site
    assert np.array_equal(q["truth_row"] >= 0, q["flag"])
    assert np.array_equal(np.where(r["truth_row"] >= 0, r["truth_row"] + in_front, -1), q["truth_row"])
    assert sorted(os.listdir(tmp_path / "imputed")) == ["accuracy.tsv", "imputed.npz", "imputed.vcf.gz",
                                                        "imputed.vcf.gz.tbi", "quality.npz"]
    vcf = tmp_path / "imputed" / "imputed.vcf.gz"
    assert gzip.decompress((tmp_path / "imputed" / "imputed.vcf.gz.tbi").read_bytes()) == T.index_vcf_bgzf(vcf).to_bytes()
    got = V.read_vcf(vcf, DEV, region=("21", int(a["ori_pos"][q["flag"]][10]), int(a["ori_pos"][q["flag"]][20])))
    assert np.array_equal(got.pos, a["ori_pos"][q["flag"]][10:21])
