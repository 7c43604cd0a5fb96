"""Tabix indexes on the host (src/dataset/tbi.py, ``write_vcf(bgzf=True, index=True)``), no GPU.

``validate`` is an independent check of an index against its file: it does not use ``tbi.build``,
``tbi.virtual_offsets`` or ``bgzf.bgzf_blocks``.  It walks the gzip members with a plain loop, inflates each
with ``gzip``, derives every line's virtual offsets, restates the bin formula of the specification's C code, and
asserts what a reader of the index relies on: every record lies in exactly one chunk of its own bin, chunks
begin and end on record boundaries, ``ioff[w]`` is the smallest offset of the records overlapping window w, and
the pseudo-bin counts the records.  No htslib, tabix or pysam was available: the specification and this
validator stand in for them."""
import gzip
import os
import struct

import numpy as np
import pytest

from src.dataset import bgzf as B
from src.dataset import tbi as T
from src.dataset.vcf_reader import write_gt_vcf


# ------------------------------------------------------------------------------------------ the validator --
def c_reg2bin(beg, end):
    """``reg2bin`` of the tabix specification, as its C code states it."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def file_records(path):
    """[(chrom, beg, end, v_beg, v_end)] of the bgzipped VCF at ``path`` in file order, and its members
    [(file offset, text bytes)]."""
    raw = open(path, "rb").read()
    members, texts, o = [], [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 12:o + 16] == b"BC\x02\x00", o
        size = struct.unpack_from("<H", raw, o + 16)[0] + 1
        text = gzip.decompress(raw[o:o + size])
        members.append((o, len(text)))
        texts.append(text)
        o += size
    assert o == len(raw) and members[-1][1] == 0, "the file ends with the empty EOF member"
    text = b"".join(texts)

    def voff(t):
        start = 0
        for off, size in members:
            if start <= t < start + size:
                return off << 16 | (t - start)
            start += size
        assert t == len(text)
        return members[-1][0] << 16

    out, t = [], 0
    for line in text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n"):
        e = t + len(line) + 1
        if line and not line.startswith(b"#"):
            col = line.split(b"\t", 4)
            beg = int(col[1]) - 1
            out.append((col[0].decode(), beg, beg + len(col[3]), voff(t), voff(min(e, len(text)))))
        t = e
    return out, members


def validate(path, index):
    recs, members = file_records(path)
    names = list(dict.fromkeys(r[0] for r in recs))
    assert index.names == names
    assert (index.format, index.col_seq, index.col_beg, index.col_end, index.meta, index.skip) == (2, 1, 2, 0, "#", 0)
    for i, name in enumerate(names):
        mine = [r for r in recs if r[0] == name]
        bins, ioff = index.bins[i], index.ioff[i]
        pseudo = bins.get(37450)
        assert pseudo == [(mine[0][3], mine[-1][4]), (len(mine), 0)], (name, pseudo)
        real = {b: c for b, c in bins.items() if b != 37450}
        assert all(0 <= b < 37449 for b in real)
        begs, ends = {r[3] for r in mine}, {r[4] for r in mine}
        for b, chunks in real.items():
            for lo, hi in chunks:
                assert lo < hi and lo in begs and hi in ends, (name, b, lo, hi)
            assert all(c0[1] <= c1[0] for c0, c1 in zip(chunks, chunks[1:])), "chunks of a bin in file order"
        for _, beg, end, v_beg, v_end in mine:
            assert end <= 1 << 29
            cover = [c for c in real.get(c_reg2bin(beg, end), ()) if c[0] <= v_beg and v_end <= c[1]]
            assert len(cover) == 1, (name, beg, end, c_reg2bin(beg, end), cover)
            others = [c for b, cs in real.items() if b != c_reg2bin(beg, end) for c in cs if c[0] <= v_beg < c[1]]
            assert not others, "a record lies in a chunk of a bin that is not its own"
        n_win = max((r[2] - 1) >> 14 for r in mine) + 1
        assert len(ioff) == n_win
        for w in range(n_win):
            over = [r[3] for r in mine if r[1] >> 14 <= w <= (r[2] - 1) >> 14]
            want = min(over) if over else (int(ioff[w - 1]) if w else 0)
            assert int(ioff[w]) == want, (name, w, int(ioff[w]), want)
    for i in range(len(names), len(index.names)):
        assert not index.bins[i] and not len(index.ioff[i])
    return recs, members


# ------------------------------------------------------------------------------------------------ the files --
def vcf_text(seqs, S=3, seed=0, long_ref=()):
    """A VCF text of ``seqs`` [(chrom, positions)]; ``long_ref``: (chrom, pos) records whose REF is 'AT'."""
    import tempfile
    rng = np.random.default_rng(seed)
    parts = []
    with tempfile.TemporaryDirectory() as d:
        for k, (chrom, pos) in enumerate(seqs):
            gt = rng.integers(0, 2, (len(pos), S, 2)).astype(np.int8)
            write_gt_vcf(os.path.join(d, "a.vcf"), [f"S{i}" for i in range(S)], pos, gt, chrom=chrom)
            text = open(os.path.join(d, "a.vcf"), "rb").read()
            parts.append(text if k == 0 else text[text.index(b"\n", text.index(b"#CHROM")) + 1:])
    text = b"".join(parts)
    for chrom, p in long_ref:
        old = f"\n{chrom}\t{p}\t.\tA\t".encode()
        assert text.count(old) == 1
        text = text.replace(old, f"\n{chrom}\t{p}\t.\tAT\t".encode())
    return text


def line_starts(text):
    return [0] + [i + 1 for i in range(len(text) - 1) if text[i] == 10]


GAPPY = [100, 200, 16000, 16384, 16385, 70000, 70001, 200000, 200100, 1 << 20, (1 << 20) + 5, 5000000]


def cases():
    """name -> (text, block_size)"""
    rng = np.random.default_rng(5)
    dense = np.cumsum(rng.integers(1, 300, 900)).tolist()
    one = vcf_text([("chr1", GAPPY)], long_ref=[("chr1", 16384)])
    three = vcf_text([("chr1", dense[:400]), ("chrX", GAPPY), ("7", dense[100:700])], long_ref=[("chrX", 16384)])
    starts = line_starts(three)
    return {"one_sequence": (one, 100),
            "three_sequences": (three, 5000),
            "one_member": (one, 0xff00),
            "record_on_a_member_boundary": (three, starts[40])}           # line 40 begins member 1


CASES = cases()


@pytest.fixture(scope="module", params=sorted(CASES))
def indexed(request, tmp_path_factory):
    text, block = CASES[request.param]
    path = tmp_path_factory.mktemp("tbi") / f"{request.param}.vcf.gz"
    B.write_bgzf(path, text, block_size=block)
    return request.param, path, text, T.index_vcf_bgzf(path)


# ------------------------------------------------------------------------------------------------ the tests --
def test_reg2bin_anchors():
    assert T.reg2bin(0, 1) == 4681 and T.reg2bin(0, 1 << 14) == 4681
    assert T.reg2bin(16383, 16385) == 585 and T.reg2bin(0, 1 << 29) == 0
    assert T.BIN_LIMIT == 1 << 29 and T.reg2bin((1 << 29) - 1, 1 << 29) == 37448
    rng = np.random.default_rng(1)
    for _ in range(300):
        b = int(rng.integers(0, 1 << 29))
        e = min(b + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 29)))), 1 << 29)
        assert T.reg2bin(b, e) == c_reg2bin(b, e)
        assert int(T._bins_of(np.array([b]), np.array([e]))[0]) == c_reg2bin(b, e)


def test_reg2bins_holds_the_bin_of_every_interval_inside():
    rng = np.random.default_rng(2)
    for _ in range(300):
        beg = int(rng.integers(0, (1 << 29) - 1))
        end = min(beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 29)))), 1 << 29)
        bins = T.reg2bins(beg, end)
        assert len(set(bins)) == len(bins) and max(bins) < 37449
        b = int(rng.integers(beg, end))
        e = int(rng.integers(b + 1, end + 1))
        assert c_reg2bin(b, e) in bins and c_reg2bin(beg, end) in bins
        assert c_reg2bin(beg, beg + 1) in bins and c_reg2bin(end - 1, end) in bins


def test_index_of_a_file_passes_the_validator(indexed):
    name, path, text, index = indexed
    recs, members = validate(path, index)
    assert len(recs) == sum(1 for l in text.split(b"\n") if l and not l.startswith(b"#"))
    if name == "one_sequence":
        assert index.names == ["chr1"] and len(members) > 3
        assert 585 in index.bins[0]                                       # REF 'AT' at POS 16384 spans two windows
        assert len(index.ioff[0]) == (5000000 - 1 >> 14) + 1
        assert int(index.ioff[0][3]) == int(index.ioff[0][2]) != 0        # an empty window takes the one before
        assert members[-2][1] < 100                                       # the last member with text is short
    if name == "three_sequences":
        assert index.names == ["chr1", "chrX", "7"] and all(585 not in b for b in (index.bins[0], index.bins[2]))
    if name == "one_member":
        assert len(members) == 2
    if name == "record_on_a_member_boundary":
        on = [r for r in recs if r[3] & 0xffff == 0]
        assert on and all(r[3] >> 16 in {m[0] for m in members[1:]} for r in on)
        full = {off: size for off, size in members if size}
        assert not any(r[4] & 0xffff == full.get(r[4] >> 16, -1) for r in recs)   # never ISIZE in the earlier member
    assert recs[-1][4] == members[-1][0] << 16                            # behind the text: the EOF block


def test_round_trip_and_optional_parts(indexed, tmp_path):
    _, path, _, index = indexed
    index.write(tmp_path / "a.tbi")
    raw = (tmp_path / "a.tbi").read_bytes()
    assert raw[-28:] == B.EOF_BLOCK and gzip.decompress(raw) == index.to_bytes()
    blocks, used = B.bgzf_blocks(raw)
    assert used == len(raw)
    assert T.read(tmp_path / "a.tbi") == index
    data = index.to_bytes()
    assert data[:4] == b"TBI\x01" and struct.unpack_from("<8i", data, 4)[:7] == (len(index.names), 2, 1, 2, 0, 35, 0)
    assert data[-8:] == bytes(8)
    B.write_bgzf(tmp_path / "old.tbi", index.to_bytes(pseudo_bin=False, n_no_coor=False))
    old = T.read(tmp_path / "old.tbi")
    assert old != index and old.ioff[0].tolist() == index.ioff[0].tolist() and old.n_no_coor == 0
    assert [{b: c for b, c in d.items() if b != 37450} for d in index.bins] == old.bins
    recs, _ = file_records(path)
    for name, beg, end, v_beg, v_end in recs[::7]:                        # the same spans with and without the pseudo-bin
        assert T.query(old, name, beg, end) == T.query(index, name, beg, end)


def test_query_spans_hold_the_records_of_the_region(indexed):
    _, path, _, index = indexed
    recs, _ = file_records(path)
    rng = np.random.default_rng(3)
    for name in index.names:
        mine = [r for r in recs if r[0] == name]
        hi = mine[-1][2] + 20000
        regions = [(r[1], r[2]) for r in mine[::5]] + [(0, hi), (mine[0][1], mine[0][1] + 1), (mine[-1][1], hi)]
        regions += [tuple(sorted(rng.integers(0, hi, 2).tolist())) for _ in range(40)]
        for beg, end in regions:
            over = [r for r in mine if r[1] < end and r[2] > beg]
            span = T.query(index, name, beg, end)
            if beg >= end:
                assert span is None
                continue
            if span is None:
                assert not over, (name, beg, end)
                continue
            assert all(span[0] <= r[3] and r[4] <= span[1] for r in over), (name, beg, end, span)
            assert mine[0][3] <= span[0] < span[1] <= mine[-1][4]         # inside this sequence's records
    assert T.query(index, "nowhere", 0, 100) is None
    assert T.query(index, index.names[0], 1 << 28, 1 << 29) is None


def test_read_errors(tmp_path):
    index = T.build(["a"], [0, 0], [5, 9], [6, 10], [100 << 16, 100 << 16 | 50], [100 << 16 | 50, 200 << 16])
    good = index.to_bytes()
    for what, data in (("magic", b"TBJ\x01" + good[4:]), ("format", good[:8] + struct.pack("<i", 1) + good[12:]),
                       ("truncated", good[:-9]), ("truncated", good[:40]), ("truncated", good[:20])):
        B.write_bgzf(tmp_path / "bad.tbi", data)
        with pytest.raises(ValueError, match=f"bad.tbi.*{what}"):
            T.read(tmp_path / "bad.tbi")
    (tmp_path / "plain.tbi").write_bytes(good)
    with pytest.raises(ValueError, match="plain.tbi"):
        T.read(tmp_path / "plain.tbi")


def test_build_errors():
    v = lambda n: (np.arange(n) * 100 + 65536, np.arange(1, n + 1) * 100 + 65536)
    with pytest.raises(ValueError, match=r"record 2 \(a:31\).*not contiguous"):
        T.build(["a", "b"], [0, 1, 0], [10, 20, 30], [11, 21, 31], *v(3))
    with pytest.raises(ValueError, match=r"record 2 \(a:6\).*in front of"):
        T.build(["a", "b"], [0, 0, 0, 1], [10, 20, 5, 1], [11, 21, 6, 2], *v(4))
    with pytest.raises(ValueError, match=r"record 1 \(a:536870912\).*2\^29"):
        T.build(["a"], [0, 0], [10, (1 << 29) - 1], [11, (1 << 29) + 1], *v(2))
    ok = T.build(["a", "b"], [1, 1, 0], [10, 10, 3], [11, 12, 1 << 29], *v(3))   # equal positions; b before a; end = 2^29
    assert ok.bins[0][0] == [(65536 + 200, 65536 + 300)] and list(ok.bins[1]) == [4681, 37450]
    empty = T.build(["a"], [], [], [], [], [])
    assert empty.bins == [{}] and len(empty.ioff[0]) == 0
    with pytest.raises(ValueError, match="record 1.*POS 536870912"):
        T.record_intervals([5, 1 << 29], [1, 1])
    with pytest.raises(ValueError, match="record 0"):
        T.record_intervals([(1 << 29) - 1], [3])


def test_index_vcf_bgzf_names_the_file(tmp_path):
    text = vcf_text([("1", [10, 20]), ("2", [5]), ("1", [30])])
    B.write_bgzf(tmp_path / "split.vcf.gz", text)
    with pytest.raises(ValueError, match="split.vcf.gz.*not contiguous"):
        T.index_vcf_bgzf(tmp_path / "split.vcf.gz")
    (tmp_path / "cut.vcf.gz").write_bytes((tmp_path / "split.vcf.gz").read_bytes()[:-40])
    with pytest.raises(ValueError, match="cut.vcf.gz"):
        T.index_vcf_bgzf(tmp_path / "cut.vcf.gz")


# ------------------------------------------------------------------------------------------ the host writer --
def writer_case(S, n, pos=None, seed=77):
    rng = np.random.default_rng(seed)
    gt = rng.dirichlet(np.ones(4) * 0.3, (n, S)).astype(np.float32)
    sure = rng.random((n, S)) < 0.5
    gt[sure] = np.eye(4, dtype=np.float32)[rng.integers(0, 4, int(sure.sum()))]
    h1, h2 = gt[..., 2] + gt[..., 3], gt[..., 1] + gt[..., 3]
    flag = np.ones(n, bool)
    flag[[2, n - 3]] = False
    pos = np.cumsum(rng.integers(1, 900, n)) + 10_000_000 if pos is None else np.asarray(pos)
    return dict(h1=h1, h2=h2, gt=gt, pos=pos, samples=[f"S{i}" for i in range(S)], flag=flag)


def check_written(path, plain_path):
    """The ``.tbi`` beside ``path`` is the specification's index of that file, and passes the validator."""
    want = T.index_vcf_bgzf(path)
    want.write(str(path) + ".spec")
    tbi = open(str(path) + ".tbi", "rb").read()
    assert gzip.decompress(tbi) == want.to_bytes() and tbi == open(str(path) + ".spec", "rb").read()
    os.remove(str(path) + ".spec")
    recs, members = validate(path, T.read(str(path) + ".tbi"))
    assert open(path, "rb").read() == open(plain_path, "rb").read()        # index=True changes no byte of the file
    return recs, members


@pytest.mark.parametrize("S,n", [(4, 700), (257, 60)])
def test_host_writer_index(tmp_path, S, n):
    from src.infer_embedding_rag import write_vcf
    c = writer_case(S, n)
    ref = ["A"] * n
    ref[5] = "ACGTT"
    args = ("chr1", c["pos"], c["h1"], c["h2"], c["gt"], c["samples"])
    write_vcf(tmp_path / "a.vcf.gz", *args, pos_flag=c["flag"], ref=ref, bgzf=True, index=True)
    write_vcf(tmp_path / "b.vcf.gz", *args, pos_flag=c["flag"], ref=ref, bgzf=True)
    assert sorted(os.listdir(tmp_path)) == ["a.vcf.gz", "a.vcf.gz.tbi", "b.vcf.gz"]
    recs, members = check_written(tmp_path / "a.vcf.gz", tmp_path / "b.vcf.gz")
    assert len(recs) == n - 2 and len(members) > 3
    assert [r[2] - r[1] for r in recs[:6]] == [1, 1, 1, 1, 5, 1]         # row 2 is not written; REF of row 5


def test_host_writer_refusals(tmp_path):
    from src import infer_embedding_rag as I
    c = writer_case(3, 8)
    args = lambda pos: ("1", pos, c["h1"], c["h2"], c["gt"], c["samples"])
    with pytest.raises(ValueError, match="bgzf"):
        I.write_vcf(tmp_path / "a.vcf", *args(c["pos"]), index=True)
    far = c["pos"].copy()
    far[4] = 1 << 29
    with pytest.raises(ValueError, match="record 4: POS 536870912"):
        I.write_vcf(tmp_path / "a.vcf.gz", *args(far), bgzf=True, index=True)
    assert os.listdir(tmp_path) == []                                     # before anything is written
    I.write_vcf(tmp_path / "a.vcf.gz", *args(far), bgzf=True)             # without an index any position goes
    flag = np.zeros(8, bool)
    I.write_vcf(tmp_path / "none.vcf.gz", *args(c["pos"]), pos_flag=flag, bgzf=True, index=True)
    assert T.read(tmp_path / "none.vcf.gz.tbi") == T.index_vcf_bgzf(tmp_path / "none.vcf.gz")
    with pytest.raises(SystemExit):
        I.parse_args(["--vcf_index"])
    a = I.parse_args(["--vcf_index", "--vcf_bgzf", "--truth_region", "imputed"])
    assert a.vcf_index and a.truth_region == "imputed"
    a = I.parse_args([])
    assert not a.vcf_index and a.truth_region == "all"


def test_bgzf_writer_tells_virtual_offsets(tmp_path):
    w = B.BgzfWriter(tmp_path / "a.gz", block_size=10)
    assert w.tell_virtual() == 0
    w.write(b"abcdefg")
    assert w.tell_virtual() == 7
    w.write(b"hij")                                                       # the member is full: the next one, offset 0
    first = len(B.bgzf_member(b"abcdefghij"))
    assert w.tell_virtual() == first << 16
    w.write(b"klm")
    assert w.tell_virtual() == first << 16 | 3
    w.close()
    size = os.path.getsize(tmp_path / "a.gz")
    assert w.tell_virtual() == (size - 28) << 16
