"""GPU tests of the site columns (CHROM, ID, REF, ALT) of the device VCF reader: the two kernels of
csrc/vcfread.hip (snvrag_vcf_cols_span, snvrag_vcf_cols_gather) per byte against the specification
(src/dataset/vcf_reader.py record_columns / site_columns_host), ``read_vcf(columns=True)`` over every source of
the text, and ``infer_embedding_rag --vcf_site_columns`` end to end.  Offsets, lengths and bytes are compared
exactly; every array a kernel writes lies between 64 guard bytes of 0xA5 that must come back untouched."""

import gzip
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from src import kernels as K  # noqa: E402
from src.dataset import bgzf as B  # noqa: E402
from src.dataset import tbi as T  # noqa: E402
from src.dataset import vcf_reader as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL = 64, 0xA5
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 129, 300)
ALPHABET = np.frombuffer(b"ACGTNacgtn.,<>:;=_*0123456789", np.uint8)


def word(rng, n) -> bytes:
    return ALPHABET[rng.integers(0, ALPHABET.size, n)].tobytes()


def record(chrom=b"chr21", pos=1, id_=b"rs1", ref=b"A", alt=b"C", cells=(b"0|1", b"1|0", b"0|0")) -> bytes:
    return b"\t".join([chrom, str(pos).encode(), id_, ref, alt, b".", b"PASS", b".", b"GT", *cells])


# ------------------------------------------------------------------------------------------------ the kernels --
def want_spans(text: bytes, starts):
    """The specification of snvrag_vcf_cols_span on a chunk: (start, length) of columns 1, 3, 4, 5 per line, and
    the strings themselves as ``record_columns`` gives them."""
    out, strings = np.zeros((len(starts), 8), np.int32), []
    for i, lo in enumerate(starts):
        nl = text.find(b"\n", lo)
        nl = len(text) if nl < 0 else nl
        end = nl - 1 if nl > lo and text[nl - 1] == 13 else nl
        tabs = [lo + j for j, c in enumerate(text[lo:end]) if c == 9]
        edge = lambda k: tabs[k] if len(tabs) > k else end              # tab k (0-based), or the line end
        cols = [(lo, edge(0))] + [(edge(k) + 1, edge(k + 1)) if len(tabs) > k else (end, end) for k in (1, 2, 3)]
        out[i] = [v for a, b in cols for v in (a, b - a)]
        strings.append(V.record_columns(text[lo:nl]))
        assert tuple(text[a:b] for a, b in cols) == strings[-1]
    return out, strings


def guarded(nbytes: int):
    """(the whole buffer, its middle ``nbytes``), the middle 64-byte aligned between two guards."""
    whole = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole, nbytes):
    g = whole.cpu().numpy()
    return (g[:GUARD] == FILL).all() and (g[GUARD + nbytes:] == FILL).all()


def check_chunk(lines, sep=b"\n", final_newline=True):
    """Both kernels on the chunk made of ``lines`` (empty ones are legal and vanish) against the specification."""
    text = sep.join(lines) + (sep if final_newline else b"")
    starts, at = [], 0
    for ln in lines:
        if ln not in (b"", b"\r"):
            starts.append(at)
        at += len(ln) + len(sep)
    nbytes, n = len(text), len(starts)
    buf = np.full((nbytes + 15) // 16 * 16, 10, np.uint8)
    buf[:nbytes] = np.frombuffer(text, np.uint8)
    dev_text = torch.from_numpy(buf).to(DEV)
    line_off, n_lines = K.vcf_line_index(dev_text, nbytes, n + 1)
    assert int(n_lines.item()) == n and line_off[:n].cpu().tolist() == starts
    want, cols = want_spans(text, starts)

    whole_s, mid = guarded(32 * n)
    spans = K.vcf_cols_span(dev_text, nbytes, line_off, n, out=mid.view(torch.int32).view(n, 8))
    np.testing.assert_array_equal(spans.cpu().numpy(), want)
    assert guards_intact(whole_s, 32 * n)

    lens = want[:, 1::2].T.reshape(-1).astype(np.int64)                 # item c n + r
    off = np.zeros(4 * n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    whole_b, blob = guarded(max(total, 1))
    K.vcf_cols_gather(dev_text, nbytes, spans, torch.from_numpy(off).to(DEV), blob)
    packed = b"".join(cols[r][c] for c in range(4) for r in range(n))
    assert len(packed) == total
    assert blob.cpu().numpy().tobytes() == (packed if total else bytes([FILL]))
    assert guards_intact(whole_b, max(total, 1))
    return spans, want


@pytest.mark.parametrize("col", range(4))
def test_column_lengths(col):
    rng = np.random.default_rng(col)
    lines = []
    for i, n in enumerate(LENGTHS):
        f = [b"chr21", b"rs%d" % i, b"A", b"C"]
        f[col] = word(rng, n)
        lines.append(record(f[0], 100 + i, *f[1:]))
    spans, want = check_chunk(lines)
    assert want[:, 2 * col + 1].tolist() == list(LENGTHS)


def test_tab_positions_at_the_walk_step_edges():
    """The first, third, fourth and fifth tab on byte 63 and on byte 64 of a 64-byte walk step, and a record
    whose fifth tab lies in the third step."""
    lines, seen = [], set()
    for tab in (1, 3, 4, 5):
        for at in (63, 64):
            base = record(b"", 7, b"rs9", b"ACG", b"T,G")
            have = [j for j, c in enumerate(base) if c == 9][tab - 1]
            ln = record(b"c" * (at - have), 7, b"rs9", b"ACG", b"T,G")
            assert [j for j, c in enumerate(ln) if c == 9][tab - 1] == at
            lines.append(ln)
            seen.add((tab, at))
    far = record(b"c" * 70, 12345, b"i" * 40, b"G" * 30, b"T")
    assert 128 <= [j for j, c in enumerate(far) if c == 9][4] < 192
    assert len(seen) == 8
    check_chunk(lines + [far])
    check_chunk(lines + [far], sep=b"\r\n")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_record_counts(n):
    rng = np.random.default_rng(n)
    pick = lambda: int(rng.choice(LENGTHS)) if rng.random() < 0.2 else int(rng.integers(0, 12))
    lines = [record(word(rng, pick()), 10 + i, word(rng, pick()), word(rng, pick()), word(rng, pick()))
             for i in range(n)]
    lines.insert(n // 2, b"")                                            # a blank line vanishes
    check_chunk(lines)


@pytest.mark.parametrize("sep", [b"\n", b"\r\n"])
def test_short_lines(sep):
    """Fewer than five tabs: the columns reached are exact (the last one ends at the line end, in front of a
    '\\r'), the rest have length 0.  Straight through the entry points: parse_gt would refuse these lines."""
    lines = [b"chr1\t5\trs7\tACGT", b"chr1\t5\trs7", b"chr1\t5", b"chr1", b"chr1\t5\trs7\tAC\tT", b"\t\t\t", b"x\t\t\t\t",
             record(b"chrX", 9, b".", b"A" * 70, b"T")]
    spans, want = check_chunk(lines, sep=sep)
    assert want[0, 1::2].tolist() == [4, 3, 4, 0] and want[1, 1::2].tolist() == [4, 3, 0, 0]
    assert want[2, 1::2].tolist() == [4, 0, 0, 0] and want[3, 1::2].tolist() == [4, 0, 0, 0]
    assert want[4, 1::2].tolist() == [4, 3, 2, 1] and want[5, 1::2].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("rem", [0, 1, 15])
@pytest.mark.parametrize("final_newline", [True, False])
def test_chunk_end(rem, final_newline):
    """nbytes % 16 in {0, 1, 15}; the last line ends with the chunk's last byte, as its '\\n' or without one
    (the kernels then read the '\\n' of the padding, or of the guard behind nbytes when there is no padding)."""
    first = record(b"chr2", 1, b"a", b"C", b"G")
    last = b"chr2\t2\tb\tG\tTTTT"                                       # a short last line: ALT runs to the chunk end
    have = len(first) + 1 + len(last) + (1 if final_newline else 0)
    last += b"A" * ((rem - have) % 16)
    nbytes = len(first) + 1 + len(last) + (1 if final_newline else 0)
    assert nbytes % 16 == rem
    spans, want = check_chunk([first, last], final_newline=final_newline)
    assert want[1, 6] + want[1, 7] == nbytes - (1 if final_newline else 0)


def test_refused_calls():
    from src import native
    lib = native.load()
    buf = torch.full((8 * 256,), FILL, dtype=torch.uint8, device=DEV)
    ref = buf.clone()
    at = lambda i, shift=0: buf[256 * i + shift:].data_ptr()
    good = dict(text=at(0), nbytes=16, index=at(1), n=1, spans=at(2), blob=at(3))

    def span(**kw):
        a = dict(good, **kw)
        return lib.snvrag_vcf_cols_span(a["text"], a["nbytes"], a["index"], a["n"], a["spans"], None), \
            lib.snvrag_last_error().decode()

    def gather(**kw):
        a = dict(good, **kw)
        return lib.snvrag_vcf_cols_gather(a["text"], a["nbytes"], a["spans"], a["n"], a["index"], a["blob"], 16, None), \
            lib.snvrag_last_error().decode()

    for call, name, ptrs in ((span, "snvrag_vcf_cols_span", ("text", "index", "spans")),
                             (gather, "snvrag_vcf_cols_gather", ("text", "index", "spans", "blob"))):
        for p in ptrs:
            rc, text = call(n=0, **{p: None})
            assert rc != 0 and text == f"{name}: null pointer"
        rc, text = call(n=0, text=at(0, 2))
        assert rc != 0 and text == f"{name}: text must be 16-byte aligned, the offsets 8-byte aligned, spans 4-byte aligned"
        assert call(n=0, spans=at(2, 2))[0] != 0 and call(n=0, index=at(1, 4))[0] != 0
        rc, text = call(n=0, nbytes=0)
        assert rc != 0 and text == f"{name}: nbytes must be in [1, 2^31)"
        assert call(n=0, nbytes=1 << 31)[0] != 0
        rc, text = call(n=17)
        assert rc != 0 and text == f"{name}: n_lines must be in [0, nbytes]"
        assert call(n=-1)[0] != 0
        assert call(n=0)[0] == 0                                         # nothing to do: no launch
    torch.cuda.synchronize()
    assert torch.equal(buf, ref), "a refused call wrote to a buffer it was passed"


# ------------------------------------------------------------------------------------------------ the reader --
SAMPLES = ["NA1", "NA2", "NA3"]


def body_lines(rng, n, lengths, chrom=None, crlf_every=0):
    """``n`` records of 3 samples; one column of each record takes a length of the mix, in turn, the others
    0 .. 10 bytes (``chrom``: one fixed CHROM), blank lines between some of them, POS ascending."""
    lines, pos = [], 1000
    cells = [b"0|1", b"1|0", b"0|0", b"1|1", b".|.", b"0/1", b"0|1:12"]
    for i in range(n):
        f = [word(rng, int(rng.integers(0, 11))) for _ in range(4)]
        f[i % 4] = word(rng, int(lengths[(i // 4) % len(lengths)]))
        pos += int(rng.integers(1, 200))
        ln = record(f[0] if chrom is None else chrom, pos, f[1], f[2], f[3],
                    [cells[int(rng.integers(0, len(cells)))] for _ in SAMPLES])
        lines.append(ln + (b"\r" if crlf_every and i % crlf_every == 0 else b""))
        if i % 37 == 5:
            lines.append(b"")
    return lines


def vcf_bytes(lines) -> bytes:
    head = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(SAMPLES).encode()
    return head + b"\n" + b"\n".join(lines) + b"\n"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (paths by form, the specification's columns): "full" holds the whole length mix, "fit" the mix
    without the 300-byte strings, so that every line, and a line's tail with a BGZF block behind it, fits a 256-byte chunk."""
    d = tmp_path_factory.mktemp("cols")
    out = {}
    for name, lengths, block in (("full", LENGTHS, 1500), ("fit", [n for n in LENGTHS if n <= 129], 40)):
        lines = body_lines(np.random.default_rng(len(lengths)), 300, lengths, crlf_every=11)
        assert name == "full" or max(len(ln) for ln in lines) + 1 + block <= 256
        data = vcf_bytes(lines)
        paths = dict(text=d / f"{name}.vcf", gz=d / f"{name}.plain.vcf.gz", bgzf=d / f"{name}.vcf.gz")
        paths["text"].write_bytes(data)
        with gzip.open(paths["gz"], "wb") as f:
            f.write(data)
        B.write_bgzf(paths["bgzf"], data, block_size=block)
        want = V.site_columns_host(data)
        assert len(want) == 300 and V.site_columns_host(paths["gz"]).column("alt") == want.column("alt")
        out[name] = (paths, want)
    assert max(out["full"][1].lengths("id").max(), out["full"][1].ref_len.max()) == 300
    return out


def same_columns(got, want):
    assert len(got) == len(want)
    for name in V.COLUMN_NAMES:
        off, blob = getattr(got, name + "_off"), getattr(got, name + "_blob")
        assert off.dtype == np.int64 and blob.dtype == np.uint8
        np.testing.assert_array_equal(off, getattr(want, name + "_off"), err_msg=name)
        assert blob.tobytes() == getattr(want, name + "_blob").tobytes(), name


@pytest.mark.parametrize("force_general", [False, True])
@pytest.mark.parametrize("form,inflate", [("text", None), ("gz", "host"), ("bgzf", "host"), ("bgzf", "device")])
@pytest.mark.parametrize("chunk_bytes", [256, 4096, None])
def test_read_vcf_columns_equal_the_specification(files, chunk_bytes, form, inflate, force_general):
    """chunk_bytes 256 reads the file whose lines fit such a chunk (a 300-byte string does not); 4096 and the
    default read the whole mix.  Records straddle chunks, and at 256 every chunk carries code rows."""
    paths, want = files["fit" if chunk_bytes == 256 else "full"]
    kw = dict(force_general=force_general, inflate=inflate, **({} if chunk_bytes is None else {"chunk_bytes": chunk_bytes}))
    got = V.read_vcf(paths[form], DEV, columns=True, **kw)
    same_columns(got.columns, want)
    assert got.columns.ref(7) == want.column("ref")[7] and got.columns.ref_len.tolist() == [len(t) for t in want.column("ref")]
    plain = V.read_vcf(paths[form], DEV, **kw)
    assert plain.columns is None and plain.n_sites == got.n_sites == 300 and plain.samples == got.samples == SAMPLES
    assert torch.equal(plain.alt_bits, got.alt_bits) and torch.equal(plain.miss_bits, got.miss_bits)
    np.testing.assert_array_equal(plain.pos, got.pos)
    assert (plain.any_missing, plain.phased) == (got.any_missing, got.phased)


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_region_read_keeps_the_kept_records_columns(tmp_path, monkeypatch, inflate):
    """A region in the middle of one sequence: the span tabix gives begins in front of it and ends behind it, so
    the span kernel sees more lines than are kept, and only the kept records' strings are gathered."""
    data = vcf_bytes(body_lines(np.random.default_rng(5), 300, LENGTHS, chrom=b"chr7"))
    path = tmp_path / "r.vcf.gz"
    B.write_bgzf(path, data, block_size=1500)
    T.index_vcf_bgzf(path).write(str(path) + ".tbi")
    _, pos, _ = V.parse_vcf_host(data)
    first, last = int(pos[100]), int(pos[180])
    want = V.site_columns_host(data)
    seen = []
    real = K.vcf_cols_span
    monkeypatch.setattr(K, "vcf_cols_span", lambda text, nbytes, line_off, n, out=None:
                        (seen.append(n), real(text, nbytes, line_off, n, out))[1])
    got = V.read_vcf(path, DEV, inflate=inflate, region=("chr7", first, last), columns=True)
    plain = V.read_vcf(path, DEV, inflate=inflate, region=("chr7", first, last))
    assert got.n_sites == plain.n_sites == 81 and sum(seen) > 81
    np.testing.assert_array_equal(got.pos, pos[100:181])
    np.testing.assert_array_equal(got.pos, plain.pos)
    assert torch.equal(got.alt_bits, plain.alt_bits) and plain.columns is None
    for name in V.COLUMN_NAMES:
        assert got.columns.column(name) == want.column(name)[100:181], name
    none = V.read_vcf(path, DEV, inflate=inflate, region=("chr8", 1, 10), columns=True)
    assert none.n_sites == 0 and len(none.columns) == 0 and none.columns.ref_len.size == 0


# ------------------------------------------------------------------------------------------------ end to end --
def write_cols_vcf(path, samples, chrom, pos, ids, ref, alt, gt):
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
                "\t".join(samples).encode() + b"\n")
        for i in range(len(pos)):
            c = chrom[i] if isinstance(chrom, (list, tuple)) else chrom
            cells = [f"{a if a >= 0 else '.'}|{b if b >= 0 else '.'}".encode() for a, b in gt[i].tolist()]
            f.write(record(c.encode(), int(pos[i]), ids[i].encode(), ref[i].encode(), alt[i].encode(), cells) + b"\n")


def write_panel_file(path, names, pops):
    with open(path, "w") as f:
        f.write("sample\tpop\tsuper_pop\tgender\n")
        for s, p in zip(names, pops):
            f.write(f"{s}\tX\t{p}\tmale\n")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """target.vcf, panel.vcf and their .panel files, nothing else (``--ref_panel_pops``): 1300 panel sites, 6
    target samples named HG0..., a panel on "chr21" with IDs, multi-base and multi-allelic alleles and a 40-base
    REF at an imputed site."""
    from src.dataset.synthetic import POPS, make_infer_arrays
    d = tmp_path_factory.mktemp("e2e")
    a = make_infer_arrays(1300, 6, 24, missing_rate=0.3, ref_missing=0, seed=11)
    rng = np.random.default_rng(3)
    names, refs = [f"HG0{i}" for i in range(6)], [f"R{i}" for i in range(24)]
    n = len(a["ref_pos"])
    imputed = np.flatnonzero(~np.isin(a["ref_pos"], a["pos"]))
    ids = [f"rs{int(rng.integers(1, 10 ** 9))}" if i % 3 else "." for i in range(n)]
    ref = [word(rng, 1 + (i % 7 == 0) * int(rng.integers(1, 5))).decode() for i in range(n)]
    alt = [word(rng, 1).decode() + (",T" if i % 11 == 0 else "") for i in range(n)]
    ref[int(imputed[3])] = "ACGT" * 10
    V.write_gt_vcf(d / "target.vcf", names, a["pos"], a["vcf"])
    write_cols_vcf(d / "panel.vcf", refs, "chr21", a["ref_pos"], ids, ref, alt, a["ref_gt"])
    write_panel_file(d / "target.panel", names, a["pops"])
    write_panel_file(d / "panel.panel", refs, [POPS[(3 * i) % 5] for i in range(24)])
    common = ["--infer_dataset", str(d / "target.vcf"), "--infer_panel", str(d / "target.panel"),
              "--ref_panel", str(d / "panel.vcf"), "--ref_panel_pops", str(d / "panel.panel"),
              "-d", "64", "-l", "2", "-a", "2", "-b", "4", "--k_retrieve", "3", "--dtype", "f32"]
    return dict(dir=d, a=a, names=names, ids=ids, ref=ref, alt=alt, imputed=imputed, common=common)


def body_records(data: bytes):
    lines = data.split(b"\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith(b"#CHROM")][0]
    return lines[at], [ln.split(b"\t") for ln in lines[at + 1:] if ln]


def test_infer_without_the_flag_writes_the_same_bytes(inputs, tmp_path):
    from src import infer_embedding_rag as I
    res = I.infer(inputs["common"] + ["-o", str(tmp_path / "plain")])
    got = (tmp_path / "plain" / "imputed.vcf").read_bytes()
    pos = np.load(tmp_path / "plain" / "imputed.npz")["pos"]
    flag = res["mask"][:, 0].astype(bool)
    I.write_vcf(tmp_path / "want.vcf", "21", pos, res["h1"], res["h2"], res["gt"], [f"S{i}" for i in range(6)],
                pos_flag=flag, ids=None, ref=None, alt=None)
    assert got == (tmp_path / "want.vcf").read_bytes()
    head, recs = body_records(got)
    assert head.split(b"\t")[9:] == [b"S%d" % i for i in range(6)] and len(recs) == int(flag.sum()) > 100
    assert {tuple(r[0:1] + r[2:5]) for r in recs} == {(b"21", b".", b".", b".")}


def test_infer_with_the_flag_carries_the_panels_columns(inputs, tmp_path, capsys):
    from src import infer_embedding_rag as I
    args = inputs["common"] + ["--vcf_site_columns"]
    I.infer(args + ["-o", str(tmp_path / "host")])
    assert "CHROM is the panel's 'chr21', not --chrom '21'" in capsys.readouterr().out
    got = (tmp_path / "host" / "imputed.vcf").read_bytes()
    head, recs = body_records(got)
    assert [c.decode() for c in head.split(b"\t")[9:]] == inputs["names"]
    # the panel file's first record at each POS, through the specification
    _, ppos, _ = V.parse_vcf_host(inputs["dir"] / "panel.vcf")
    pc = V.site_columns_host(inputs["dir"] / "panel.vcf")
    first = {}
    for i, p in enumerate(ppos.tolist()):
        first.setdefault(p, i)
    assert len(first) == len(ppos)
    z = np.load(tmp_path / "host" / "imputed.npz")
    want_pos = z["pos"][z["mask"][:, 0].astype(bool)]                     # the imputed sites: what the writers select
    assert [int(r[1]) for r in recs] == want_pos.tolist() and len(recs) > 100
    for r in recs:
        i = first[int(r[1])]
        assert (r[0], r[2], r[3], r[4]) == (pc.chrom(i), pc.id(i), pc.ref(i), pc.alt(i)), r[:5]
    assert any(len(r[3]) == 40 for r in recs) and any(b"," in r[4] for r in recs)

    I.infer(args + ["--vcf_writer", "device", "-o", str(tmp_path / "device")])
    assert (tmp_path / "device" / "imputed.vcf").read_bytes() == got

    for writer in ("host", "device"):
        out = tmp_path / f"gz_{writer}"
        I.infer(args + ["--vcf_writer", writer, "--vcf_bgzf", "--vcf_index", "-o", str(out)])
        vcf = out / "imputed.vcf.gz"
        assert gzip.decompress(vcf.read_bytes()) == got
        index = T.index_vcf_bgzf(vcf)                                     # the slow host indexer: ends from len(REF)
        assert gzip.decompress((out / "imputed.vcf.gz.tbi").read_bytes()) == index.to_bytes()
        assert index.names == ["chr21"]
    long_pos = int([r[1] for r in recs if len(r[3]) == 40][0])
    hit = V.read_vcf(tmp_path / "gz_device" / "imputed.vcf.gz", DEV, region=("chr21", long_pos, long_pos), columns=True)
    assert hit.n_sites == 1 and hit.columns.ref(0) == b"ACGT" * 10


def test_a_panel_with_two_sequences_is_refused(inputs, tmp_path):
    from src import infer_embedding_rag as I
    a = inputs["a"]
    chrom = ["chr21"] * len(a["ref_pos"])
    chrom[int(inputs["imputed"][-1])] = "chr22"
    write_cols_vcf(tmp_path / "two.vcf", [f"R{i}" for i in range(24)], chrom, a["ref_pos"], inputs["ids"],
                   inputs["ref"], inputs["alt"], a["ref_gt"])
    args = list(inputs["common"])
    args[args.index("--ref_panel") + 1] = str(tmp_path / "two.vcf")
    ds, _ = I.build_dataset(I.parse_args(args + ["--vcf_site_columns"]))
    with pytest.raises(ValueError, match="'chr21' and 'chr22'"):
        I.panel_site_columns(ds, "21")


def test_first_record_at_a_position_absent_sites_and_bytes_that_do_not_decode(tmp_path):
    """``panel_site_columns`` on a small panel: a position held twice gives its first record's strings, a site
    the panel does not hold stays '.', and a record whose bytes do not decode raises with its POS."""
    import types
    from src import infer_embedding_rag as I
    lines = [record(b"chr3", 10, b"a", b"A", b"C"), record(b"chr3", 20, b"first", b"AC", b"G"),
             record(b"chr3", 20, b"second", b"T", b"TT"), record(b"chr3", 40, b"bad\xff", b"G", b"A")]
    (tmp_path / "p.vcf").write_bytes(vcf_bytes(lines))
    vg = V.read_vcf(tmp_path / "p.vcf", DEV, columns=True)
    got = I.panel_site_columns(types.SimpleNamespace(ref_panel_vcf=vg, ori_pos=np.array([10, 20, 30])), "21")
    assert (got["chrom"], got["ids"], got["ref"], got["alt"]) == ("chr3", ["a", "first", "."], ["A", "AC", "."], ["C", "G", "."])
    assert got["rows"].tolist() == [0, 1, -1]
    none = I.panel_site_columns(types.SimpleNamespace(ref_panel_vcf=vg, ori_pos=np.array([5])), "21")
    assert (none["chrom"], none["ids"]) == ("21", ["."])
    import locale
    if locale.getpreferredencoding(False).lower().replace("-", "") in ("utf8", "ascii", "ansi_x3.41968"):
        with pytest.raises(ValueError, match="POS 40"):
            I.panel_site_columns(types.SimpleNamespace(ref_panel_vcf=vg, ori_pos=np.array([10, 40])), "21")


def test_a_truth_record_with_other_alleles_is_not_scored(inputs, tmp_path, capsys):
    from src import infer_embedding_rag as I
    a, imputed = inputs["a"], inputs["imputed"]
    n = len(a["ref_pos"])
    truth_gt = np.asarray(a["truth"])
    names = inputs["names"]
    write_cols_vcf(tmp_path / "truth.vcf", names, "chr21", a["ref_pos"], inputs["ids"], inputs["ref"], inputs["alt"], truth_gt)
    changed = int(imputed[40])
    alt = list(inputs["alt"])
    alt[changed] = alt[changed] + "A"
    write_cols_vcf(tmp_path / "other.vcf", names, "chr21", a["ref_pos"], inputs["ids"], inputs["ref"], alt, truth_gt)
    args = inputs["common"] + ["--vcf_site_columns", "--no_vcf"]
    I.infer(args + ["--truth_vcf", str(tmp_path / "truth.vcf"), "-o", str(tmp_path / "same")])
    assert "allele_mismatch=0" in capsys.readouterr().out
    I.infer(args + ["--truth_vcf", str(tmp_path / "other.vcf"), "-o", str(tmp_path / "other")])
    assert "allele_mismatch=1" in capsys.readouterr().out
    q, r = np.load(tmp_path / "same" / "quality.npz"), np.load(tmp_path / "other" / "quality.npz")
    assert int(q["allele_mismatch"]) == 0 and int(r["allele_mismatch"]) == 1
    assert q["truth_row"][changed] == changed and r["truth_row"][changed] == -1
    rest = np.arange(n) != changed
    np.testing.assert_array_equal(q["truth_row"][rest], r["truth_row"][rest])
    assert np.array_equal(q["truth_row"] >= 0, q["flag"]) and q["flag"][changed] and n == len(q["truth_row"])
    for k in ("acc", "table", "acc_n", "acc_r2", "concordance", "nonref_concordance", "est"):
        assert np.array_equal(q[k][rest], r[k][rest], equal_nan=True), k
    assert q["acc_n"][changed] == 6 and r["acc_n"][changed] == 0
