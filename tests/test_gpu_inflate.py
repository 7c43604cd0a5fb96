"""GPU tests of the device inflate (csrc/inflate.hip, read_vcf(inflate="device")): the kernel against zlib over
every deflate block form at odd and packed output offsets with sentinels around, its statuses on broken streams
against the specification (src/dataset/bgzf.py), the CRC verdict, the last-newline reduction, and read_vcf on
BGZF files against the host-inflate path and parse_vcf_host, with the fallbacks, errors and entry-point wiring."""

import gzip
import struct
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bgzf_corpus import corpus, deflate, negatives, vcf_text  # noqa: E402
from test_gpu_vcf_reader import mixed_text, same_as_host, same_bits, write_common_files  # noqa: E402

DEV = "cuda"
SENTINEL = 0xA5


def V():
    from src.dataset import vcf_reader
    return vcf_reader


def B():
    from src.dataset import bgzf
    return bgzf


def K():
    from src import kernels
    return kernels


def inflate_blocks(blocks, gaps, lead=5):
    """One launch over ``blocks`` [(payload, isize, crc)]: block i is written ``gaps[i]`` bytes behind block i - 1
    (``lead`` behind the buffer start) into a text buffer full of sentinels.  Returns (status, text, out_off)."""
    comp, in_off, out_off, o = b"", [], [], lead
    for (payload, isize, crc), gap in zip(blocks, gaps):
        comp += b"\xee" * 3                                   # never part of a block's range
        in_off.append(len(comp))
        comp += payload
        o += gap
        out_off.append(o)
        o += isize
    text = torch.full((o + 37,), SENTINEL, dtype=torch.uint8, device=DEV)
    table = K().bgzf_table(in_off, out_off, [len(b[0]) for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks])
    comp_d = torch.frombuffer(bytearray(comp + b"\0"), dtype=torch.uint8).to(DEV)
    status = K().bgzf_inflate(comp_d, table, text)
    torch.cuda.synchronize()
    return status.cpu().numpy(), text.cpu().numpy(), out_off


def check_ranges(text, out_off, blocks, want):
    """Every block's range holds ``want[i]`` (None: untouched) and every other byte is still a sentinel."""
    mask = np.ones(len(text), bool)
    for off, (_, isize, _), w in zip(out_off, blocks, want):
        got = text[off:off + isize]
        if w is None:
            assert (got == SENTINEL).all()
        else:
            assert got.tobytes() == w
        mask[off:off + isize] = False
    assert (text[mask] == SENTINEL).all()


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["odd_offsets", "packed"])
def test_kernel_equals_zlib(layout):
    items = list(corpus())
    empty = ("empty", b"", deflate(b""))
    items[3:3] = [empty]
    items[9:9] = [empty, empty]
    items += [empty]
    assert 30 <= len(items) <= 50
    blocks = [(p, len(d), zlib.crc32(d)) for _, d, p in items]
    gaps = [0] * len(blocks) if layout == "packed" else [1 + (7 * i) % 13 for i in range(len(blocks))]
    status, text, out_off = inflate_blocks(blocks, gaps)
    assert (np.array(out_off) % 16 != 0).any()
    assert not status.any(), dict(zip([n for n, _, _ in items], status))
    check_ranges(text, out_off, blocks, [d for _, d, _ in items])


def test_300_small_blocks_in_one_launch():
    rng = np.random.default_rng(5)
    text = vcf_text(40000, seed=9)
    datas = []
    for i in range(300):
        n, o = int(rng.integers(1, 3001)), int(rng.integers(0, 30000))
        datas.append(text[o:o + n] if i % 3 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    blocks = [(deflate(d), len(d), zlib.crc32(d)) for d in datas]
    status, out, out_off = inflate_blocks(blocks, [i % 3 for i in range(300)])
    assert not status.any()
    check_ranges(out, out_off, blocks, datas)


def test_broken_streams_get_their_status_beside_good_blocks():
    good = [(p, len(d), zlib.crc32(d), d) for name, d, p in corpus() if name in ("fixed", "rle", "size_259", "huffman_only")]
    blocks, want_status, want_bytes = [], [], []
    for i, (name, payload, isize, crc, _) in enumerate(negatives()):
        g = good[i % len(good)]
        blocks.append(g[:3])
        want_status.append(0)
        want_bytes.append(g[3])
        data, st = B().inflate_member_host(payload, isize, crc)
        blocks.append((payload, isize, crc))
        want_status.append(st)
        want_bytes.append(data if st == 9 else None)          # a block is written only when it inflated
    status, text, out_off = inflate_blocks(blocks, [2 + i % 5 for i in range(len(blocks))])
    np.testing.assert_array_equal(status, want_status)
    assert set(range(10)) <= set(want_status)
    check_ranges(text, out_off, blocks, want_bytes)


def stored(data: bytes) -> bytes:
    out, n = b"", max(1, (len(data) + 65534) // 65535)
    for i in range(n):
        piece = data[i * 65535:(i + 1) * 65535]
        out += bytes([1 if i == n - 1 else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece
    return out


def test_crc_verdict_equals_zlib():
    rng = np.random.default_rng(1)
    blocks, want, datas = [], [], []
    for n in (0, 1, 63, 64, 65, 1023, 1024, 65280, 65536):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for crc, st in ((zlib.crc32(d), 0), (zlib.crc32(d) ^ 1, 9), (zlib.crc32(d + b"\0"), 9)):
            blocks.append((stored(d), n, crc))
            want.append(st)
            datas.append(d)
    status, text, out_off = inflate_blocks(blocks, [3] * len(blocks))
    np.testing.assert_array_equal(status, want)
    check_ranges(text, out_off, blocks, datas)


def test_launcher_refuses_ranges_outside_the_buffers():
    d = b"abc" * 10
    p = deflate(d)
    comp = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(DEV)
    text = torch.full((64,), SENTINEL, dtype=torch.uint8, device=DEV)
    for in_off, out_off, in_len, isize in ((0, 0, -1, 30), (0, 0, len(p), 65537), (1, 0, len(p), 30), (-1, 0, 4, 30),
                                           (0, 35, len(p), 30), (0, -1, len(p), 30), (0, 0, len(p) + 1, 30)):
        with pytest.raises(Exception, match="bgzf_inflate"):
            K().bgzf_inflate(comp, K().bgzf_table([in_off], [out_off], [in_len], [isize], [0]), text)
    torch.cuda.synchronize()
    assert (text.cpu().numpy() == SENTINEL).all()
    st = K().bgzf_inflate(comp, K().bgzf_table([0], [34], [len(p)], [30], [zlib.crc32(d)]), text)
    assert st.cpu().tolist() == [0] and text.cpu().numpy()[34:].tobytes() == d


def test_text_last_newline():
    span = 4096
    cases = []
    for n in (1, 15, 16, 17, span - 1, span, span + 1, 3 * span + 5):
        cases += [(n, None), (n, 0), (n, n - 1)]
    cases += [(3 * span + 5, span - 1), (3 * span + 5, span), (3 * span + 5, 7), (2 * span, span + 16)]
    for n, at in cases:
        a = np.full((n + 31) // 16 * 16, ord("x"), np.uint8)
        a[n:] = 10                                            # newlines behind nbytes do not count
        want = -1
        if at is not None:
            a[at] = 10
            want = at
            if at > 3:
                a[at // 2] = 10                               # an earlier one does not win
        got = K().text_last_newline(torch.from_numpy(a).to(DEV), n)
        assert int(got.item()) == want, (n, at)
    assert int(K().text_last_newline(torch.zeros(16, dtype=torch.uint8, device=DEV), 0).item()) == -1


def three_ways(path, chunk_bytes, **kw):
    """read_vcf(inflate="device") == read_vcf(inflate="host") == parse_vcf_host."""
    host, _ = same_as_host(path, chunk_bytes=chunk_bytes, inflate="host", **kw)
    dev, _ = same_as_host(path, chunk_bytes=chunk_bytes, inflate="device", **kw)
    same_bits(host, dev)
    assert host.samples == dev.samples and host.n_sites == dev.n_sites
    return dev


def vcf_bytes(S, n, seed):
    rng = np.random.default_rng(seed)
    gt = (rng.random((n, S, 2)) < 0.3).astype(np.int8)
    pos = np.cumsum(rng.integers(1, 10 ** 5, n)).astype(np.int32)
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"S{i}" for i in range(S))]
    for i in range(n):
        lines.append(f"1\t{pos[i]}\t.\tA\tC\t.\tPASS\t.\tGT\t" + "\t".join(f"{a}|{b}" for a, b in gt[i]))
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("S", [1, 65, 257])
def test_read_vcf_device_inflate_equals_host(tmp_path, S):
    line = 4 * S + 40
    for n in (1, 64, 65, 130):
        data = vcf_bytes(S, n, seed=S + n)
        # blocks far smaller than a line (a line spans blocks and chunks), a few lines per block, htslib's size
        for bs, chunk in ((200, max(4096 if S == 65 else 2 * line, 512)), (4096, 3 * max(line, 4096)), (0xff00, 1 << 20)):
            path = tmp_path / f"s{S}_n{n}_b{bs}.vcf.gz"
            B().write_bgzf(path, data, block_size=bs)
            vg = three_ways(path, chunk)
            assert vg.n_sites == n


def test_read_vcf_write_gt_vcf_bgzf(tmp_path):
    rng = np.random.default_rng(3)
    gt = (rng.random((130, 65, 2)) < 0.3).astype(np.int8)
    path = tmp_path / "w.vcf.gz"
    V().write_gt_vcf(path, [f"S{i}" for i in range(65)], np.arange(1, 131) * 7, gt, bgzf=True)
    assert B().is_bgzf(path)
    vg = three_ways(path, 1 << 17)                            # htslib-size blocks: a chunk holds at least one
    np.testing.assert_array_equal(vg.gt(), gt)


@pytest.mark.parametrize("kind", ["mixed", "crlf", "no_final_newline", "no_eof_block", "empty_block", "long_header"])
def test_read_vcf_device_inflate_file_forms(tmp_path, kind):
    path = tmp_path / f"{kind}.vcf.gz"
    data = mixed_text(70, 5, seed=4, crlf=kind == "crlf", final_newline=kind != "no_final_newline")
    if kind == "long_header":
        head, body = data.split(b"#CHROM", 1)
        data = head + b"".join(b"##INFO=<ID=X%d,Description=\"%s\">\n" % (i, b"y" * 300) for i in range(20)) + b"#CHROM" + body
    if kind == "empty_block":
        members = [B().bgzf_member(data[o:o + 700]) for o in range(0, len(data), 700)]
        members[3:3] = [B().bgzf_member(b""), B().bgzf_member(b"")]
        path.write_bytes(b"".join(members) + B().EOF_BLOCK)
    else:
        B().write_bgzf(path, data, block_size=1000 if kind == "long_header" else 700, eof=kind != "no_eof_block")
    assert gzip.decompress(path.read_bytes()) == data
    a = three_ways(path, 4096)
    b = three_ways(path, 4096, force_general=True)
    same_bits(a, b)


def test_fallbacks_print_one_line_and_read_on_the_host(tmp_path, capsys):
    data = vcf_bytes(5, 70, seed=1)
    plain, single = tmp_path / "p.vcf", tmp_path / "g.vcf.gz"
    plain.write_bytes(data)
    single.write_bytes(gzip.compress(data))
    for path in (plain, single):
        capsys.readouterr()
        host = V().read_vcf(path, DEV, chunk_bytes=4096, inflate="host")
        assert capsys.readouterr().out == ""
        dev = V().read_vcf(path, DEV, chunk_bytes=4096, inflate="device")
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and str(path) in out and "host" in out
        same_bits(host, dev)
    with pytest.raises(ValueError, match="inflate"):
        V().read_vcf(plain, DEV, inflate="gpu")


def test_errors_name_the_block_or_the_line(tmp_path):
    data = vcf_bytes(9, 200, seed=2)
    members = [B().bgzf_member(data[o:o + 900], level=0) for o in range(0, len(data), 900)]
    offs = np.cumsum([0] + [len(m) for m in members])
    good = b"".join(members) + B().EOF_BLOCK
    k = 5
    bad = bytearray(good)
    bad[offs[k] + 18 + 5 + 100] ^= 0x40                       # one payload byte of block k: a stored literal
    p = tmp_path / "flip.vcf.gz"
    p.write_bytes(bad)
    with pytest.raises(ValueError, match=rf"flip.vcf.gz: BGZF block at byte {offs[k]}: CRC mismatch"):
        V().read_vcf(p, DEV, chunk_bytes=4096, inflate="device")
    bad = bytearray(good)
    bad[offs[k] + 18 + 3] ^= 1                                # NLEN of block k
    p.write_bytes(bad)
    with pytest.raises(ValueError, match=rf"BGZF block at byte {offs[k]}: stored block LEN / NLEN mismatch"):
        V().read_vcf(p, DEV, chunk_bytes=4096, inflate="device")
    p = tmp_path / "cut.vcf.gz"
    p.write_bytes(good[:offs[7] + 40])
    with pytest.raises(ValueError, match=rf"cut.vcf.gz: BGZF block at byte {offs[7]}: truncated"):
        V().read_vcf(p, DEV, chunk_bytes=4096, inflate="device")
    p = tmp_path / "small.vcf.gz"
    p.write_bytes(good)
    with pytest.raises(ValueError, match="chunk_bytes"):
        V().read_vcf(p, DEV, chunk_bytes=512, inflate="device")
    lines = data.split(b"\n")
    lines[40] = lines[40].replace(b"\tGT\t", b"\tDS\t")
    p = tmp_path / "record.vcf.gz"
    B().write_bgzf(p, b"\n".join(lines), block_size=900)
    errs = []
    for mode in ("host", "device"):
        with pytest.raises(ValueError) as e:
            V().read_vcf(p, DEV, chunk_bytes=4096, inflate=mode)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "line 41" in errs[0]
    # a body of lines shorter than any record fails in its chunk's line index; a bad block in a later chunk comes first
    head, body = data.split(b"\n", 2)[:2], data.split(b"\n", 2)[2]
    short = b"\n".join(head) + b"\n" + b"x\n" * 3000 + body
    members = [B().bgzf_member(short[o:o + 900], level=0) for o in range(0, len(short), 900)]
    offs = np.cumsum([0] + [len(m) for m in members])
    p = tmp_path / "short.vcf.gz"
    p.write_bytes(b"".join(members) + B().EOF_BLOCK)
    errs = []
    for mode in ("host", "device"):
        with pytest.raises(ValueError) as e:
            V().read_vcf(p, DEV, chunk_bytes=4096, inflate=mode)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "BGZF" not in errs[0]
    bad = bytearray(p.read_bytes())
    k = len(members) - 3
    bad[offs[k] + 18 + 5 + 100] ^= 0x40
    p.write_bytes(bad)
    with pytest.raises(ValueError, match=rf"BGZF block at byte {offs[k]}: CRC mismatch"):
        V().read_vcf(p, DEV, chunk_bytes=4096, inflate="device")


def test_entry_points_follow_the_default(tmp_path):
    from src.dataset.synthetic import make_infer_arrays
    from src import infer_embedding_rag as I, train_embedding_rag as T
    assert I.parse_args([]).vcf_inflate == "host" and T.parse_args([]).vcf_inflate == "host"
    assert I.parse_args(["--vcf_inflate", "device"]).vcf_inflate == "device"
    assert T.parse_args(["--vcf_inflate", "device"]).vcf_inflate == "device"
    a = make_infer_arrays(1300, 6, 24, missing_rate=0.3, ref_missing=5, seed=11)
    samples = [f"S{i}" for i in range(6)]
    V().write_gt_vcf(tmp_path / "target.vcf.gz", samples, a["pos"], a["vcf"], bgzf=True)
    V().write_gt_vcf(tmp_path / "panel.vcf.gz", [f"R{i}" for i in range(24)], a["ref_pos"], a["ref_gt"], bgzf=True)
    write_common_files(tmp_path, a, samples)
    dev = torch.device("cuda", torch.cuda.current_device())
    assert V().DEFAULT_INFLATE == "host"
    seen = {}
    real = V()._read_vcf_device_inflate
    calls = []
    try:
        V()._read_vcf_device_inflate = lambda *a_, **k_: (calls.append(a_[1]), real(*a_, **k_))[1]
        for mode in ("host", "device"):
            args = I.parse_args(["--infer_dataset", str(tmp_path / "target.vcf.gz"), "--infer_panel", str(tmp_path / "panel.txt"),
                                 "--freq_path", str(tmp_path / "freq.npy"), "--type_path", str(tmp_path / "type.pkl"),
                                 "--pop_path", str(tmp_path / "pop.pkl"), "--pos_path", str(tmp_path / "pos.pkl"),
                                 "--ref_panel", str(tmp_path / "panel.vcf.gz"), "--vcf_inflate", mode,
                                 "-d", "64", "-l", "2", "-a", "2", "-b", "4", "--k_retrieve", "3"])
            V().set_default_inflate(args.vcf_inflate)
            ds, _ = I.build_dataset(args)
            seen[mode] = (ds.vcf.copy(), ds.panel_index(0, dev).data.clone(), ds.panel_index(1, dev).data.clone(),
                          ds.vcf_genotypes.alt_bits.clone(), ds.ref_panel_vcf.alt_bits.clone(), ds.ref_panel_vcf.miss_bits.clone())
            assert len(calls) == (0 if mode == "host" else 2)
    finally:
        V()._read_vcf_device_inflate = real
        V().set_default_inflate("host")
    np.testing.assert_array_equal(seen["host"][0], a["vcf"])
    np.testing.assert_array_equal(seen["host"][0], seen["device"][0])
    for x, y in zip(seen["host"][1:], seen["device"][1:]):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        V().set_default_inflate("gpu")


def test_new_kernels_use_no_scratch():
    """CPU-side: the code-object metadata of the inflate and last-newline kernels (the CRC is folded into the
    inflate kernel) reports no private segment and no spills."""
    import test_kernel_resources as R
    res = R._kernel_resources()
    for prefix in ("snvrag::bgzf_inflate_kernel", "snvrag::text_last_newline_kernel"):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert hits, prefix
        for k, (scratch, spills) in hits.items():
            assert scratch == 0 and spills == 0, (k, scratch, spills)
