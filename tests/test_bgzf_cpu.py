"""src/dataset/bgzf.py on the host: inflate_block_host (the specification of the device inflate) against zlib
over every deflate block form, its status codes on broken streams, the member walk and the writer."""

import gzip
import struct
import sys
import zlib
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from src.dataset import bgzf as B  # noqa: E402
from bgzf_corpus import corpus, negatives, short_dynamic  # noqa: E402


@pytest.mark.parametrize("i", range(len(corpus())), ids=[c[0] for c in corpus()])
def test_host_decoder_equals_zlib(i):
    name, data, payload = corpus()[i]
    got, st = B.inflate_block_host(payload, len(data))
    assert st == B.OK, name
    assert got == data == zlib.decompress(payload, -15)
    assert B.inflate_member_host(payload, len(data), zlib.crc32(data))[1] == B.OK


def test_corpus_covers_the_block_forms():
    first = {name: (payload[0] >> 1) & 3 for name, _, payload in corpus()}
    assert first["stored_65280"] == 0 and first["random_65280"] == 0
    assert first["fixed"] == 1
    assert first["dynamic_text_65280"] == 2 and first["rle"] == 2 and first["huffman_only"] == 2
    by = {name: payload for name, _, payload in corpus()}
    assert len(by["random_65280"]) + 26 == 65326              # zlib's stored fallback: BSIZE + 1 = 65 326
    # more than one stored block per member: the first one is not the last
    assert not by["stored_65280"][0] & 1
    assert not by["stored_flushed"][0] & 1 and struct.unpack_from("<H", by["stored_flushed"], 1)[0] == 3000
    assert not by["mem_level_1"][0] & 1                       # the first dynamic block is not the last
    tr = {}
    for name, data, payload in corpus():
        tr[name] = {}
        assert B.inflate_block_host(payload, len(data), tr[name]) == (data, B.OK)
    assert tr["stored_flushed"]["block_types"].count(0) >= 3
    assert tr["mem_level_1"]["block_types"].count(2) >= 3     # several dynamic blocks in one member
    assert tr["rle"]["matches"] and {d for _, d, _ in tr["rle"]["matches"]} == {1}        # distance 1 only,
    assert max(n for _, _, n in tr["rle"]["matches"]) == 258                                # overlapping, up to 258
    assert tr["huffman_only"]["block_types"] == [2] and not tr["huffman_only"]["matches"]  # no distance at all
    assert tr["fibonacci_lengths"]["max_code_length"] == 15 and not tr["fibonacci_lengths"]["matches"]
    far = tr["distance_32768"]["matches"]
    assert far[0] == (32768, 32768, 258)                      # the source is exactly the block's first byte
    assert max(d for _, d, _ in far) == 32768 and (33029, 32768, 3) in far and far[-1][1:] == (32767, 258)
    assert tr["distance_32768"]["block_types"] == [0, 1]
    one = tr["one_code_distance_tree"]
    assert one["incomplete_distance_trees"] == 1 and one["matches"] == [(1, 1, 3), (4, 1, 3)]
    assert all(t.get("incomplete_distance_trees", 0) == 0 for n, t in tr.items() if n != "one_code_distance_tree")
    assert any(p < d + n and d < n for t in tr.values() for p, d, n in t["matches"])       # distance < length


@pytest.mark.parametrize("i", range(len(negatives())), ids=[c[0] for c in negatives()])
def test_each_broken_stream_has_its_status(i):
    name, payload, isize, crc, want = negatives()[i]
    data, st = B.inflate_member_host(payload, isize, crc)       # never raises
    if want is None:
        assert st in (B.INPUT_END, B.OUTPUT_SHORT), (name, st)
    else:
        assert st == want, (name, st)
    assert len(data) <= isize


def test_cut_payloads_mostly_run_out_of_input():
    sts = [B.inflate_block_host(p, n)[1] for name, p, n, _, want in negatives() if want is None]
    assert len(sts) >= 5 and B.INPUT_END in sts


def test_blocks_walk_bc_behind_another_subfield_and_partial_tail():
    data = b"hello bgzf\n" * 50
    payload = zlib.compress(data)[2:-4]
    extra = b"XY\x03\x00abc" + b"BC\x02\x00"
    bsize = 12 + len(extra) + 2 + len(payload) + 8 - 1
    member = (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra) + 2) + extra + struct.pack("<H", bsize) +
              payload + struct.pack("<II", zlib.crc32(data), len(data)))
    assert gzip.decompress(member) == data
    plain = B.bgzf_member(data)
    buf = member + plain + plain[:30]
    blocks, used = B.bgzf_blocks(buf, base=1000)
    assert used == len(member) + len(plain) and len(blocks) == 2
    b0, b1 = blocks
    assert (b0.file_off, b0.payload_off, b0.payload_len, b0.isize, b0.crc) == (
        1000, 12 + len(extra) + 2, len(payload), len(data), zlib.crc32(data))
    assert b1.file_off == 1000 + len(member) and b1.payload_off == len(member) + 18
    for b in blocks:
        assert B.inflate_member_host(buf[b.payload_off:b.payload_off + b.payload_len], b.isize, b.crc) == (data, B.OK)
    assert B.bgzf_blocks(buf[:5]) == ([], 0)
    for bad in (b"\x1f\x8b\x07" + member[3:], member[:3] + b"\0" + member[4:],
                member[:12] + b"XY\x03\x00abcBD" + member[21:]):
        with pytest.raises(ValueError, match="byte 1000"):
            B.bgzf_blocks(bad, base=1000)


def test_write_bgzf_reads_back_through_gzip(tmp_path):
    data = bytes(range(256)) * 1000
    for bs, eof in ((0xff00, True), (200, True), (4096, False)):
        p = tmp_path / f"w{bs}.gz"
        B.write_bgzf(p, data[:50000 if bs == 200 else None], block_size=bs, eof=eof)
        raw = p.read_bytes()
        assert gzip.decompress(raw) == data[:50000 if bs == 200 else None]
        assert raw.endswith(B.EOF_BLOCK) == eof
        assert B.is_bgzf(p)
        blocks, used = B.bgzf_blocks(raw)
        assert used == len(raw) and sum(b.isize for b in blocks) == len(gzip.decompress(raw))
    plain = tmp_path / "plain.gz"
    with gzip.open(plain, "wb") as f:
        f.write(data)
    assert not B.is_bgzf(plain)
    assert len(B.EOF_BLOCK) == 28 and gzip.decompress(B.EOF_BLOCK) == b""


def test_write_gt_vcf_bgzf_keyword(tmp_path):
    import numpy as np
    from src.dataset import vcf_reader as V
    gt = np.zeros((5, 3, 2), np.int8)
    gt[2, 1, 0] = 1
    a, b = tmp_path / "a.vcf.gz", tmp_path / "b.vcf.gz"
    V.write_gt_vcf(a, ["x", "y", "z"], [1, 2, 3, 4, 5], gt)
    V.write_gt_vcf(b, ["x", "y", "z"], [1, 2, 3, 4, 5], gt, bgzf=True)
    assert not B.is_bgzf(a) and B.is_bgzf(b)
    assert gzip.decompress(a.read_bytes()) == gzip.decompress(b.read_bytes())
    short = short_dynamic()
    assert B.inflate_block_host(short[1], len(short[0])) == (short[0], B.OK)
