"""GPU tests of the device deflate (csrc/deflate.hip, write_vcf_device(bgzf=True), --vcf_bgzf): the kernel against
zlib over the corpus and the edge lengths with sentinels behind every member, its independence of the grid and
its equality with the host build of csrc/deflate_core.h, the pack kernels, the size conditions, the round trip
through the device inflate, and the writer against the host writer's file, with the fallback, the refusals and the
entry-point wiring."""

import gzip
import os
import zlib

import numpy as np
import pytest
import torch

from deflate_cases import B, cell_text, check_member, core_T, edge_inputs, window_pair, zlib_members
from test_deflate_core_cpu import BUILDS, build_and_run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = 0xA5
SLOT = 65536


def K():
    from src import kernels
    return kernels


def deflate(data: bytes, block_size: int = 0xff00, shift: int = 0):
    """One launch over ``data`` placed ``shift`` bytes into its buffer: the members as bytes, after checking that
    every length is at most 65 536 and every slot byte past its member still holds the sentinel."""
    n = len(data)
    text = torch.frombuffer(bytearray(b"\x5a" * shift + data + b"\x5a"), dtype=torch.uint8).to(DEV)[shift:shift + n]
    nb = -(-n // block_size)
    slots = torch.full((nb, SLOT), SENTINEL, dtype=torch.uint8, device=DEV)
    lens = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    members, member_len = K().bgzf_deflate(text, n, block_size, slots, lens)
    torch.cuda.synchronize()
    lens, slots = member_len.cpu().numpy(), members.cpu().numpy()
    assert lens.shape == (nb,) and (lens >= 28).all() and (lens <= SLOT).all()
    past = np.arange(SLOT)[None, :] >= lens[:, None]
    assert (slots[past] == SENTINEL).all()
    return [slots[b, :lens[b]].tobytes() for b in range(nb)]


def check_members(members, data, block_size):
    assert len(members) == -(-len(data) // block_size)
    for b, m in enumerate(members):
        check_member(m, data[b * block_size:(b + 1) * block_size])


@pytest.fixture(scope="module")
def edge_members():
    """name -> (data, member) of every edge input, one launch each (an edge length is a launch's last piece)."""
    return {name: (data, deflate(data)[0] if data else b"") for name, data in edge_inputs()}


def test_every_edge_input_round_trips_through_zlib(edge_members):
    for name, (data, member) in edge_members.items():
        if data:
            check_member(member, data)
    data, member = edge_members["random_ff00"]
    assert len(member) == 0xff00 + 31 and member[18] == 1                 # incompressible: one stored block


@pytest.mark.parametrize("block_size,nbytes", [(1, 600), (7, 5000), (259, 70001), (0xff00, 400000)])
def test_one_launch_over_many_members(block_size, nbytes):
    data = b"".join(d for _, d in edge_inputs())
    data = data[40000:40000 + nbytes]                                     # text, then runs, then random bytes
    assert len(data) == nbytes
    members = deflate(data, block_size)
    check_members(members, data, block_size)
    assert deflate(data, block_size, shift=1) == members                  # a text pointer at an odd offset
    assert deflate(data, block_size, shift=6) == members


def test_members_do_not_depend_on_the_grid():
    rng = np.random.default_rng(31)
    piece = cell_text(0.9, lines=4)[:0xff00]
    assert len(piece) == 0xff00
    other = [rng.integers(0, 4, 0xff00, dtype=np.uint8).tobytes(), bytes(0xff00), cell_text(0.0, lines=4)[:0xff00]]
    a = deflate(piece + other[0])
    b = deflate(b"".join(other[i % 3] for i in range(37)) + piece + other[1] * 2)
    assert a[0] == b[37] and a[1] == b[0]
    assert deflate(piece + other[0]) == a


def test_members_equal_the_host_build(tmp_path, edge_members):
    """The device's bytes are those of the host program built from the same csrc/deflate_core.h."""
    keep = {f"{i:03d}": (data, member) for i, (name, (data, member)) in enumerate(edge_members.items())
            if data and (name.startswith(("corpus_", "window_", "vcf_ff00", "cells_")) or name.endswith(str(core_T() + 1)))}
    assert len(keep) > 30
    host = build_and_run(tmp_path, BUILDS["plain"], {k: d for k, (d, _) in keep.items()})
    diff = [k for k, (_, member) in keep.items() if host[k] != member]
    assert not diff, diff


def pack(lens, slack=0, rng=None):
    rng = rng or np.random.default_rng(len(lens))
    n, total = len(lens), int(np.sum(lens))
    slots = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
    want = b"".join(slots[b, :lens[b]].tobytes() for b in range(n))
    lead = 3
    buf = torch.full((lead + total + slack + 40,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = buf[lead:lead + total + slack]
    got = K().bgzf_pack(torch.from_numpy(slots).to(DEV), torch.from_numpy(np.asarray(lens, np.int32)).to(DEV), out)
    torch.cuda.synchronize()
    return int(got.item()), buf.cpu().numpy(), lead, want


@pytest.mark.parametrize("n", [1, 255, 256, 257, 300, 700])
def test_pack(n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 400, n)
    lens[rng.integers(0, n, 3)] = (SLOT, 0, 28)
    lens[n // 2] = 65519
    total, buf, lead, want = pack(lens, slack=5)
    assert total == len(want) == int(lens.sum())
    assert buf[lead:lead + total].tobytes() == want
    assert (buf[:lead] == SENTINEL).all() and (buf[lead + total:] == SENTINEL).all()
    if n == 300:
        total, buf, _, _ = pack(lens, slack=-1)                           # one byte too small
        assert total == -1 and (buf == SENTINEL).all()
        lens[7] = SLOT + 1                                                # no member is that long
        total, buf, _, _ = pack(lens, slack=5)
        assert total == -1 and (buf == SENTINEL).all()


@pytest.mark.parametrize("confident", [0.9, 0.99, 0.0])
def test_size_conditions(confident):
    text = cell_text(confident)
    raw = B.deflate_device(text, device=DEV)
    assert gzip.decompress(raw) == text
    blocks, used = B.bgzf_blocks(raw)
    assert used == len(raw) and len(blocks) == -(-len(text) // 0xff00)
    l1, l6 = zlib_members(text, 1), zlib_members(text, 6)
    bound = zlib_members(text, 1, zlib.Z_FIXED) if confident == 0.0 else zlib_members(text, 6, zlib.Z_HUFFMAN_ONLY)
    print(f"confident {confident}: text {len(text)}  device {len(raw)}  zlib-1 {l1}  zlib-6 {l6}  bound {bound}")
    assert len(raw) < bound, (len(raw), bound)


def test_device_inflate_reads_what_the_device_deflated():
    text = cell_text(0.5, lines=12) + window_pair(32768) + bytes(1000)
    raw = B.deflate_device(text, block_size=0xff00, device=DEV)
    blocks, used = B.bgzf_blocks(raw)
    assert used == len(raw)
    out_off = np.concatenate([[0], np.cumsum([b.isize for b in blocks])])
    assert int(out_off[-1]) == len(text)
    table = K().bgzf_table([b.payload_off for b in blocks], out_off[:-1], [b.payload_len for b in blocks],
                           [b.isize for b in blocks], [b.crc for b in blocks])
    comp = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    out = torch.full((len(text) + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = K().bgzf_inflate(comp, table, out)
    assert (status.cpu().numpy() == 0).all()
    assert out[:len(text)].cpu().numpy().tobytes() == text


def writer_case(S=500, n=10):
    rng = np.random.default_rng(77)
    gt = rng.dirichlet(np.ones(4) * 0.3, (n, S)).astype(np.float32)
    sure = rng.random((n, S)) < 0.5
    gt[sure] = np.eye(4, dtype=np.float32)[rng.integers(0, 4, int(sure.sum()))]
    h1, h2 = gt[..., 2] + gt[..., 3], gt[..., 1] + gt[..., 3]
    flag = np.ones(n, bool)
    flag[[2, 7]] = False
    return dict(h1=h1, h2=h2, gt=gt, pos=np.arange(n) * 100 + 11, samples=[f"S{i}" for i in range(S)], flag=flag)


def write_both(tmp_path, c, form="device", expect=True, **kw):
    from src.infer_embedding_rag import write_vcf, write_vcf_device
    conv = (lambda a: torch.from_numpy(a.copy()).to(DEV)) if form == "device" else (lambda a: a)
    write_vcf(tmp_path / "host.vcf", "21", c["pos"], c["h1"], c["h2"], c["gt"], c["samples"], pos_flag=c["flag"])
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    ok = write_vcf_device(out / "dev.vcf.gz", "21", c["pos"], conv(c["h1"]), conv(c["h2"]), conv(c["gt"]), c["samples"],
                          pos_flag=c["flag"], device=DEV, bgzf=True, **kw)
    assert ok is expect
    assert os.listdir(out) == ["dev.vcf.gz"]
    return (out / "dev.vcf.gz").read_bytes(), (tmp_path / "host.vcf").read_bytes()


@pytest.mark.parametrize("chunk_lines", [None, 3])
def test_writer_bgzf_inflates_to_the_host_writers_file(tmp_path, chunk_lines):
    from src import vcf_device as V
    from src.dataset.vcf_reader import read_vcf
    c = writer_case()
    kw = {}
    if chunk_lines:
        _, _, p_off = V.site_prefixes("21", c["pos"], c["flag"])
        kw["chunk_bytes"] = int(V.line_lengths(p_off, 500).max()) * chunk_lines
    raw, want = write_both(tmp_path, c, **kw)
    assert gzip.decompress(raw) == want
    blocks, used = B.bgzf_blocks(raw)
    assert used == len(raw) and raw[-28:] == B.EOF_BLOCK
    n_chunks = 3 if chunk_lines else 1
    assert len(blocks) == 1 + sum(-(-nb // 0xff00) for nb in chunk_sizes(c, n_chunks)) + 1   # header, chunks, EOF
    got = read_vcf(tmp_path / "out" / "dev.vcf.gz", DEV, inflate="device")
    g = np.argmax(c["gt"][c["flag"]], -1)
    assert np.array_equal(got.pos, c["pos"][c["flag"]])
    assert np.array_equal(got.gt(), np.stack([g >> 1, g & 1], -1).astype(np.int8))


def chunk_sizes(c, n_chunks):
    from src import vcf_device as V
    _, _, p_off = V.site_prefixes("21", c["pos"], c["flag"])
    length = V.line_lengths(p_off, len(c["samples"]))
    per = -(-len(length) // n_chunks)
    return [int(length[i:i + per].sum()) for i in range(0, len(length), per)]


@pytest.mark.parametrize("form", ["device", "numpy"])
def test_writer_bgzf_falls_back_to_the_host_writer(tmp_path, capsys, form):
    c = writer_case(S=70)
    c["h1"] = c["h1"].copy()
    c["h1"][8, 40] = np.nan
    raw, want = write_both(tmp_path, c, form=form, expect=False)
    assert gzip.decompress(raw) == want and raw[-28:] == B.EOF_BLOCK
    note = capsys.readouterr().out
    assert note.count("\n") == 1 and "host writer" in note


def test_refusals():
    from src import native as N
    lib = N.lib()
    text = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    slots = torch.full((4 * SLOT + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    lens = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    t, s, l = text.data_ptr(), slots.data_ptr(), lens.data_ptr()
    for args in ((None, 100, 0xff00, s, l), (t, 100, 0xff00, None, l), (t, 100, 0xff00, s, None), (t, -1, 0xff00, s, l),
                 (t, 1 << 31, 0xff00, s, l), (t, 100, 0, s, l), (t, 100, 0xff01, s, l), (t, 100, 0xff00, s + 1, l),
                 (t, 100, 0xff00, s + 8, l)):
        assert lib.snvrag_bgzf_deflate(*args, N.stream_ptr()) != 0, args
    assert lib.snvrag_bgzf_deflate(t, 0, 0xff00, s, l, N.stream_ptr()) == 0
    for kw in (dict(block_size=0), dict(block_size=0xff01), dict(nbytes=-1), dict(nbytes=4097), dict(members=slots[1:])):
        with pytest.raises(ValueError, match="bgzf_deflate"):
            K().bgzf_deflate(text, **{**dict(nbytes=100, block_size=0xff00, members=slots, member_len=lens), **kw})
    total = torch.full((1,), -5, dtype=torch.int64, device=DEV)
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=DEV)
    o, tt = out.data_ptr(), total.data_ptr()
    for args in ((None, l, 4, o, 64, tt), (s, None, 4, o, 64, tt), (s, l, 4, None, 64, tt), (s, l, 4, o, 64, None),
                 (s, l, -1, o, 64, tt), (s, l, 4, o, -1, tt), (s + 1, l, 4, o, 64, tt)):
        assert lib.snvrag_bgzf_pack(*args, N.stream_ptr()) != 0, args
    torch.cuda.synchronize()
    assert (slots.cpu().numpy() == SENTINEL).all() and (lens.cpu().numpy() == -7).all()       # nothing was launched
    assert int(total.item()) == -5 and (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError, match="block_size"):
        B.deflate_device(b"abc", block_size=0x10000, device=DEV)
    assert B.deflate_device(b"", device=DEV) == b""


def test_infer_cli_writes_imputed_vcf_gz(tmp_path):
    from src import infer_embedding_rag as I
    args = ["--synthetic", "6", "--synthetic_sites", "2040", "--synthetic_ref", "24", "-d", "64", "-l", "2", "-a", "2",
            "-b", "4", "--k_retrieve", "3", "--mask_rate", "0.5", "--index_window_len", "1020", "--vcf_writer", "device"]
    I.infer(args + ["-o", str(tmp_path / "plain")])
    I.infer(args + ["--vcf_bgzf", "-o", str(tmp_path / "bgzf")])
    assert sorted(os.listdir(tmp_path / "bgzf")) == ["imputed.npz", "imputed.vcf.gz"]
    raw, want = (tmp_path / "bgzf" / "imputed.vcf.gz").read_bytes(), (tmp_path / "plain" / "imputed.vcf").read_bytes()
    assert want.count(b"\n") > 7 + 500 and gzip.decompress(raw) == want and raw[-28:] == B.EOF_BLOCK
    I.infer(args[:-2] + ["--vcf_bgzf", "-o", str(tmp_path / "host")])                         # --vcf_writer host: zlib
    assert gzip.decompress((tmp_path / "host" / "imputed.vcf.gz").read_bytes()) == want
