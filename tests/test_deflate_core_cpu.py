"""csrc/deflate_core.h — the compressor text the device kernel compiles — built as a plain host program
(tests/deflate_core_main.cc), once as it is and once under AddressSanitizer + UBSan, and run over the corpus,
the edge lengths, the window pair and 2 000 random inputs.  Every member must be a BGZF member that zlib (and,
for the small ones, the specification inflate_block_host) inflates to the input; the two builds must agree byte
for byte; the size conditions hold only if matches are found and the dynamic codes work."""

import gzip
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from deflate_cases import B, REPO, cell_text, check_member, core_T, member_inputs, zlib_members

CXX = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
BUILDS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_and_run(tmp, flags, inputs):
    """name -> member bytes of the host build with ``flags`` over ``inputs`` (name -> data)."""
    assert CXX, "no host C++ compiler (g++, c++, clang++): the compressor's bounds cannot be checked"
    src, dst, exe = tmp / "in", tmp / "out", tmp / "deflate_core_main"
    src.mkdir(), dst.mkdir()
    for name, data in inputs.items():
        (src / name).write_bytes(data)
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, "-I", str(REPO / "rag-snvbert_amd" / "csrc"),
                    str(REPO / "tests" / "deflate_core_main.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    return {name: (dst / name).read_bytes() for name in inputs}


@pytest.fixture(scope="module")
def inputs():
    return member_inputs()


@pytest.fixture(scope="module")
def members(tmp_path_factory, inputs):
    return {key: build_and_run(tmp_path_factory.mktemp(key), flags, inputs) for key, flags in BUILDS.items()}


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_member_round_trips_through_zlib(members, inputs, build):
    for name, data in inputs.items():
        check_member(members[build][name], data)


def test_the_two_builds_agree(members):
    assert members["plain"] == members["asan_ubsan"]


def test_the_specification_inflates_the_small_members(members, inputs):
    n = 0
    for name, data in inputs.items():
        if len(data) <= 3000:
            m = members["plain"][name]
            (blk,), _ = B.bgzf_blocks(m)
            got, st = B.inflate_member_host(m[blk.payload_off:blk.payload_off + blk.payload_len], blk.isize, blk.crc)
            assert st == B.OK and got == data, (name, st)
            n += 1
    assert n > 2000


def test_what_the_inputs_exercise(members, inputs):
    """Stored and dynamic members both occur; the window pair is coded with a match at distance 32 768 and with
    none above it; zeros give maximum-length matches at distance 1 .. DEFL_BATCH."""
    by = {name.split("_", 1)[1]: name for name in inputs}
    m = members["plain"][by["random_ff00"]]
    assert len(m) == 0xff00 + 5 + 26 and m[18] == 1                       # one stored block
    for gap, far in ((32768, True), (32769, False)):
        m = members["plain"][by[f"window_{gap}"]]
        (blk,), _ = B.bgzf_blocks(m)
        trace = {}
        _, st = B.inflate_block_host(m[blk.payload_off:blk.payload_off + blk.payload_len], blk.isize, trace)
        assert st == B.OK
        dist = [d for _, d, _ in trace["matches"]]
        assert max(dist) <= 32768 and (32768 in dist) == far, (gap, max(dist))
    m = members["plain"][by["zeros_ff00"]]
    (blk,), _ = B.bgzf_blocks(m)
    trace = {}
    B.inflate_block_host(m[blk.payload_off:blk.payload_off + blk.payload_len], blk.isize, trace)
    assert set(trace["block_types"]) == {2} and len(trace["block_types"]) == -(-0xff00 // core_T())
    assert max(ln for _, _, ln in trace["matches"]) == 258 and len(m) < 2000


@pytest.mark.parametrize("confident", [0.9, 0.99, 0.0])
def test_size_conditions(tmp_path, confident):
    """Confident text: below zlib Z_HUFFMAN_ONLY, which needs matches.  Random probabilities: below zlib Z_FIXED
    level 1, which needs the dynamic codes.  The ratio to level 1 is printed, not fixed."""
    text = cell_text(confident)
    pieces = {f"{i:04d}": text[o:o + 0xff00] for i, o in enumerate(range(0, len(text), 0xff00))}
    got = build_and_run(tmp_path, BUILDS["plain"], pieces)
    for name, data in pieces.items():
        check_member(got[name], data)
    total = sum(map(len, got.values()))
    l1, l6 = zlib_members(text, 1), zlib_members(text, 6)
    bound = zlib_members(text, 1, zlib.Z_FIXED) if confident == 0.0 else zlib_members(text, 6, zlib.Z_HUFFMAN_ONLY)
    print(f"confident {confident}: text {len(text)}  core {total} (ratio {len(text) / total:.2f})  zlib-1 {l1} "
          f"(core / zlib-1 {total / l1:.3f})  zlib-6 {l6} (core / zlib-6 {total / l6:.3f})  bound {bound}")
    assert total < bound, (total, bound)


def test_host_writer_bgzf(tmp_path):
    from src.infer_embedding_rag import write_vcf
    rng = np.random.default_rng(2)
    n, S = 7, 33
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)
    h1, h2 = gt[..., 2] + gt[..., 3], gt[..., 1] + gt[..., 3]
    pos, samples, flag = np.arange(n) * 10 + 5, [f"S{i}" for i in range(S)], np.arange(n) != 2
    write_vcf(tmp_path / "a.vcf", "7", pos, h1, h2, gt, samples, pos_flag=flag)
    write_vcf(tmp_path / "a.vcf.gz", "7", pos, h1, h2, gt, samples, pos_flag=flag, bgzf=True)
    raw = (tmp_path / "a.vcf.gz").read_bytes()
    assert gzip.decompress(raw) == (tmp_path / "a.vcf").read_bytes()
    assert raw.endswith(B.EOF_BLOCK)
    blocks, used = B.bgzf_blocks(raw)
    assert used == len(raw) and blocks[-1].isize == 0
