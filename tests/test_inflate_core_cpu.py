"""csrc/inflate_core.h — the decoder text the device kernel compiles — built as a plain host program
(tests/inflate_core_main.cc), once as it is and once under AddressSanitizer + UBSan, and run over the
deflate corpus, the broken streams and 2 000 payloads of random bytes.  Status and CRC must equal the
specification's (src/dataset/bgzf.py inflate_block_host), and the sanitised run must end clean: this is where
the decoder's bounds are checked, on the CPU, for any bytes whatever."""

import shutil
import struct
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from src.dataset import bgzf as B  # noqa: E402
from bgzf_corpus import corpus, negatives, short_dynamic  # noqa: E402

CXX = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)


def random_cases(n=2000, seed=11):
    """Random bytes with random isize; a third begin with a valid dynamic header so the walk gets past it."""
    rng = np.random.default_rng(seed)
    _, dyn = short_dynamic()
    out = []
    for i in range(n):
        ln = int(rng.integers(0, 400))
        p = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        if i % 3 == 1:
            p = dyn[:int(rng.integers(1, len(dyn)))] + p
        elif i % 3 == 2 and ln:
            p = bytes([p[0] & 0xf8 | int(rng.integers(0, 2)) | 2]) + p[1:]        # a fixed-code block
        out.append((p, int(rng.integers(0, 3000))))
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("blocks")
    items = [(payload, len(data)) for _, data, payload in corpus()]
    items += [(payload, isize) for _, payload, isize, _, _ in negatives()]
    items += random_cases()
    for i, (payload, isize) in enumerate(items):
        (d / f"{i:06d}.bin").write_bytes(struct.pack("<I", isize) + payload)
    want = []
    for payload, isize in items:
        data, st = B.inflate_block_host(payload, isize)
        want.append((st, zlib.crc32(data) if st == B.OK else 0))
    return d, want


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_specification(tmp_path, cases, flags):
    assert CXX, "no host C++ compiler (g++, c++, clang++): the decoder's bounds cannot be checked"
    d, want = cases
    exe = tmp_path / "inflate_core_main"
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, "-I", str(REPO / "rag-snvbert_amd" / "csrc"),
                    str(REPO / "tests" / "inflate_core_main.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    got = [(int(f[1]), int(f[2], 16)) for f in (line.split() for line in r.stdout.splitlines())]
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:10]
    seen = {st for st, _ in want}
    assert seen >= set(range(9)), seen                      # every decoder status occurs (9 is the CRC's)
