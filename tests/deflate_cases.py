"""Inputs shared by the deflate tests (csrc/deflate_core.h host build, device kernel): built at call time, no
fixture files.  ``member_inputs()`` is an ordered dict name -> data of at most 0xff00 bytes."""

import functools
import sys
import zlib
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from src.dataset import bgzf as B  # noqa: E402
from bgzf_corpus import corpus, vcf_text  # noqa: E402

MAX_IN = 0xff00


def core_T() -> int:
    """DEFL_T as the header states it."""
    import re
    text = (REPO / "rag-snvbert_amd" / "csrc" / "deflate_core.h").read_text()
    return int(re.search(r"constexpr int DEFL_T = (\d+);", text).group(1))


def window_pair(gap: int, seed: int = 5) -> bytes:
    """A 300-byte random segment (bytes 2 .. 255), random filler of the bytes 0 and 1 (so that the filler's
    three-byte groups leave the segment's hash heads alone), then the segment again, beginning exactly ``gap``
    bytes after the first."""
    rng = np.random.default_rng(seed)
    seg = rng.integers(2, 256, 300, dtype=np.uint8).tobytes()
    fill = rng.integers(0, 2, gap - 300, dtype=np.uint8).tobytes()
    return seg + fill + seg


def cell_text(confident: float, lines: int = 60, samples: int = 500, seed: int = 3) -> bytes:
    """Records with the writer's exact cells (``vcf_cells``); ``confident`` is the share of cells whose
    probabilities are 0 or 1."""
    from src.infer_embedding_rag import vcf_cells
    rng = np.random.default_rng(seed)
    out = []
    for i in range(lines):
        gt = rng.dirichlet(np.ones(4), samples).astype(np.float32)
        sure = rng.random(samples) < confident
        cls = rng.choice(4, samples, p=[0.8, 0.08, 0.08, 0.04])
        gt[sure] = np.eye(4, dtype=np.float32)[cls[sure]]
        h1, h2 = gt[:, 2] + gt[:, 3], gt[:, 1] + gt[:, 3]
        out.append(f"1\t{1000 + 37 * i}\t.\t.\t.\t0.0\tPASS\t.\tGT:HDS:GP:DS\t" + "\t".join(vcf_cells(h1, h2, gt)) + "\n")
    return "".join(out).encode()


def zlib_members(data: bytes, level: int, strategy: int = zlib.Z_DEFAULT_STRATEGY, block_size: int = MAX_IN) -> int:
    """Total bytes of zlib's BGZF members of ``data`` at the same member size."""
    return sum(len(B.bgzf_member(data[o:o + block_size], level, strategy)) for o in range(0, len(data), block_size))


def random_inputs(n: int = 2000, seed: int = 17):
    """0 to 3 000 bytes each; every third one from a 4-symbol alphabet, so that matches occur."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(0, 3001))
        hi = 4 if i % 3 == 0 else 256
        out.append(rng.integers(0, hi, ln, dtype=np.uint8).tobytes())
    return out


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """(name, data): the corpus, the edge lengths, zeros, random bytes, VCF text and the window pair."""
    rng = np.random.default_rng(23)
    t = core_T()
    items = [(f"corpus_{name}", data[:MAX_IN]) for name, data, _ in corpus()]
    text = vcf_text(MAX_IN, seed=4)
    for ln in (0, 1, 2, 3, 4, 257, 258, 259, 260, t - 1, t, t + 1):
        items.append((f"len_{ln}", text[:ln]))
        items.append((f"zeros_{ln}", bytes(ln)))
    items.append(("zeros_ff00", bytes(MAX_IN)))
    items.append(("random_ff00", rng.integers(0, 256, MAX_IN, dtype=np.uint8).tobytes()))
    items.append(("vcf_ff00", text))
    items.append(("vcf_20000", vcf_text(20000, seed=9)))
    items.append(("cells_ff00", cell_text(0.9, lines=4)[:MAX_IN]))
    items.append(("window_32768", window_pair(32768)))
    items.append(("window_32769", window_pair(32769)))
    return tuple(items)


def member_inputs(with_random: bool = True):
    items = list(edge_inputs())
    if with_random:
        items += [(f"rnd_{i:04d}", d) for i, d in enumerate(random_inputs())]
    return {f"{i:05d}_{name}": data for i, (name, data) in enumerate(items)}


def check_member(member: bytes, data: bytes) -> None:
    """One whole BGZF member of at most 65 536 bytes that zlib inflates to ``data``."""
    assert len(member) <= 65536
    blocks, used = B.bgzf_blocks(member)
    assert used == len(member) and len(blocks) == 1, (used, len(member), len(blocks))
    assert blocks[0].isize == len(data) and blocks[0].crc == zlib.crc32(data)
    assert zlib.decompress(member, 31) == data
