"""The deflate corpus shared by the BGZF tests (host decoder, inflate_core.h host build, device kernel): built
with zlib at import of ``corpus()`` / ``negatives()``, no fixture files.  Every positive item is (name, data,
payload) with ``zlib.decompress(payload, -15) == data``; every negative one (name, payload, isize, crc)."""

import functools
import zlib

import numpy as np


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return co.compress(data) + co.flush()


def vcf_text(n: int, seed: int = 0) -> bytes:
    rng = np.random.default_rng(seed)
    out, pos = [], 1000
    while sum(map(len, out)) < n:
        pos += int(rng.integers(1, 900))
        cells = "\t".join(f"{a}|{b}" for a, b in (rng.random((40, 2)) < 0.2).astype(int))
        out.append(f"1\t{pos}\t.\tA\tC\t.\tPASS\t.\tGT\t{cells}\n")
    return "".join(out).encode()[:n]


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value: int, bits: int):                     # LSB first: header fields, extra bits
        self.acc |= value << self.n
        self.n += bits
        return self

    def code(self, code: int, bits: int):                     # a Huffman code: most significant bit first
        for i in range(bits - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def distance_32768(first: bytes):
    """(data, payload) built by hand, since zlib emits no distance above 32 506: 32 768 bytes in a stored block,
    then a fixed-code block with a match of 258 at distance 32 768 = pos (its source is the block's first byte),
    three literals, a match of 3 at distance 32 768 from pos 33 029, and one of 258 at distance 32 767."""
    assert len(first) == 32768
    w = BitWriter().put(0, 1).put(0, 2).put(0, 5)             # not last, stored, padding to the byte
    w.put(32768, 16).put(32768 ^ 0xffff, 16).put(int.from_bytes(first, "little"), 8 * 32768)
    w.put(1, 1).put(1, 2)                                     # last, fixed codes
    w.code(0b11000101, 8).code(29, 5).put(8191, 13)           # length 258 (symbol 285); distance code 29 + 8191 = 32 768
    for c in b"xyz":
        w.code(0x30 + c, 8)
    w.code(0b0000001, 7).code(29, 5).put(8191, 13)            # length 3 (symbol 257), distance 32 768
    w.code(0b11000101, 8).code(29, 5).put(8190, 13)           # length 258, distance 32 767
    w.code(0, 7)                                              # end of block
    out = bytearray(first)
    out += out[0:258]
    out += b"xyz"
    out += out[len(out) - 32768:len(out) - 32768 + 3]
    out += out[len(out) - 32767:len(out) - 32767 + 258]
    return bytes(out), w.bytes()


def one_code_distance_tree():
    """(data, payload) built by hand, since zlib always sends two distance codes: a dynamic block whose distance
    tree is the single one-bit code that RFC 1951 3.2.7 allows (incomplete), used by two overlapping matches.
    Literal/length code: 'a' 1 bit, 256 and 257 two bits; code-length code: 18 one bit, 1 and 2 two bits."""
    w = BitWriter().put(1, 1).put(2, 2).put(1, 5).put(0, 5).put(14, 4)        # HLIT 258, HDIST 1, HCLEN 18
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    cl = {18: 1, 1: 2, 2: 2}
    for sym in order[:18]:
        w.put(cl.get(sym, 0), 3)
    zeros = lambda n: w.code(0b0, 1).put(n - 11, 7)           # symbol 18: 11 .. 138 zeros
    zeros(97)
    w.code(0b10, 2)                                           # length 1 for 'a'
    zeros(138)
    zeros(20)                                                 # 98 .. 255
    w.code(0b11, 2).code(0b11, 2)                             # length 2 for 256 and 257
    w.code(0b10, 2)                                           # the distance tree: symbol 0, one bit
    w.code(0b0, 1)                                            # 'a'
    w.code(0b11, 2).code(0b0, 1)                              # length 3, distance 1
    w.code(0b11, 2).code(0b0, 1)
    w.code(0b10, 2)                                           # end of block
    return b"a" * 7, w.bytes()


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(7)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    text = vcf_text(65280)
    items = [
        ("stored_65280", text, deflate(text, level=0)),
        ("fixed", text[:5000], deflate(text[:5000], strategy=zlib.Z_FIXED)),
        ("dynamic_text_65280", text, deflate(text)),
        ("rle", (b"a" * 700 + b"bc" + b"\t" * 300 + text[:200]) * 3, None),
        ("huffman_only", text[:4000], deflate(text[:4000], strategy=zlib.Z_HUFFMAN_ONLY)),
        ("mem_level_1", text[:20000], deflate(text[:20000], mem_level=1)),
    ]
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    items.append(("stored_flushed", text[:7001], co.compress(text[:3000]) + co.flush(zlib.Z_FULL_FLUSH) +
                  co.compress(text[3000:7001]) + co.flush()))
    items[3] = ("rle", items[3][1], deflate(items[3][1], strategy=zlib.Z_RLE))
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    skew = np.repeat(np.arange(24, dtype=np.uint8) + 65, np.minimum(fib, 40000))
    skew = skew[rng.permutation(len(skew))][:60000].tobytes()
    items += [("fibonacci_lengths", skew, deflate(skew, strategy=zlib.Z_HUFFMAN_ONLY)),
              ("distance_32768",) + distance_32768(rand(32768)), ("one_code_distance_tree",) + one_code_distance_tree()]
    for n in (0, 1, 2, 257, 258, 259):
        d = (b"x" * n) if n in (257, 258, 259) else text[:n]
        items.append((f"size_{n}", d, deflate(d)))
        items.append((f"size_{n}_text", text[:n], deflate(text[:n])))
    small = rng.integers(0, 4, 9000, dtype=np.uint8).tobytes()
    items += [("level_1", text[:30000], deflate(text[:30000], level=1)),
              ("level_9", text[:30000], deflate(text[:30000], level=9)),
              ("filtered", text[:9000], deflate(text[:9000], strategy=zlib.Z_FILTERED)),
              ("fixed_run_258", b"x" * 258, deflate(b"x" * 258, strategy=zlib.Z_FIXED)),
              ("rle_run_65280", b"a" * 65280, deflate(b"a" * 65280, strategy=zlib.Z_RLE)),
              ("huffman_only_1", b"q", deflate(b"q", strategy=zlib.Z_HUFFMAN_ONLY)),
              ("four_symbols", small, deflate(small)),
              ("four_symbols_fixed", small, deflate(small, strategy=zlib.Z_FIXED)),
              ("random_3000", r3 := rand(3000), deflate(r3)),
              ("stored_1", b"z", deflate(b"z", level=0))]
    r = rand(65280)
    items.append(("random_65280", r, deflate(r)))
    for name, data, payload in items:
        assert zlib.decompress(payload, -15) == data, name
    return tuple(items)


def short_dynamic():
    data = vcf_text(600, seed=3)
    payload = deflate(data)
    assert (payload[0] >> 1) & 3 == 2
    return data, payload


@functools.lru_cache(maxsize=None)
def negatives():
    """(name, payload, isize, crc, status): status None where the specification decides (6 or 8)."""
    out = []
    crc = zlib.crc32
    out.append(("reserved_type", b"\x07", 0, 0, 1))
    lit = b"stored literal bytes\n" * 10
    st = deflate(lit, level=0)
    assert st[0] & 7 == 1 and st[1:3] == len(lit).to_bytes(2, "little")
    out.append(("nlen_flipped", st[:3] + bytes([st[3] ^ 1]) + st[4:], len(lit), crc(lit), 2))
    w = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        w.put(1, 3)                                           # nineteen codes of one bit
    out.append(("oversubscribed", w.bytes() + b"\0" * 8, 10, 0, 3))
    out.append(("symbol_286", BitWriter().put(1, 1).put(1, 2).code(0b11000110, 8).bytes() + b"\0\0", 4, 0, 4))
    out.append(("distance_before_start", BitWriter().put(1, 1).put(1, 2).code(0b0000001, 7).code(0, 5).bytes() + b"\0\0",
                3, 0, 5))
    data, payload = short_dynamic()
    out.append(("isize_minus_1", payload, len(data) - 1, crc(data), 7))
    out.append(("isize_plus_1", payload, len(data) + 1, crc(data), 8))
    for cut in range(0, len(payload), 8):
        out.append((f"cut_{cut}", payload[:cut], len(data), crc(data), None))
    flipped = bytearray(st)
    flipped[5 + 7] ^= 0x10                                    # one bit of one literal of the stored block
    out.append(("crc_flip", bytes(flipped), len(lit), crc(lit), 9))
    return tuple(out)
