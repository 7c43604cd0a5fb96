"""BGZF (blocked gzip, the container of ``.vcf.gz`` as bgzip / htslib write it) on the host: the member walk,
a writer, and the specification of the device inflate.

A BGZF file is a sequence of gzip members of at most 64 KiB, none of which refers back into another.  Each
carries its own size in the header (extra subfield ``BC``, ``BSIZE`` = member bytes - 1) and its inflated size
and CRC-32 in the trailer, so the host lays out every block's input and output range from the headers alone
and ``csrc/inflate.hip`` inflates them side by side.  Layout of a member: 12 bytes of gzip header with
``FLG.FEXTRA``, ``XLEN`` bytes of extra field, the deflate payload (``BSIZE + 1 - XLEN - 20`` bytes), ``CRC32``,
``ISIZE``.

``inflate_block_host`` is the specification of the kernel and of ``csrc/inflate_core.h``: a plain RFC 1951
decoder that returns ``(bytes, status)`` and never raises.  The first condition met in stream order wins:

  0  ok
  1  reserved block type
  2  stored LEN / NLEN mismatch
  3  bad code-length set: HLIT > 286 or HDIST > 30; an oversubscribed code; an incomplete one, other than a
     distance code of at most one code, that of one bit (RFC 1951 3.2.7); a repeat with no previous length; a
     repeat that runs past HLIT + HDIST; no code for the end-of-block symbol
  4  invalid symbol (literal/length 286-287, distance 30-31, or bits that no code of such a distance tree matches)
  5  distance reaches in front of the block's output
  6  input exhausted (the bit position passed 8 * len(payload))
  7  output would pass ISIZE
  8  stream ended short of ISIZE
  9  CRC mismatch (``inflate_member_host``; the decoder itself knows no CRC)
"""

from __future__ import annotations

import struct
import zlib
from typing import List, NamedTuple, Tuple

OK, BAD_TYPE, BAD_STORED, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, INPUT_END, OUTPUT_FULL, OUTPUT_SHORT, BAD_CRC = range(10)
STATUS_TEXT = {
    BAD_TYPE: "reserved deflate block type",
    BAD_STORED: "stored block LEN / NLEN mismatch",
    BAD_LENGTHS: "bad code-length set",
    BAD_SYMBOL: "invalid symbol",
    BAD_DISTANCE: "distance reaches in front of the block",
    INPUT_END: "compressed data exhausted",
    OUTPUT_FULL: "output would pass ISIZE",
    OUTPUT_SHORT: "stream ended short of ISIZE",
    BAD_CRC: "CRC mismatch",
}
MAX_ISIZE = 65536
MAX_BLOCK = 65536                     # BSIZE + 1
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Block(NamedTuple):
    file_off: int        # of the member's first byte (``base`` + its offset in the buffer)
    payload_off: int     # of the deflate payload, in the buffer
    payload_len: int
    isize: int
    crc: int


def bgzf_blocks(buf, base: int = 0) -> Tuple[List[Block], int]:
    """(whole blocks of the bytes-like ``buf``, bytes consumed): a trailing partial block stays for the next
    read.  ``base`` is the file offset of ``buf[0]``, for the ``ValueError`` that a broken header raises."""
    mv = memoryview(buf).cast("B")
    n, o, out = len(mv), 0, []
    while n - o >= 12:
        if not (mv[o] == 0x1f and mv[o + 1] == 0x8b and mv[o + 2] == 8):
            raise ValueError(f"BGZF block at byte {base + o}: not a gzip member (magic 1f 8b 08)")
        if not mv[o + 3] & 4:
            raise ValueError(f"BGZF block at byte {base + o}: no extra field (FLG.FEXTRA)")
        xlen = mv[o + 10] | mv[o + 11] << 8
        if n - o < 12 + xlen:
            break
        q, end, bsize = o + 12, o + 12 + xlen, -1
        while q + 4 <= end:
            slen = mv[q + 2] | mv[q + 3] << 8
            if q + 4 + slen > end:
                break
            if mv[q] == 66 and mv[q + 1] == 67 and slen == 2:
                bsize = mv[q + 4] | mv[q + 5] << 8
                break
            q += 4 + slen
        if bsize < 0:
            raise ValueError(f"BGZF block at byte {base + o}: no BC subfield in the extra field")
        plen = bsize + 1 - xlen - 20
        if plen < 0:
            raise ValueError(f"BGZF block at byte {base + o}: BSIZE {bsize} is smaller than the member's frame")
        if n - o < bsize + 1:
            break
        t = o + bsize + 1 - 8
        crc, isize = struct.unpack_from("<II", mv, t)
        if isize > MAX_ISIZE:
            raise ValueError(f"BGZF block at byte {base + o}: ISIZE {isize} exceeds 65536")
        out.append(Block(base + o, o + 12 + xlen, plen, isize, crc))
        o += bsize + 1
    return out, o


def is_bgzf(path) -> bool:
    """The first gzip member of the file carries the ``BC`` subfield."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:3] != b"\x1f\x8b\x08" or not head[3] & 4:
            return False
        xlen = head[10] | head[11] << 8
        extra = f.read(xlen)
    q = 0
    while q + 4 <= len(extra):
        slen = extra[q + 2] | extra[q + 3] << 8
        if extra[q:q + 2] == b"BC" and slen == 2 and q + 6 <= len(extra):
            return True
        q += 4 + slen
    return False


def bgzf_member(data: bytes, level: int = 6, strategy: int = 0, mem_level: int = 8) -> bytes:
    """One BGZF member holding ``data`` (at most 65 536 bytes)."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    payload = co.compress(data) + co.flush()
    bsize = len(payload) + 25
    assert bsize + 1 <= MAX_BLOCK, f"a block of {len(data)} bytes deflates to {len(payload)}: BSIZE would pass 65536"
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + payload +
            struct.pack("<II", zlib.crc32(data), len(data)))


def write_bgzf(path_or_fh, data, block_size: int = 0xff00, level: int = 6, strategy: int = 0, mem_level: int = 8,
               eof: bool = True) -> None:
    """``data`` as BGZF: members of ``block_size`` input bytes each, then the 28-byte EOF block."""
    assert 1 <= block_size <= MAX_ISIZE
    mv = memoryview(data).cast("B")
    fh = open(path_or_fh, "wb") if not hasattr(path_or_fh, "write") else path_or_fh
    try:
        for o in range(0, len(mv), block_size):
            fh.write(bgzf_member(bytes(mv[o:o + block_size]), level, strategy, mem_level))
        if eof:
            fh.write(EOF_BLOCK)
    finally:
        if fh is not path_or_fh:
            fh.close()


class BgzfWriter:
    """A write-only file object that buffers ``block_size`` bytes per member (``write_gt_vcf(bgzf=True)``)."""

    def __init__(self, path, block_size: int = 0xff00, level: int = 6):
        self.fh, self.block_size, self.level, self.buf = open(path, "wb"), block_size, level, bytearray()
        self.eof_virtual = None

    def write(self, data) -> int:
        self.buf += data
        while len(self.buf) >= self.block_size:
            self.fh.write(bgzf_member(bytes(self.buf[:self.block_size]), self.level))
            del self.buf[:self.block_size]
        return len(data)

    def tell_virtual(self) -> int:
        """The virtual offset of the next byte written: the file offset of the member being filled ``<< 16`` and
        the bytes buffered in it (fewer than ``block_size``: a full member has left, so a position on a member
        boundary has offset 0 in the later member).  After ``close``: the EOF block's offset ``<< 16``."""
        return self.fh.tell() << 16 | len(self.buf) if self.eof_virtual is None else self.eof_virtual

    def close(self) -> None:
        if self.buf:
            self.fh.write(bgzf_member(bytes(self.buf), self.level))
            self.buf = bytearray()
        self.eof_virtual = self.fh.tell() << 16
        self.fh.write(EOF_BLOCK)
        self.fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def deflate_device(data, block_size: int = 0xff00, device=None) -> bytes:
    """The BGZF members of the bytes-like ``data``, ``block_size`` input bytes each, deflated and packed on the
    GPU (csrc/deflate.hip; the compressor is csrc/deflate_core.h), without the EOF block.  The bytes depend on
    ``data`` and ``block_size`` alone."""
    import numpy as np
    import torch
    from .. import kernels as K
    if not 1 <= block_size <= 0xff00:
        raise ValueError(f"deflate_device: block_size {block_size} must lie in [1, 0xff00]")
    mv = memoryview(data).cast("B")
    if len(mv) == 0:
        return b""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        text = torch.from_numpy(np.frombuffer(mv, np.uint8).copy()).to(dev)
        members, member_len = K.bgzf_deflate(text, len(mv), block_size)
        out = torch.empty(len(mv) + 31 * members.shape[0], device=dev, dtype=torch.uint8)   # a member adds at most 31
        total = int(K.bgzf_pack(members, member_len, out).item())
        if total < 0:
            raise RuntimeError("deflate_device: the members exceed their bound")
        return out[:total].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------- the specification --
class _Bits:
    """LSB-first bits of ``data``; bits past its end read as zero, ``over()`` once the position passed it."""

    def __init__(self, data: bytes):
        self.n, self.d, self.pos = len(data), data + b"\0\0\0\0", 0

    def get(self, k: int) -> int:
        i, s = self.pos >> 3, self.pos & 7
        self.pos += k
        if i >= self.n:
            return 0
        d = self.d
        return ((d[i] | d[i + 1] << 8 | d[i + 2] << 16) >> s) & ((1 << k) - 1)

    def over(self) -> bool:
        return self.pos > 8 * self.n


def _build(lengths):
    """(count[16], symbols in code order, left): left < 0 oversubscribed, 0 complete, > 0 incomplete."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    left = 1
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            return count, [], left
    symbol = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]
    return count, symbol, left


def _decode(b: _Bits, count, symbol) -> int:
    """One symbol by the canonical walk; -1 when 15 bits match no code."""
    code = first = index = 0
    for l in range(1, 16):
        code |= b.get(1)
        c = count[l]
        if code - c < first:
            return symbol[index + (code - first)]
        index += c
        first = (first + c) << 1
        code <<= 1
    return -1


def _len_base(s):
    return 3 + s if s < 8 else 258 if s == 28 else 3 + ((4 + (s & 3)) << ((s >> 2) - 1))


def _len_extra(s):
    return 0 if s < 8 or s == 28 else (s >> 2) - 1


def _dist_base(s):
    return 1 + s if s < 4 else 1 + ((2 + (s & 1)) << ((s >> 1) - 1))


def _dist_extra(s):
    return 0 if s < 4 else (s >> 1) - 1


_FIXED = (_build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _build([5] * 30))


def _dynamic(b: _Bits, trace=None):
    nlen, ndist, ncode = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    if b.over():
        return INPUT_END, None, None
    if nlen > 286 or ndist > 30:
        return BAD_LENGTHS, None, None
    cl = [0] * 19
    for i in range(ncode):
        cl[_ORDER[i]] = b.get(3)
    if b.over():
        return INPUT_END, None, None
    ccount, csym, left = _build(cl)
    if left != 0:
        return BAD_LENGTHS, None, None
    lengths: List[int] = []
    while len(lengths) < nlen + ndist:
        sym = _decode(b, ccount, csym)
        if b.over():
            return INPUT_END, None, None
        if sym < 0:
            return BAD_LENGTHS, None, None
        if sym < 16:
            lengths.append(sym)
            continue
        prev = 0
        if sym == 16:
            if not lengths:
                return BAD_LENGTHS, None, None
            prev, rep = lengths[-1], 3 + b.get(2)
        elif sym == 17:
            rep = 3 + b.get(3)
        else:
            rep = 11 + b.get(7)
        if b.over():
            return INPUT_END, None, None
        if len(lengths) + rep > nlen + ndist:
            return BAD_LENGTHS, None, None
        lengths += [prev] * rep
    if lengths[256] == 0:
        return BAD_LENGTHS, None, None
    lcount, lsym, left = _build(lengths[:nlen])
    if left != 0:
        return BAD_LENGTHS, None, None
    dcount, dsym, left = _build(lengths[nlen:])
    if left < 0 or (left > 0 and dcount[0] + dcount[1] != ndist):
        return BAD_LENGTHS, None, None
    if trace is not None:
        trace["max_code_length"] = max(trace.get("max_code_length", 0), max(lengths))
        trace["incomplete_distance_trees"] = trace.get("incomplete_distance_trees", 0) + (left > 0)
    return OK, (lcount, lsym), (dcount, dsym)


def inflate_block_host(payload, isize: int, trace: dict = None) -> Tuple[bytes, int]:
    """(bytes produced, status) of the raw deflate stream ``payload`` that must inflate to exactly ``isize``
    bytes.  Never raises; the bytes of a failed block are what was produced up to the failure.  ``trace`` (a
    dict) collects what the stream exercised: ``block_types`` (list), ``matches`` [(pos, distance, length)],
    ``max_code_length`` of the dynamic codes, ``incomplete_distance_trees``."""
    payload = bytes(payload)
    if trace is not None:
        trace.setdefault("block_types", [])
        trace.setdefault("matches", [])
    n, out, base = len(payload), bytearray(), 0
    b = _Bits(payload)
    while True:
        last, typ = b.get(1), b.get(2)
        if b.over():
            return bytes(out), INPUT_END
        if typ == 3:
            return bytes(out), BAD_TYPE
        if trace is not None:
            trace["block_types"].append(typ)
        if typ == 0:
            at = base + ((b.pos + 7) >> 3)
            if at + 4 > n:
                return bytes(out), INPUT_END
            ln, nln = payload[at] | payload[at + 1] << 8, payload[at + 2] | payload[at + 3] << 8
            if ln != (~nln & 0xffff):
                return bytes(out), BAD_STORED
            have, room = n - (at + 4), isize - len(out)
            if ln > have and have < room:                      # bytes in stream order: the input ends first
                return bytes(out), INPUT_END
            if ln > room:
                return bytes(out), OUTPUT_FULL
            out += payload[at + 4:at + 4 + ln]
            base = at + 4 + ln
            b = _Bits(payload[base:])
        else:
            if typ == 1:
                (lcount, lsym, _), (dcount, dsym, _) = _FIXED
            else:
                st, lc, dc = _dynamic(b, trace)
                if st != OK:
                    return bytes(out), st
                (lcount, lsym), (dcount, dsym) = lc, dc
            while True:
                sym = _decode(b, lcount, lsym)
                if b.over():
                    return bytes(out), INPUT_END
                if sym < 0:
                    return bytes(out), BAD_SYMBOL
                if sym < 256:
                    if len(out) >= isize:
                        return bytes(out), OUTPUT_FULL
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                sym -= 257
                if sym >= 29:
                    return bytes(out), BAD_SYMBOL
                ln = _len_base(sym) + b.get(_len_extra(sym))
                if b.over():
                    return bytes(out), INPUT_END
                ds = _decode(b, dcount, dsym)
                if b.over():
                    return bytes(out), INPUT_END
                if ds < 0 or ds >= 30:
                    return bytes(out), BAD_SYMBOL
                dist = _dist_base(ds) + b.get(_dist_extra(ds))
                if b.over():
                    return bytes(out), INPUT_END
                if dist > len(out):
                    return bytes(out), BAD_DISTANCE
                if len(out) + ln > isize:
                    return bytes(out), OUTPUT_FULL
                if trace is not None:
                    trace["matches"].append((len(out), dist, ln))
                start = len(out) - dist
                if dist >= ln:
                    out += out[start:start + ln]
                else:
                    for i in range(ln):                        # the run-length case, byte by byte
                        out.append(out[start + i])
        if last:
            break
    return bytes(out), (OK if len(out) == isize else OUTPUT_SHORT)


def inflate_member_host(payload, isize: int, crc: int) -> Tuple[bytes, int]:
    """``inflate_block_host`` with the member's CRC-32 checked behind it: status 9 where the block inflated
    and its checksum differs."""
    data, st = inflate_block_host(payload, isize)
    if st == OK and zlib.crc32(data) != (crc & 0xffffffff):
        st = BAD_CRC
    return data, st
