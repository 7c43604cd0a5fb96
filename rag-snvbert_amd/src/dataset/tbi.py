"""Tabix (``.tbi``) indexes of bgzipped VCF files on the host: the format, one canonical construction, the
specification for a file on disk, and the query the region reads use.  numpy only, no GPU.

The tabix specification (TBI: ``min_shift`` 14, depth 5, coordinates below 2^29) on 0-based half-open
intervals.  A record of a VCF covers ``[POS - 1, POS - 1 + len(REF))``.  Bins: level l (0..5) holds
``8^l`` bins of ``2^(29 - 3 l)`` bases, numbered from ``(8^l - 1) / 7``; a record goes into the smallest bin
that contains it.  The linear index holds one virtual offset per 16 384-base window.

A virtual offset is ``file offset of a BGZF member << 16 | offset inside the member's text``.  The canonical
mapping of a text position (``virtual_offsets``): the member that holds that byte, so a position on a member
boundary has offset 0 in the later member and never ISIZE in the earlier one; the position behind the last
byte of the text is the EOF block's offset ``<< 16``.

``build`` is the one construction (both VCF writers and ``index_vcf_bgzf`` call it): a chunk per maximal run
of consecutive records of one sequence in one bin, not merged further; ``ioff[w]`` the smallest ``v_beg`` of
the records that overlap window w, a window without a record taking the value of the window before it,
leading windows 0; the pseudo-bin 37450 as htslib writes it ((first ``v_beg``, last ``v_end``), (record
count, 0)).  Bins are written in increasing order.

Layout of the file (little-endian, the whole of it BGZF-compressed and ended by the EOF block): magic
``TBI\\1``, n_ref, format (2 = VCF), col_seq, col_beg, col_end, meta, skip, l_nm, the names with their NULs;
per sequence n_bin, then per bin (bin u32, n_chunk i32, n_chunk x (cnk_beg u64, cnk_end u64)), n_intv, n_intv
x ioff u64; a trailing n_no_coor u64.

Not covered: ``.csi``, formats other than VCF, an indexer on the device for files this project did not write
(``index_vcf_bgzf`` is slow and meant as the specification)."""

from __future__ import annotations

import gzip
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAGIC = b"TBI\x01"
MIN_SHIFT, DEPTH = 14, 5
BIN_LIMIT = 1 << 29
PSEUDO_BIN = 37450                                   # ((1 << 18) - 1) / 7 + 1: one past the last real bin
FORMAT_VCF = 2
_LEVELS = ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1))      # (shift, first bin) from the finest level up


def reg2bin(beg: int, end: int) -> int:
    """The smallest bin that contains [beg, end)."""
    end -= 1
    for shift, first in _LEVELS:
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg: int, end: int) -> List[int]:
    """Every bin that can hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in reversed(_LEVELS):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def _bins_of(beg: np.ndarray, end: np.ndarray) -> np.ndarray:
    """``reg2bin`` of every interval (int64 arrays)."""
    last = end - 1
    out = np.zeros(beg.shape, np.int64)
    done = np.zeros(beg.shape, bool)
    for shift, first in _LEVELS:
        hit = ~done & (beg >> shift == last >> shift)
        out[hit] = first + (beg[hit] >> shift)
        done |= hit
    return out


class TabixIndex:
    """``names`` [n_ref]; per sequence ``bins[i]`` {bin: [(cnk_beg, cnk_end), ...]} (the pseudo-bin among
    them when the file holds it) and ``ioff[i]`` u64 [n_intv]; the header fields of a VCF index."""

    def __init__(self, names: Sequence[str], bins: Sequence[Dict[int, List[Tuple[int, int]]]], ioff: Sequence,
                 format: int = FORMAT_VCF, col_seq: int = 1, col_beg: int = 2, col_end: int = 0, meta: str = "#",
                 skip: int = 0, n_no_coor: int = 0):
        self.names = [str(n) for n in names]
        self.bins = [{int(b): [(int(lo), int(hi)) for lo, hi in c] for b, c in d.items()} for d in bins]
        self.ioff = [np.asarray(a, np.uint64).reshape(-1) for a in ioff]
        assert len(self.names) == len(self.bins) == len(self.ioff)
        self.format, self.col_seq, self.col_beg, self.col_end = format, col_seq, col_beg, col_end
        self.meta, self.skip, self.n_no_coor = meta, skip, n_no_coor

    def _fields(self):
        return (self.names, self.bins, self.format, self.col_seq, self.col_beg, self.col_end, self.meta, self.skip,
                self.n_no_coor)

    def __eq__(self, other):
        return (isinstance(other, TabixIndex) and self._fields() == other._fields() and
                all(np.array_equal(a, b) for a, b in zip(self.ioff, other.ioff)))

    def __repr__(self):
        return (f"TabixIndex({len(self.names)} sequences, "
                f"{sum(len(c) for d in self.bins for c in d.values())} chunks)")

    def to_bytes(self, pseudo_bin: bool = True, n_no_coor: bool = True) -> bytes:
        """The uncompressed layout.  ``pseudo_bin`` / ``n_no_coor`` False leave those optional parts out (the
        files of older tools)."""
        names = b"".join(n.encode() + b"\0" for n in self.names)
        out = [MAGIC, struct.pack("<8i", len(self.names), self.format, self.col_seq, self.col_beg, self.col_end,
                                  ord(self.meta), self.skip, len(names)), names]
        for bins, ioff in zip(self.bins, self.ioff):
            keep = sorted(b for b in bins if pseudo_bin or b != PSEUDO_BIN)
            out.append(struct.pack("<i", len(keep)))
            for b in keep:
                out.append(struct.pack("<Ii", b, len(bins[b])))
                out.append(np.asarray(bins[b], np.uint64).reshape(-1).astype("<u8").tobytes())
            out.append(struct.pack("<i", len(ioff)))
            out.append(ioff.astype("<u8").tobytes())
        if n_no_coor:
            out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)

    def write(self, path) -> None:
        """``to_bytes()`` as a BGZF file with the EOF block."""
        from .bgzf import write_bgzf
        write_bgzf(path, self.to_bytes())


def read(path) -> TabixIndex:
    """The index at ``path``, with or without the pseudo-bin and the trailing n_no_coor.  ``ValueError`` naming
    the path: not gzip, a wrong magic, a format other than VCF, a truncated body."""
    name = str(path)
    with open(path, "rb") as f:
        raw = f.read()
    try:
        data = gzip.decompress(raw)
    except (OSError, EOFError, zlib.error) as e:
        raise ValueError(f"{name}: not a BGZF-compressed tabix index ({e})") from None
    if data[:4] != MAGIC:
        raise ValueError(f"{name}: not a tabix index (magic {data[:4]!r}, expected {MAGIC!r})")
    o = 4

    def take(fmt):
        nonlocal o
        size = struct.calcsize(fmt)
        if o + size > len(data):
            raise ValueError(f"{name}: truncated tabix index ({len(data)} bytes, {fmt!r} wanted at byte {o})")
        v = struct.unpack_from(fmt, data, o)
        o += size
        return v

    def take_u64(n):
        nonlocal o
        if n < 0 or o + 8 * n > len(data):
            raise ValueError(f"{name}: truncated tabix index ({len(data)} bytes, {n} offsets wanted at byte {o})")
        a = np.frombuffer(data, "<u8", n, o).astype(np.uint64)
        o += 8 * n
        return a

    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = take("<8i")
    if fmt != FORMAT_VCF:
        raise ValueError(f"{name}: the index is of format {fmt}, not of a VCF (2)")
    if n_ref < 0 or l_nm < 0 or o + l_nm > len(data):
        raise ValueError(f"{name}: truncated tabix index ({len(data)} bytes, {l_nm} bytes of names wanted at byte {o})")
    names = data[o:o + l_nm].split(b"\0")[:-1]
    o += l_nm
    if len(names) != n_ref:
        raise ValueError(f"{name}: the index names {len(names)} sequences, its header says {n_ref}")
    bins, ioff = [], []
    for _ in range(n_ref):
        d = {}
        for _ in range(take("<i")[0]):
            b, n_chunk = take("<Ii")
            c = take_u64(2 * n_chunk)
            d[b] = [(int(lo), int(hi)) for lo, hi in zip(c[0::2].tolist(), c[1::2].tolist())]
        bins.append(d)
        ioff.append(take_u64(take("<i")[0]))
    n_no_coor = take("<Q")[0] if o < len(data) else 0
    return TabixIndex([n.decode() for n in names], bins, ioff, fmt, col_seq, col_beg, col_end, chr(meta), skip, n_no_coor)


def record_intervals(pos, ref_len) -> Tuple[np.ndarray, np.ndarray]:
    """(beg, end) int64 of records with 1-based ``pos`` and REF lengths ``ref_len``.  ``ValueError`` naming the
    record where POS is not in [1, 2^29) or the record ends behind 2^29: a ``.tbi`` cannot hold it."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    beg = pos - 1
    end = beg + np.maximum(np.asarray(ref_len, np.int64).reshape(-1), 1)
    bad = np.flatnonzero((pos < 1) | (pos >= BIN_LIMIT) | (end > BIN_LIMIT))
    if bad.size:
        r = int(bad[0])
        raise ValueError(f"record {r}: POS {int(pos[r])} (end {int(end[r])}) lies outside [1, 2^29): a .tbi index "
                         "cannot hold it")
    return beg, end


def vcf_intervals(pos, pos_flag=None, ref=None) -> Tuple[np.ndarray, np.ndarray]:
    """``record_intervals`` of the site rows the VCF writers select (``pos_flag``; all without it), REF being
    '.' without ``ref``.  The record numbers of an error count the selected rows."""
    sel = np.arange(len(pos)) if pos_flag is None else np.flatnonzero(np.asarray(pos_flag))
    ref_len = np.ones(sel.size, np.int64) if ref is None else np.asarray([len(str(ref[i])) for i in sel], np.int64)
    return record_intervals(np.asarray(pos)[sel], ref_len)


def virtual_offsets(text_pos, member_off, member_isize, end_off: int) -> np.ndarray:
    """u64 virtual offsets of the text positions ``text_pos`` of a BGZF file whose members begin at the file
    offsets ``member_off`` and hold ``member_isize`` bytes of text each: a prefix sum over the sizes and a
    search.  A position behind the last byte gives ``end_off << 16`` (the EOF block, or what follows)."""
    t = np.asarray(text_pos, np.int64).reshape(-1)
    off = np.asarray(member_off, np.int64).reshape(-1)
    ends = np.cumsum(np.asarray(member_isize, np.int64).reshape(-1))
    if not ends.size:
        return np.full(t.shape, int(end_off) << 16, np.uint64)
    m = np.searchsorted(ends, t, side="right")           # the first member that ends behind t: empty ones are passed
    mm = np.minimum(m, ends.size - 1)
    starts = ends - np.asarray(member_isize, np.int64).reshape(-1)
    v = np.where(m < ends.size, off[mm] << 16 | (t - starts[mm]), int(end_off) << 16)
    return v.astype(np.uint64)


def build(names, seq_id, beg, end, v_beg, v_end) -> TabixIndex:
    """The index of records given in file order: ``seq_id`` into ``names``, the 0-based ``[beg, end)``, and the
    virtual offsets of each record's first byte and of the byte behind its newline.  ``ValueError`` naming the
    record: the records of a sequence are not contiguous, positions decrease inside a sequence, end > 2^29."""
    names = [str(n) for n in names]
    seq = np.asarray(seq_id, np.int64).reshape(-1)
    beg, end = np.asarray(beg, np.int64).reshape(-1), np.asarray(end, np.int64).reshape(-1)
    vb, ve = np.asarray(v_beg, np.uint64).reshape(-1), np.asarray(v_end, np.uint64).reshape(-1)
    n = seq.size
    assert beg.size == end.size == vb.size == ve.size == n
    bins: List[Dict[int, List[Tuple[int, int]]]] = [{} for _ in names]
    ioff = [np.zeros(0, np.uint64) for _ in names]
    if n == 0:
        return TabixIndex(names, bins, ioff)
    what = lambda r: f"record {r} ({names[int(seq[r])]}:{int(beg[r]) + 1})"
    if seq.min() < 0 or seq.max() >= len(names):
        raise ValueError(f"record {int(np.flatnonzero((seq < 0) | (seq >= len(names)))[0])}: a sequence id outside the names")
    bad = np.flatnonzero((end > BIN_LIMIT) | (beg < 0))
    if bad.size:
        raise ValueError(f"{what(int(bad[0]))}: the record ends at {int(end[bad[0]])}, beyond 2^29: a .tbi index "
                         "cannot hold it")
    end = np.maximum(end, beg + 1)
    first = np.concatenate([[0], np.flatnonzero(seq[1:] != seq[:-1]) + 1])      # the first record of every sequence run
    seen = set()
    for r in first.tolist():
        if int(seq[r]) in seen:
            raise ValueError(f"{what(r)}: the records of sequence {names[int(seq[r])]} are not contiguous")
        seen.add(int(seq[r]))
    down = np.flatnonzero((beg[1:] < beg[:-1]) & (seq[1:] == seq[:-1]))
    if down.size:
        r = int(down[0]) + 1
        raise ValueError(f"{what(r)}: the position lies in front of the previous record's ({int(beg[r - 1]) + 1})")
    rbin = _bins_of(beg, end)
    run = np.concatenate([[0], np.flatnonzero((seq[1:] != seq[:-1]) | (rbin[1:] != rbin[:-1])) + 1, [n]])
    for a, b in zip(run[:-1].tolist(), run[1:].tolist()):
        bins[int(seq[a])].setdefault(int(rbin[a]), []).append((int(vb[a]), int(ve[b - 1])))
    none = np.iinfo(np.int64).max
    for a, b in zip(first.tolist(), first[1:].tolist() + [n]):
        s = int(seq[a])
        w0, w1 = beg[a:b] >> MIN_SHIFT, (end[a:b] - 1) >> MIN_SHIFT
        lin = np.full(int(w1.max()) + 1, none, np.int64)
        v = vb[a:b].astype(np.int64)
        np.minimum.at(lin, w0, v)
        for r in np.flatnonzero(w1 > w0).tolist():                              # the few records longer than a window
            lin[w0[r] + 1:w1[r] + 1] = np.minimum(lin[w0[r] + 1:w1[r] + 1], v[r])
        have = lin != none
        src = np.maximum.accumulate(np.where(have, np.arange(lin.size), -1))    # the last window with a record
        ioff[s] = np.where(src >= 0, lin[np.maximum(src, 0)], 0).astype(np.uint64)
        bins[s][PSEUDO_BIN] = [(int(vb[a]), int(ve[b - 1])), (b - a, 0)]
    return TabixIndex(names, bins, ioff)


def index_vcf_bgzf(path) -> TabixIndex:
    """The index of the bgzipped VCF at ``path``: the specification.  Walks the members, inflates them with
    zlib, finds the lines, takes CHROM, POS and len(REF) of every line that does not begin with '#', and calls
    ``build``.  Slow."""
    from . import bgzf
    name = str(path)
    with open(path, "rb") as f:
        raw = f.read()
    try:
        blocks, used = bgzf.bgzf_blocks(raw)
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None
    if used != len(raw) or not blocks:
        raise ValueError(f"{name}: BGZF block at byte {used}: truncated")
    parts = []
    for blk in blocks:
        data = zlib.decompress(raw[blk.payload_off:blk.payload_off + blk.payload_len], -15)
        if len(data) != blk.isize or zlib.crc32(data) != blk.crc:
            raise ValueError(f"{name}: BGZF block at byte {blk.file_off}: does not inflate to its ISIZE and CRC")
        parts.append(data)
    text = b"".join(parts)
    end_off = blocks[-1].file_off if blocks[-1].isize == 0 else len(raw)
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    starts = np.concatenate([[0], nl + 1])
    ends = np.concatenate([nl + 1, [len(text)]])                                # behind the newline
    if starts[-1] == len(text):
        starts, ends = starts[:-1], ends[:-1]
    ids: Dict[str, int] = {}
    seq, pos, ref_len, t_beg, t_end = [], [], [], [], []
    for s, e in zip(starts.tolist(), ends.tolist()):
        if text[s:s + 1] in (b"#", b"\n", b"\r") or s == e:
            continue
        t1 = text.find(b"\t", s, e)
        t2 = text.find(b"\t", t1 + 1, e)
        t3 = text.find(b"\t", t2 + 1, e)
        t4 = text.find(b"\t", t3 + 1, e)
        p = text[t1 + 1:t2]
        if min(t1, t2, t3, t4) < 0 or not p.isdigit():
            raise ValueError(f"{name}: the line at text byte {s} is not a VCF record (CHROM, POS, ID, REF)")
        seq.append(ids.setdefault(text[s:t1].decode(), len(ids)))
        pos.append(int(p))
        ref_len.append(t4 - t3 - 1)
        t_beg.append(s)
        t_end.append(e)
    try:
        beg, end = record_intervals(pos, ref_len)
        v = virtual_offsets(t_beg + t_end, [b.file_off for b in blocks], [b.isize for b in blocks], end_off)
        return build(list(ids), seq, beg, end, v[:len(t_beg)], v[len(t_beg):])
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None


def query(index: TabixIndex, name: str, beg: int, end: int) -> Optional[Tuple[int, int]]:
    """One span ``(v_lo, v_hi)`` of virtual offsets that holds every record of sequence ``name`` overlapping the
    0-based ``[beg, end)``, or None: the chunks of ``reg2bins`` that end behind ``ioff[beg >> 14]``, from the
    smallest ``cnk_beg`` (not below that ``ioff``) to the largest ``cnk_end``.  A sequence's records are
    contiguous in an indexed file, so the span holds that sequence only."""
    if name not in index.names:
        return None
    beg, end = max(int(beg), 0), min(int(end), BIN_LIMIT)
    if beg >= end:
        return None
    i = index.names.index(name)
    bins, ioff = index.bins[i], index.ioff[i]
    floor = int(ioff[min(beg >> MIN_SHIFT, ioff.size - 1)]) if ioff.size else 0
    chunks = [c for b in reg2bins(beg, end) for c in bins.get(b, ()) if c[1] > floor]
    if not chunks:
        return None
    return max(min(c[0] for c in chunks), floor), max(c[1] for c in chunks)
