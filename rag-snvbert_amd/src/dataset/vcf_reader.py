"""VCF input: POS and GT of ``.vcf`` / ``.vcf.gz`` files, the genotypes parsed on the GPU into bit rows.

The reference reads its inputs with ``allel.read_vcf(fields=['variants/POS', 'calldata/GT'])``
(src/dataset/embedding_rag_dataset.py:463-484, embedding_rag_infer_dataset.py:56-69); scikit-allel is
not a dependency here.  Two readers of the same grammar:

``parse_vcf_host``  the specification: plain, slow Python.  ``gt`` holds allele numbers, -1 for missing.
``read_vcf``        csrc/vcfread.hip: the body is streamed to the device in chunks, indexed by line,
                    parsed into one code byte per call and transposed into haplotype-major bit rows
                    (``device_features.gt_bits`` / the packed ``PanelIndex`` layout).

Grammar of a record (a body line of non-zero length, '\\n' or '\\r\\n' ended; lines are numbered from 1 over
the whole file): tab-separated columns, POS the second, FORMAT the ninth, one cell per sample from the
tenth.  Only the first ':'-delimited subfield of a cell is read, and FORMAT must begin with GT.  A GT
subfield is ``allele (sep allele)*``, allele = decimal digits or '.', sep = '|' or '/'; one allele is a
haploid call (the second haplotype is missing).  Conditions that raise ``ValueError`` naming the line —
the flag bits of ``snvrag_vcf_parse_gt``:

  1   FORMAT is absent or does not begin with GT followed by ':' or the column's end
  2   the number of sample columns differs from the header's
  4   a call has more than two alleles
  8   POS is absent, is not 1-10 decimal digits, or is >= 2^31
  16  a GT subfield does not follow the grammar (a byte that is none of digit . | /, an empty subfield,
      an empty allele)

``read_vcf`` streams: a chunk of at most ``chunk_bytes`` is cut at its last newline and the tail carried
into the next; two pinned host buffers alternate, chunk c + 1 is read (and inflated) and uploaded on a side
stream while chunk c parses.  Records beyond the last multiple of 64 stay in the code buffer for the next
chunk, so every chunk's bit block is whole bytes; the blocks are concatenated at the end.

``inflate="device"`` (``--vcf_inflate device``; ``DEFAULT_INFLATE`` / ``set_default_inflate``) inflates a BGZF
``.vcf.gz`` on the GPU (csrc/inflate.hip, one wave per block; ``bgzf.py`` walks the block headers and is the
kernel's specification): raw file bytes go up, the blocks of a chunk are inflated behind the previous chunk's
tail straight into the text buffer, the chunk is cut at its last newline by a device reduction, and the line
index, parse and pack steps run unchanged.  Only the few blocks that hold the header are inflated on the host.
A file that is not BGZF (plain text, a single-member gzip) takes the host path with one line of notice.

``region=(name, first, last)`` reads the records of one sequence with ``first <= POS <= last`` through the
file's tabix index ``path + ".tbi"`` (``tbi.py``; both VCF writers produce one with ``index=True`` /
``--vcf_index``): the header comes from the front of the file, ``tbi.query`` gives one span of virtual offsets, and
only the raw bytes of the members that span touches are read, inflated (either mode) and parsed.  Selection is
by POS, not by overlap: REF is not parsed, so a record that begins in front of ``first`` and reaches into the
region is not returned.  ``READ_STATS`` counts the members the last call inflated.

Not covered: single-member gzip on the device, ``.csi`` indexes, overlap (REF-length) selection of a region, an
indexer on the device for files this project did not write (``tbi.index_vcf_bgzf`` is the slow host
specification), a rank reading only its shard's sample columns, multi-allelic splitting (any allele number > 0 is
ALT; ALT ``A,C`` is carried as written), QUAL / FILTER / INFO and the header lines of an input, h5 files.

``columns=True`` also returns the CHROM, ID, REF and ALT strings of every record (``VcfGenotypes.columns``, a
``SiteColumns``; ``site_columns_host`` is the specification).  They are cut out on the device, inside the chunk
pipeline and before the text buffer is recycled: ``snvrag_vcf_cols_span`` walks every line to its fifth tab and
writes four (start, length) spans, the spans of the kept records are scanned (``torch.cumsum``) and
``snvrag_vcf_cols_gather`` packs the bytes into one blob per chunk; the blob is allocated by an upper bound (the
chunk's bytes less 2 S per record) and trimmed to its real size once the next chunk's line count has come back,
so no host wait is added.  The strings append in file order; the 64-record carry of the code rows does not touch them.
"""

from __future__ import annotations

import contextlib
import gzip
import io
import os
from dataclasses import dataclass
from typing import List, Tuple, Union

import numpy as np

FLAG_FORMAT, FLAG_COUNT, FLAG_PLOIDY, FLAG_POS, FLAG_GT = 1, 2, 4, 8, 16
FLAG_ERRORS = FLAG_FORMAT | FLAG_COUNT | FLAG_PLOIDY | FLAG_POS | FLAG_GT
FLAG_OFFSET = 1 << 31
FLAG_TEXT = {FLAG_FORMAT: "FORMAT does not begin with GT",
             FLAG_COUNT: "the number of sample columns differs from the header's",
             FLAG_PLOIDY: "a call has more than two alleles",
             FLAG_POS: "POS is not a decimal number below 2^31",
             FLAG_GT: "a GT field is malformed"}
CODE_ALT1, CODE_ALT2, CODE_MISS1, CODE_MISS2, CODE_SLASH = 1, 2, 4, 8, 16
DEFAULT_CHUNK_BYTES = 256 << 20
MAX_CHUNK_BYTES = (1 << 31) - 64
INFLATE_MODES = ("host", "device")
DEFAULT_INFLATE = "host"               # what read_vcf(inflate=None) does; set_default_inflate changes it
MAX_CHUNK_BLOCKS = 1 << 16             # BGZF blocks per chunk of the device inflate (empty blocks are legal)
RAW_PIECE = 1 << 20                    # raw file bytes per read of the device inflate
SMALL_SPAN = 32 << 20                  # a region's raw bytes up to here are read at once and size its buffers
READ_STATS = {"members_inflated": 0}   # of the last read_vcf of a BGZF file by its member table (header members too)


def set_default_inflate(mode: str) -> None:
    """Where ``read_vcf`` inflates BGZF files unless told otherwise: "host" (zlib) or "device"."""
    global DEFAULT_INFLATE
    if mode not in INFLATE_MODES:
        raise ValueError(f"inflate must be one of {INFLATE_MODES}, not {mode!r}")
    DEFAULT_INFLATE = mode


def is_vcf_path(path) -> bool:
    p = str(path).lower()
    return p.endswith(".vcf") or p.endswith(".vcf.gz")


def flag_error(name: str, lineno: int, flags: int) -> ValueError:
    """The error both readers raise for a record whose flags are not zero."""
    what = "; ".join(t for bit, t in FLAG_TEXT.items() if flags & bit)
    return ValueError(f"{name}: line {lineno}: {what}")


def _open(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")      # BGZF is multi-member gzip


def _header_samples(line: bytes, name: str) -> List[str]:
    cols = line.rstrip(b"\r\n").split(b"\t")
    if len(cols) < 10:
        raise ValueError(f"{name}: the #CHROM header names no samples")
    return [c.decode() for c in cols[9:]]


def gt_alleles(sub: bytes) -> Tuple[List[int], bool]:
    """(allele numbers with -1 for '.', malformed) of one GT subfield."""
    alleles: List[int] = []
    state, bad = 0, False                  # 0: an allele must begin, 1: inside digits, 2: behind '.'
    for c in sub:
        if 48 <= c <= 57:
            if state == 0:
                alleles.append(c - 48)
                state = 1
            elif state == 1:
                alleles[-1] = alleles[-1] * 10 + (c - 48)
            else:
                bad = True
        elif c == 46:
            if state == 0:
                alleles.append(-1)
                state = 2
            else:
                bad = True
        elif c in (124, 47):
            if state == 0:
                bad = True
            state = 0
        else:
            bad = True
    return alleles, bad or state == 0


def record_flags(line: bytes, n_samples: int):
    """(flags, pos, calls) of one record without its newline: calls = [(allele 1, allele 2)] per cell."""
    if line.endswith(b"\r"):
        line = line[:-1]
    f = line.split(b"\t")
    flags, pos = 0, 0
    p = f[1] if len(f) > 1 else b""
    if 1 <= len(p) <= 10 and p.isdigit() and int(p) < 1 << 31:
        pos = int(p)
    else:
        flags |= FLAG_POS
    fmt = f[8] if len(f) > 8 else b""
    if not (fmt[:2] == b"GT" and (len(fmt) == 2 or fmt[2:3] == b":")):
        flags |= FLAG_FORMAT
    cells = f[9:]
    if len(cells) != n_samples:
        flags |= FLAG_COUNT
    calls = []
    for cell in cells:
        alleles, bad = gt_alleles(cell.split(b":", 1)[0])
        if bad:
            flags |= FLAG_GT
        if len(alleles) > 2:
            flags |= FLAG_PLOIDY
        a = (alleles + [-1, -1])[:2]
        calls.append((min(a[0], 127), min(a[1], 127)))
    return flags, pos, calls


def _host_text(path_or_bytes) -> Tuple[str, bytes]:
    """(name, the whole text) of a VCF given by path or as bytes, ``.gz`` by its magic bytes."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        name, data = "<bytes>", bytes(path_or_bytes)
        if data[:2] == b"\x1f\x8b":
            data = gzip.decompress(data)
    else:
        name = str(path_or_bytes)
        with _open(path_or_bytes) as fh:
            data = fh.read()
    return name, data


def parse_vcf_host(path_or_bytes: Union[str, os.PathLike, bytes]):
    """(samples, pos int32 [n], gt int8 [n, S, 2]) of a VCF given by path (``.gz`` by its magic bytes) or
    as bytes: allele numbers (capped at 127), -1 for missing, as ``allel.read_vcf`` documents
    ``calldata/GT``.  The specification of ``read_vcf``; ``ValueError`` names the 1-based file line."""
    name, data = _host_text(path_or_bytes)
    samples, pos, gt = None, [], []
    for lineno, line in enumerate(data.split(b"\n"), 1):
        if samples is None:
            if line.startswith(b"#CHROM"):
                samples = _header_samples(line, name)
            elif line.strip() and not line.startswith(b"#"):
                raise ValueError(f"{name}: line {lineno}: a record in front of the #CHROM header")
            continue
        if line in (b"", b"\r"):
            continue
        flags, p, calls = record_flags(line, len(samples))
        if flags:
            raise flag_error(name, lineno, flags)
        pos.append(p)
        gt.append(calls)
    if samples is None:
        raise ValueError(f"{name}: no #CHROM header")
    S = len(samples)
    return samples, np.asarray(pos, np.int32), np.asarray(gt, np.int8).reshape(len(pos), S, 2)


COLUMN_NAMES = ("chrom", "id", "ref", "alt")
COLUMN_FIELDS = (0, 2, 3, 4)               # their 0-based places in a record


def record_columns(line: bytes) -> Tuple[bytes, bytes, bytes, bytes]:
    """(CHROM, ID, REF, ALT) of one record without its newline: the tab-separated columns 1, 3, 4 and 5, the
    last column of a short line ending in front of a trailing '\\r'; a column the line does not reach is b""."""
    if line.endswith(b"\r"):
        line = line[:-1]
    f = line.split(b"\t")
    return tuple(f[k] if len(f) > k else b"" for k in COLUMN_FIELDS)


class SiteColumns:
    """CHROM, ID, REF and ALT of ``n`` records as packed bytes: for each name of ``COLUMN_NAMES`` an int64
    ``<name>_off`` [n + 1] and a uint8 ``<name>_blob`` (host arrays); record r's string is
    ``blob[off[r]:off[r + 1]]``.  ``chrom(r)`` / ``id(r)`` / ``ref(r)`` / ``alt(r)`` give it as ``bytes``,
    ``column(name)`` all of them, ``lengths(name)`` and ``ref_len`` the int64 lengths."""

    def __init__(self, parts):
        """``parts``: (off, blob) per name of ``COLUMN_NAMES``, in that order."""
        assert len(parts) == len(COLUMN_NAMES)
        for name, (off, blob) in zip(COLUMN_NAMES, parts):
            off, blob = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(blob, np.uint8)
            assert off.ndim == 1 and off.size >= 1 and off[0] == 0 and off[-1] == blob.size
            setattr(self, name + "_off", off)
            setattr(self, name + "_blob", blob)
        self.n = int(self.chrom_off.size) - 1
        assert all(getattr(self, name + "_off").size == self.n + 1 for name in COLUMN_NAMES)

    @classmethod
    def from_records(cls, records) -> "SiteColumns":
        """Of a sequence of (CHROM, ID, REF, ALT) bytes."""
        parts = []
        for c in range(len(COLUMN_NAMES)):
            strings = [r[c] for r in records]
            off = np.zeros(len(strings) + 1, np.int64)
            np.cumsum([len(t) for t in strings], out=off[1:])
            parts.append((off, np.frombuffer(b"".join(strings), np.uint8)))
        return cls(parts)

    def __len__(self) -> int:
        return self.n

    def get(self, name: str, r: int) -> bytes:
        off = getattr(self, name + "_off")
        if not 0 <= r < self.n:
            raise IndexError(r)
        return getattr(self, name + "_blob")[off[r]:off[r + 1]].tobytes()

    def chrom(self, r: int) -> bytes:
        return self.get("chrom", r)

    def id(self, r: int) -> bytes:
        return self.get("id", r)

    def ref(self, r: int) -> bytes:
        return self.get("ref", r)

    def alt(self, r: int) -> bytes:
        return self.get("alt", r)

    def column(self, name: str) -> List[bytes]:
        off, blob = getattr(self, name + "_off"), getattr(self, name + "_blob").tobytes()
        return [blob[off[r]:off[r + 1]] for r in range(self.n)]

    def lengths(self, name: str) -> np.ndarray:
        return np.diff(getattr(self, name + "_off"))

    @property
    def ref_len(self) -> np.ndarray:
        return self.lengths("ref")


def site_columns_host(path_or_bytes: Union[str, os.PathLike, bytes]) -> SiteColumns:
    """CHROM, ID, REF and ALT of every record of a VCF given by path (``.gz`` by its magic bytes) or as bytes:
    the specification of ``read_vcf(columns=True).columns``.  The line rules of ``parse_vcf_host``: the body
    begins behind the #CHROM line, zero-length lines ("" and "\\r") vanish, "\\r\\n" ends a line as "\\n"
    does.  The records are not checked otherwise (``parse_vcf_host`` does that)."""
    name, data = _host_text(path_or_bytes)
    records, body = [], False
    for line in data.split(b"\n"):
        if not body:
            body = line.startswith(b"#CHROM")
            continue
        if line in (b"", b"\r"):
            continue
        records.append(record_columns(line))
    if not body:
        raise ValueError(f"{name}: no #CHROM header")
    return SiteColumns.from_records(records)


@dataclass
class VcfGenotypes:
    """What ``read_vcf`` returns.  ``alt_bits`` / ``miss_bits``: device u8 [2 S, ceil(n_sites / 8)],
    haplotype h of sample s in row 2 s + h, site r at bit r & 7 of byte r >> 3 (``gt_bits`` layout);
    an ALT bit is 0 where the call is missing.  ``phased``: no call used '/'."""
    samples: List[str]
    pos: np.ndarray
    alt_bits: "object"
    miss_bits: "object"
    n_sites: int
    any_missing: bool
    phased: bool
    columns: "SiteColumns" = None          # read_vcf(columns=True): CHROM, ID, REF, ALT of the n_sites records

    def gt(self) -> np.ndarray:
        """int8 [n_sites, S, 2]: 0 / 1 (any ALT allele is 1), -1 where missing; unpacked on the device,
        one copy to the host."""
        from .. import kernels as K
        if self.n_sites == 0:
            return np.zeros((0, len(self.samples), 2), np.int8)
        return K.vcf_unpack_gt(self.alt_bits, self.miss_bits, self.n_sites).cpu().numpy()


def _last_newline(a: np.ndarray, n: int) -> int:
    """Index of the last '\\n' in a[:n], or -1."""
    hi, step = n, 1 << 16
    while hi > 0:
        lo = max(0, hi - step)
        hit = np.flatnonzero(a[lo:hi] == 10)
        if hit.size:
            return lo + int(hit[-1])
        hi, step = lo, step * 4
    return -1


def _record_line(path, record: int) -> int:
    """The 1-based file line of body record ``record`` (0-based among the lines of non-zero length)."""
    seen, body = -1, False
    with _open(path) as fh:
        for lineno, line in enumerate(fh, 1):
            if not body:
                body = line.startswith(b"#CHROM")
                continue
            if line not in (b"\n", b"\r\n", b"", b"\r"):
                seen += 1
                if seen == record:
                    return lineno
    raise ValueError(f"{path}: record {record} not found")


class _ChunkParser:
    """What follows a chunk's text on the device, for either source of the text: line index, parse, and the
    pack of every whole group of 64 records; ``finish`` joins the parts."""

    def __init__(self, path, name, dev, samples, chunk_bytes, force_general, region=None, columns=False):
        import torch
        # columns: per chunk the lengths (i64 [4 n], column-major) and the trimmed blob of each column; the last
        # chunk's untrimmed blob with its offsets waits in col_pending until its kernels are known to be done
        self.columns, self.col_lens, self.col_blobs, self.col_pending = columns, [], [[] for _ in COLUMN_NAMES], None
        self.path, self.name, self.dev, self.samples, self.force_general = path, name, dev, samples, force_general
        # a region read: the records kept per chunk (count, their line offsets, the chunk's place in the span's
        # text) and the span's members (file offset, ISIZE), for the virtual offset an error message names
        self.region, self.kept, self.members, self.text_base = region, [], [], 0
        self.S = S = len(samples)
        # a record holds at least 8 one-byte columns, GT and S one-byte cells, each with its separator
        self.max_lines = chunk_bytes // (2 * S + 17) + 1
        self.codes = torch.empty(self.max_lines + 64, (S + 3) // 4 * 4, device=dev, dtype=torch.uint8)
        self.pos_parts, self.flag_parts, self.alt_parts, self.miss_parts = [], [], [], []
        self.carry = self.n_records = 0

    def _pack(self, n):
        import torch
        from .. import kernels as K
        ld = ((n + 7) // 8 + 7) // 8 * 8
        alt = torch.empty(2 * self.S, ld, device=self.dev, dtype=torch.uint8)
        miss = torch.empty(2 * self.S, ld, device=self.dev, dtype=torch.uint8)
        K.vcf_pack_rows(self.codes, n, self.S, alt, miss)
        self.alt_parts.append(alt[:, :(n + 7) // 8])
        self.miss_parts.append(miss[:, :(n + 7) // 8])

    def chunk(self, text, cut, last, parsed_event, stream):
        """``text[:cut]`` (padded with '\\n' to 16 bytes) is a chunk of whole lines; ``last``: nothing follows."""
        from .. import kernels as K
        line_off, n_lines = K.vcf_line_index(text, cut, self.max_lines)
        nl = int(n_lines.item())                       # also: the chunk's upload has left the host
        self._trim()                                   # and the previous chunk's gather is done
        if nl > self.max_lines:                        # a line shorter than any record
            if self.region is None:                    # (a region read does not scan the file for the line)
                parse_vcf_host(self.path)
            raise ValueError(f"{self.name}: a body line is shorter than a record of {self.S} samples")
        if nl:
            p, f = K.vcf_parse_gt(text, cut, line_off, nl, self.S, self.codes[self.carry:], self.force_general)
            spans, lo = (K.vcf_cols_span(text, cut, line_off, nl) if self.columns else None), 0
            if self.region is not None:
                p, f, nl, lo = self._select(p, f, line_off, nl)
        if nl:
            self.pos_parts.append(p)
            self.flag_parts.append(f)
            if self.columns:
                self._gather(text, cut, spans[lo:lo + nl])
        parsed_event.record(stream)
        total = self.carry + nl
        full = total if last else total // 64 * 64
        if full:
            self._pack(full)
            self.carry = total - full
            if self.carry:                             # fewer than 64 <= full rows: no overlap
                self.codes[:self.carry].copy_(self.codes[full:total])
        else:
            self.carry = total
        self.n_records += nl

    def _select(self, p, f, line_off, nl):
        """Drop the records the span brought in outside [first, last]: positions are sorted inside a sequence,
        so those are a prefix and a suffix of the chunk, and the kept code rows move to the front of the chunk's."""
        _, first, last = self.region
        pos = p.cpu().numpy()
        hit = np.flatnonzero((pos >= first) & (pos <= last))
        lo, hi = (int(hit[0]), int(hit[-1]) + 1) if hit.size else (0, 0)
        if hit.size != hi - lo:
            raise ValueError(f"{self.name}: the positions between POS {int(pos[lo])} and {int(pos[hi - 1])} are not "
                             "sorted: the index does not describe this file")
        if lo and hi > lo:
            self.codes[self.carry:self.carry + hi - lo].copy_(self.codes[self.carry + lo:self.carry + hi].clone())
        if hi > lo:
            self.kept.append((hi - lo, line_off[lo:hi].clone(), self.text_base))
        return p[lo:hi], f[lo:hi], hi - lo, lo

    def _gather(self, text, cut, spans):
        """The strings of the kept records' spans packed into one blob, the four columns one behind the other.
        A valid record spends at least 2 S bytes on its cells, so the blob is bounded without a host wait; a
        record that breaks the bound is flagged by the parse and copied nowhere."""
        import torch
        from .. import kernels as K
        n = spans.shape[0]
        lens = spans[:, 1::2].t().reshape(-1).to(torch.int64)          # item c n + r: column c of record r
        off = torch.zeros(4 * n + 1, device=self.dev, dtype=torch.int64)
        torch.cumsum(lens, 0, out=off[1:])
        blob = torch.empty(max(cut - 2 * self.S * n, 16), device=self.dev, dtype=torch.uint8)
        K.vcf_cols_gather(text, cut, spans, off, blob)
        self.col_lens.append(lens.view(4, n))
        self.col_pending = (blob, off[::n])

    def _trim(self):
        """The pending blob cut into its four columns at their real sizes.  Called where the kernels that wrote
        it are known to have finished, so the five offsets come back without a wait of their own."""
        if self.col_pending is None:
            return
        blob, bounds = self.col_pending
        b = [min(int(v), blob.numel()) for v in bounds.cpu().tolist()]
        for c in range(len(COLUMN_NAMES)):
            self.col_blobs[c].append(blob[b[c]:b[c + 1]].clone())
        self.col_pending = None

    def _site_columns(self) -> "SiteColumns":
        """The parts joined: per column one copy of the offsets and one of the blob to the host."""
        import torch
        parts = []
        for c in range(len(COLUMN_NAMES)):
            off = torch.zeros(self.n_records + 1, device=self.dev, dtype=torch.int64)
            if self.n_records:
                torch.cumsum(torch.cat([l[c] for l in self.col_lens]), 0, out=off[1:])
                blob = torch.cat(self.col_blobs[c])
            else:
                blob = torch.zeros(0, device=self.dev, dtype=torch.uint8)
            off, blob = off.cpu().numpy(), blob.cpu().numpy()
            if off[-1] != blob.size:                   # every record passed the flags: cannot happen
                raise RuntimeError(f"{self.name}: the {COLUMN_NAMES[c].upper()} strings take {int(off[-1])} bytes, "
                                   f"{blob.size} were gathered")
            parts.append((off, blob))
        return SiteColumns(parts)

    def _region_error(self, r, pos, flags) -> ValueError:
        """The file line of a region's record is not known without a full scan: POS and the virtual offset."""
        from . import tbi
        for k, off, base in self.kept:
            if r < k:
                t = base + int(off[r].item())
                break
            r -= k
        offs, sizes = zip(*self.members)
        v = int(tbi.virtual_offsets([t], offs, sizes, offs[-1] + 1)[0])
        what = "; ".join(t for bit, t in FLAG_TEXT.items() if flags & bit)
        return ValueError(f"{self.name}: record at POS {pos} (virtual offset {v}: byte {v & 0xffff} of the member at "
                          f"file byte {v >> 16}): {what}")

    def finish(self) -> "VcfGenotypes":
        import torch
        dev, S, name = self.dev, self.S, self.name
        if self.carry:                                 # the file ended in an empty chunk
            self._pack(self.carry)
        if self.n_records:
            flags = torch.cat(self.flag_parts).cpu().numpy().view(np.uint32)
            pos = torch.cat(self.pos_parts).cpu().numpy()
            alt_bits = torch.cat(self.alt_parts, 1).contiguous()
            miss_bits = torch.cat(self.miss_parts, 1).contiguous()
        else:
            flags, pos = np.zeros(0, np.uint32), np.zeros(0, np.int32)
            alt_bits = torch.zeros(2 * S, 0, device=dev, dtype=torch.uint8)
            miss_bits = torch.zeros(2 * S, 0, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize(dev)
        self._trim()
        bad = np.flatnonzero(flags & np.uint32(FLAG_ERRORS | FLAG_OFFSET))
        if bad.size:
            r = int(bad[0])
            if int(flags[r]) & FLAG_OFFSET:
                raise RuntimeError(f"{name}: record {r}: the line index gave an offset outside its chunk")
            if self.region is not None:
                raise self._region_error(r, int(pos[r]), int(flags[r]) & FLAG_ERRORS)
            raise flag_error(name, _record_line(self.path, r), int(flags[r]) & FLAG_ERRORS)
        seen = int(np.bitwise_or.reduce(flags >> np.uint32(8))) if flags.size else 0
        return VcfGenotypes(self.samples, pos.astype(np.int32, copy=False), alt_bits, miss_bits, self.n_records,
                            bool(seen & (CODE_MISS1 | CODE_MISS2)), not seen & CODE_SLASH,
                            self._site_columns() if self.columns else None)


def read_vcf(path, device, chunk_bytes: int = DEFAULT_CHUNK_BYTES, force_general: bool = False,
             inflate: str = None, region=None, columns: bool = False) -> VcfGenotypes:
    """POS and GT of the VCF at ``path``, the body parsed on ``device``.  ``.gz`` / BGZF is inflated on the host
    (streaming), or with ``inflate="device"`` (``None``: ``DEFAULT_INFLATE``) on the GPU when the file is BGZF.
    ``force_general`` sends every line through the general parse path (same result).  ``ValueError``: what
    ``parse_vcf_host`` raises for the file, a line longer than ``chunk_bytes``, or a BGZF block that does not
    inflate (``inflate="device"``: "<path>: BGZF block at byte <file offset>: <what>").

    ``region=(name, first, last)``: what the whole-file read gives, restricted to the records of sequence ``name``
    with ``first <= POS <= last`` (1-based, inclusive; by POS, not by overlap: REF is not parsed).  Needs a BGZF
    file and its tabix index ``path + ".tbi"`` (``ValueError`` without either; ``.csi`` is not read); only the
    members the index names for the region are read from disk, inflated (zlib member by member, or the device
    table path) and parsed.  A name the index does not hold, or an empty span, gives an empty result.  An error
    message of a region read names the record's POS and virtual offset in place of the file line.  The record
    flags are checked for the region's records only; a line of the span that is shorter than any record raises
    whether or not it lies in the region (it is met before POS is known), without the file line.

    ``columns=True``: the result's ``columns`` holds the CHROM, ID, REF and ALT bytes of the returned records
    (``SiteColumns``; of a region read, of the kept records only), cut out of the text on the device.  Every
    other field is what ``columns=False`` gives, bit for bit."""
    import torch
    from .. import native as N
    N.require_gpu()
    if not 64 <= chunk_bytes <= MAX_CHUNK_BYTES:
        raise ValueError(f"chunk_bytes must be in [64, {MAX_CHUNK_BYTES}]")
    mode = DEFAULT_INFLATE if inflate is None else inflate
    if mode not in INFLATE_MODES:
        raise ValueError(f"inflate must be one of {INFLATE_MODES}, not {mode!r}")
    name, dev = str(path), torch.device(device)
    READ_STATS["members_inflated"] = 0
    if region is not None:
        return _read_vcf_region(path, name, dev, chunk_bytes, force_general, mode, region, columns)
    if mode == "device":
        from .bgzf import is_bgzf
        if is_bgzf(path):
            return _read_vcf_device_inflate(path, name, dev, chunk_bytes, force_general, columns=columns)
        print(f"{name}: not a BGZF file, inflate=\"device\" does not apply: reading it on the host")
    with _open(path) as fh:
        if not isinstance(fh, gzip.GzipFile):               # no buffer larger than the file itself
            chunk_bytes = min(chunk_bytes, max(64, os.path.getsize(path) + 1))
        samples = None
        for line in fh:
            if line.startswith(b"#CHROM"):
                samples = _header_samples(line, name)
                break
            if line.strip() and not line.startswith(b"#"):
                parse_vcf_host(path)           # raises the specification's error
                raise ValueError(f"{name}: a record in front of the #CHROM header")
        if samples is None:
            raise ValueError(f"{name}: no #CHROM header")
        return _parse_text(fh, _ChunkParser(path, name, dev, samples, chunk_bytes, force_general, columns=columns),
                           chunk_bytes)


def _parse_text(fh, parser, chunk_bytes) -> VcfGenotypes:
    """The body text that ``fh.readinto`` gives, streamed through ``parser`` in chunks of whole lines."""
    import torch
    name, dev = parser.name, parser.dev
    cap = (chunk_bytes + 15) // 16 * 16
    with torch.cuda.device(dev):
        main, side = torch.cuda.current_stream(), torch.cuda.Stream()
        pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        text = [torch.empty(cap, device=dev, dtype=torch.uint8) for _ in range(2)]
        uploaded = [torch.cuda.Event(), torch.cuda.Event()]
        parsed = [torch.cuda.Event(), torch.cuda.Event()]
        tail, eof, c, taken = b"", False, 0, 0
        while not eof or tail:
            b = c & 1
            buf = pinned[b].numpy()                      # chunk c - 2 left it: its parse was waited for below
            n = len(tail)
            buf[:n] = np.frombuffer(tail, np.uint8)
            view = memoryview(buf)
            parser.text_base = taken - n                 # of buf[0] in the text read so far
            while n < chunk_bytes:
                got = fh.readinto(view[n:chunk_bytes])
                if not got:
                    eof = True
                    break
                n += got
                taken += got
            if eof and n and buf[n - 1] != 10 and n < chunk_bytes:
                buf[n] = 10                                # a last line without its newline
                n += 1
            cut = _last_newline(buf, n) + 1
            if cut == 0 and n:
                raise ValueError(f"{name}: a line is longer than chunk_bytes = {chunk_bytes}")
            tail = buf[cut:n].tobytes()
            c += 1
            if cut == 0:
                continue
            padded = (cut + 15) // 16 * 16
            buf[cut:padded] = 10
            side.wait_event(parsed[b])                     # text[b] was last read by chunk c - 2's parse
            with torch.cuda.stream(side):
                text[b][:padded].copy_(pinned[b][:padded], non_blocking=True)
                uploaded[b].record(side)
            main.wait_event(uploaded[b])
            parser.chunk(text[b], cut, eof and not tail, parsed[b], main)
        main.wait_stream(side)
        return parser.finish()


def _bgzf_error(name: str, file_off: int, what: str) -> ValueError:
    return ValueError(f"{name}: BGZF block at byte {file_off}: {what}")


def _bgzf_header(path, name, fh):
    """Inflate blocks from the front on the host until the #CHROM line is whole.  Returns (samples, the file
    offset of the block that holds the first body byte, the header bytes in front of it in that block)."""
    import zlib
    from . import bgzf
    head, starts, buf, pos, scan, ended = bytearray(), [], b"", 0, 0, False
    while True:
        piece = fh.read(RAW_PIECE)
        buf += piece
        try:
            blocks, used = bgzf.bgzf_blocks(buf, pos)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if not piece:
            if used < len(buf):
                raise _bgzf_error(name, pos + used, "truncated")
            ended = True
        for blk in blocks:
            o = blk.payload_off
            payload = bytes(buf[o:o + blk.payload_len])
            try:
                data = zlib.decompress(payload, -15)
                ok = len(data) == blk.isize and zlib.crc32(data) == blk.crc
            except zlib.error:
                ok = False
            if not ok:
                st = bgzf.inflate_member_host(payload, blk.isize, blk.crc)[1]
                raise _bgzf_error(name, blk.file_off, bgzf.STATUS_TEXT.get(st, "does not inflate"))
            READ_STATS["members_inflated"] += 1
            starts.append((blk.file_off, len(head), o + blk.payload_len + 8 - (blk.file_off - pos)))
            head += data
            while True:                                        # whole lines of the header so far
                e = head.find(b"\n", scan)
                if e < 0:
                    break
                line = bytes(head[scan:e])
                if line.startswith(b"#CHROM"):
                    body0 = e + 1
                    for file_off, start, size in reversed(starts):
                        if start <= body0:
                            if body0 == len(head):             # the body begins with the next block
                                return _header_samples(line, name), file_off + size, 0
                            return _header_samples(line, name), file_off, body0 - start
                if line.strip() and not line.startswith(b"#"):
                    parse_vcf_host(path)                       # raises the specification's error
                    raise ValueError(f"{name}: a record in front of the #CHROM header")
                scan = e + 1
        buf, pos = buf[used:], pos + used
        if ended:
            line = bytes(head[scan:])
            if line.startswith(b"#CHROM"):                     # a header line without its newline ends the file
                return _header_samples(line, name), pos, 0
            if line.strip() and not line.startswith(b"#"):
                parse_vcf_host(path)
            raise ValueError(f"{name}: no #CHROM header")


class _RawSpan:
    """The raw bytes [start, end) of an open file, as the reads of the device inflate take them."""

    def __init__(self, fh, start: int, end: int):
        self.fh, self.left = fh, end - start
        fh.seek(start)

    def readinto(self, view) -> int:
        got = self.fh.readinto(view[:min(len(view), self.left)]) if self.left > 0 else 0
        self.left -= got or 0
        return got or 0

    def read(self, n: int) -> bytes:
        data = self.fh.read(max(min(n, self.left), 0))
        self.left -= len(data)
        return data


class _SpanText:
    """The text of the members of a span, inflated with zlib member by member (a region read with
    ``inflate="host"``), as ``readinto`` gives it: ``skip`` bytes of the first member are replaced by '\n', and
    the member at file offset ``cut_off`` is cut (filled with '\n') from its byte ``cut``."""

    def __init__(self, raw: _RawSpan, name, start, skip, cut_off, cut, parser):
        self.raw, self.name, self.pos, self.parser = raw, name, start, parser
        self.skip, self.cut_off, self.cut = skip, cut_off, cut
        self.rest, self.text, self.at = b"", b"", 0

    def _more(self) -> bool:
        import zlib
        from . import bgzf
        piece = self.raw.read(RAW_PIECE)
        data = self.rest + piece
        try:
            blocks, used = bgzf.bgzf_blocks(data, self.pos)
        except ValueError as e:
            raise ValueError(f"{self.name}: {e}") from None
        if not piece:
            if data:
                raise _bgzf_error(self.name, self.pos, "truncated")
            return False
        parts = []
        for blk in blocks:
            payload = data[blk.payload_off:blk.payload_off + blk.payload_len]
            try:
                text = zlib.decompress(payload, -15)
                ok = len(text) == blk.isize and zlib.crc32(text) == blk.crc
            except zlib.error:
                ok = False
            if not ok:
                st = bgzf.inflate_member_host(payload, blk.isize, blk.crc)[1]
                raise _bgzf_error(self.name, blk.file_off, bgzf.STATUS_TEXT.get(st, "does not inflate"))
            if self.skip:
                text, self.skip = b"\n" * self.skip + text[self.skip:], 0
            if self.cut and blk.file_off == self.cut_off:
                text = text[:self.cut] + b"\n" * (len(text) - self.cut)
            parts.append(text)
            self.parser.members.append((blk.file_off, blk.isize))
            READ_STATS["members_inflated"] += 1
        self.rest, self.pos = data[used:], self.pos + used
        self.text, self.at = b"".join(parts), 0
        return True

    def readinto(self, view) -> int:
        while self.at == len(self.text):
            if not self._more():
                return 0
        n = min(len(view), len(self.text) - self.at)
        view[:n] = self.text[self.at:self.at + n]
        self.at += n
        return n


def _read_vcf_region(path, name, dev, chunk_bytes, force_general, mode, region, columns=False) -> VcfGenotypes:
    """``read_vcf(region=...)``: the header from the front of the file, the body from the one span of virtual
    offsets ``tbi.query`` gives for the region.  Raw bytes are read from the member at ``v_lo >> 16`` to the end
    of the member at ``v_hi >> 16`` (its length from its own header; not read when ``v_hi & 0xffff`` is 0); the
    text in front of ``v_lo & 0xffff`` in the first member becomes '\n' (the grammar skips empty lines) and the
    last member is cut at ``v_hi & 0xffff``."""
    from . import bgzf, tbi
    seq, first, last = str(region[0]), int(region[1]), int(region[2])
    if not bgzf.is_bgzf(path):
        raise ValueError(f"{name}: a region read needs a BGZF file (bgzip / --vcf_bgzf) and its .tbi index")
    if not os.path.exists(name + ".tbi"):
        raise ValueError(f"{name}: a region read needs the tabix index {name}.tbi (write_vcf(index=True) / "
                         "--vcf_index, or tabix -p vcf); .csi indexes are not read")
    index = tbi.read(name + ".tbi")
    with open(path, "rb") as fh:
        samples, _, _ = _bgzf_header(path, name, fh)
        span = tbi.query(index, seq, first - 1, last) if first <= last else None
        if span is None:
            return _ChunkParser(path, name, dev, samples, 64, force_general, columns=columns).finish()
        (start, cut_off), (skip, cut) = (v >> 16 for v in span), (v & 0xffff for v in span)
        end = cut_off
        if cut:                                            # the last member's length, from its own header
            fh.seek(cut_off)
            try:
                blocks, _ = bgzf.bgzf_blocks(fh.read(bgzf.MAX_BLOCK), cut_off)
            except ValueError as e:
                raise ValueError(f"{name}: {e} (does {name}.tbi describe this file?)") from None
            if not blocks:
                raise _bgzf_error(name, cut_off, f"truncated (does {name}.tbi describe this file?)")
            end = cut_off + blocks[0].payload_off + blocks[0].payload_len + 8
        raw = _RawSpan(fh, start, end)
        if end - start <= SMALL_SPAN:                      # buffers of the span's size, not of chunk_bytes
            data = raw.read(end - start)
            try:
                blocks, used = bgzf.bgzf_blocks(data, start)
            except ValueError as e:
                raise ValueError(f"{name}: {e} (does {name}.tbi describe this file?)") from None
            if used != end - start:
                raise _bgzf_error(name, start + used, f"truncated (does {name}.tbi describe this file?)")
            chunk_bytes = min(chunk_bytes, max(64, sum(blk.isize for blk in blocks) + 64))
            raw = _RawSpan(io.BytesIO(data), 0, len(data))
        parser = _ChunkParser(path, name, dev, samples, chunk_bytes, force_general, region=(seq, first, last),
                              columns=columns)
        if mode == "device":
            return _read_vcf_device_inflate(path, name, dev, chunk_bytes, force_general, parser,
                                            (raw, start, end, skip, cut_off, cut))
        return _parse_text(_SpanText(raw, name, start, skip, cut_off, cut, parser), parser, chunk_bytes)


def _read_vcf_device_inflate(path, name, dev, chunk_bytes, force_general, parser=None, span=None,
                             columns=False) -> VcfGenotypes:
    """``read_vcf`` of a BGZF file with the blocks inflated on the device (``span``: of a region read, the raw
    bytes, their file range, and where the text begins in the first member and ends in the last).  Per chunk:
    raw bytes are read into
    one of two pinned buffers RAW_PIECE at a time and their block headers walked until the next block would not
    fit (``tail + sum ISIZE <= chunk_bytes``, at most MAX_CHUNK_BLOCKS blocks, the raw buffer); the taken bytes
    go up on the side stream; the blocks are inflated into ``text[b]`` behind the previous chunk's tail; status
    and the index of the last newline come back in one read; the tail is copied to the other text buffer, the
    chunk padded and parsed."""
    import torch
    from .. import kernels as K
    from . import bgzf
    with (open(path, "rb") if span is None else contextlib.nullcontext(span[0])) as fh:
        span_cut_off = span_cut = 0                    # a region's end: the member it lies in, the text byte in it
        if span is None:
            samples, off0, skip = _bgzf_header(path, name, fh)
            fh.seek(off0)
            end = os.path.getsize(path)
        else:
            _, off0, end, skip, span_cut_off, span_cut = span
        cap = (chunk_bytes + 15) // 16 * 16
        rawcap = min(chunk_bytes // 4 + 2 * RAW_PIECE, max(end - off0, 0) + 64)
        with torch.cuda.device(dev):
            main, side = torch.cuda.current_stream(), torch.cuda.Stream()
            raw = [torch.empty(rawcap, dtype=torch.uint8).pin_memory() for _ in range(2)]
            tables = [torch.empty(MAX_CHUNK_BLOCKS, 4, dtype=torch.int64).pin_memory() for _ in range(2)]
            comp = [torch.empty(rawcap, device=dev, dtype=torch.uint8) for _ in range(2)]
            table_dev = torch.empty(MAX_CHUNK_BLOCKS, 4, device=dev, dtype=torch.int64)
            text = [torch.empty(cap, device=dev, dtype=torch.uint8) for _ in range(2)]
            res = torch.empty(2 + MAX_CHUNK_BLOCKS, device=dev, dtype=torch.int32)     # last newline (i64), status
            uploaded = [torch.cuda.Event(), torch.cuda.Event()]
            parsed = [torch.cuda.Event(), torch.cuda.Event()]
            if parser is None:
                parser = _ChunkParser(path, name, dev, samples, chunk_bytes, force_general, columns=columns)
            rest = np.zeros(0, np.uint8)           # raw bytes read and not yet taken: whole blocks and a partial one
            base = off0                            # file offset of rest[0]
            tail_len, eof, c, text_seen = 0, False, 0, 0
            deferred = None                        # a record-level error: raised once every block has inflated
            while not eof or tail_len or rest.size:
                b = c & 1
                # raw[b] and tables[b] were last read by chunk c - 2's copies, which chunk c - 1's read-back followed
                buf = raw[b].numpy()
                n = rest.size
                buf[:n] = rest
                view, o, taken, out_bytes, full = memoryview(buf), 0, [], tail_len, False
                while not full:
                    try:
                        blocks, used = bgzf.bgzf_blocks(view[o:n], base + o)
                    except ValueError as e:
                        raise ValueError(f"{name}: {e}") from None
                    used_fit = 0
                    for blk in blocks:
                        if out_bytes + blk.isize > chunk_bytes or len(taken) == MAX_CHUNK_BLOCKS:
                            full = True
                            break
                        taken.append((blk.file_off, o + blk.payload_off, blk.payload_len, out_bytes, blk.isize, blk.crc))
                        out_bytes += blk.isize
                        used_fit = blk.payload_off + blk.payload_len + 8
                    o += used_fit
                    if full or eof:
                        break
                    if n == rawcap:
                        if not taken and not blocks:
                            raise _bgzf_error(name, base, "larger than 64 KiB")      # cannot happen: rawcap > 64 KiB
                        break
                    got = fh.readinto(view[n:min(rawcap, n + RAW_PIECE)])
                    if not got:
                        eof = True
                    n += got or 0
                if eof and not full and o < n:
                    raise _bgzf_error(name, base + o, "truncated")
                if not taken and o < n:
                    raise ValueError(f"{name}: chunk_bytes = {chunk_bytes} is too small for the BGZF block at byte "
                                     f"{base + o} behind a line tail of {tail_len} bytes (a line longer than chunk_bytes?)")
                rest, base = buf[o:n].copy(), base + o
                last = eof and not rest.size
                c += 1
                nb, n_text = len(taken), out_bytes
                if n_text == 0:
                    continue
                if nb:
                    cols = list(zip(*taken))
                    table = K.bgzf_table(cols[1], cols[3], cols[2], cols[4], cols[5], tables[b])
                    with torch.cuda.stream(side):              # comp[b] was last read by chunk c - 2's inflate: main has passed it
                        side.wait_stream(main)
                        comp[b][:o].copy_(raw[b][:o], non_blocking=True)
                        uploaded[b].record(side)
                    main.wait_event(uploaded[b])
                    K.bgzf_inflate(comp[b][:o], table, text[b], res[2:], table_dev)
                    READ_STATS["members_inflated"] += nb
                    if skip:                                   # the header lines in front of the body in its first block
                        text[b][:skip].fill_(10)
                        skip = 0
                    if span_cut and taken[-1][0] == span_cut_off:   # a region's last member: the text behind the span
                        text[b][taken[-1][3] + span_cut:taken[-1][3] + taken[-1][4]].fill_(10)
                    if parser.region is not None:
                        parser.members += [(t[0], t[4]) for t in taken]
                parser.text_base, text_seen = text_seen - tail_len, text_seen + n_text - tail_len
                if last and n_text < chunk_bytes:
                    text[b][n_text:n_text + 1].fill_(10)       # a last line without its newline
                    n_text += 1
                K.text_last_newline(text[b], n_text, res[:2].view(torch.int64))
                host = res[:2 + nb].cpu().numpy()
                for i in np.flatnonzero(host[2:]):
                    raise _bgzf_error(name, taken[int(i)][0], bgzf.STATUS_TEXT.get(int(host[2 + i]), "does not inflate"))
                cut = int(host[:2].view(np.int64)[0]) + 1
                if cut == 0:
                    raise ValueError(f"{name}: a line is longer than chunk_bytes = {chunk_bytes}")
                tail_len = n_text - cut
                if tail_len:                                   # text[b ^ 1] was last read by chunk c - 1's parse, on this stream
                    text[b ^ 1][:tail_len].copy_(text[b][cut:n_text])
                padded = (cut + 15) // 16 * 16
                text[b][cut:padded].fill_(10)
                if deferred is None:
                    try:
                        parser.chunk(text[b], cut, last and not tail_len, parsed[b], main)
                    except (ValueError, OSError, EOFError) as e:   # a BGZF error of a later block comes first (the
                        deferred = e                               # host parser, asked for its error, may meet that block)
            main.wait_stream(side)
            if deferred is not None:
                raise deferred
            return parser.finish()


def write_gt_vcf(path, samples, pos, gt, chrom: str = "1", fmt: str = "GT", extra=None, phased=True,
                 bgzf: bool = False) -> None:
    """A minimal VCF of ``gt`` [n, S, 2] (allele numbers, -1 = '.'): what the tools and tests read back.
    ``fmt`` "GT" writes ``a|b`` cells; a longer FORMAT appends ``extra`` (a string per cell, or one string
    for all) behind the call.  ``.gz`` paths are gzip-compressed: one plain member, or BGZF blocks with ``bgzf``."""
    gt = np.asarray(gt)
    sep = "|" if phased else "/"
    sym = np.array(["."] + [str(i) for i in range(128)])
    opener = gzip.open if str(path).endswith(".gz") else open
    if bgzf:
        from .bgzf import BgzfWriter
        opener = lambda p, mode: BgzfWriter(p)
    with opener(path, "wb") as fh:
        fh.write(b"##fileformat=VCFv4.2\n")
        fh.write(("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n").encode())
        for i in range(len(pos)):
            a, b = sym[gt[i, :, 0] + 1], sym[gt[i, :, 1] + 1]
            cells = np.char.add(np.char.add(a, sep), b)
            if extra is not None:
                cells = np.char.add(cells, extra if isinstance(extra, str) else np.asarray(extra[i]))
            fh.write((f"{chrom}\t{int(pos[i])}\t.\tA\tC\t.\tPASS\t.\t{fmt}\t" + "\t".join(cells.tolist()) + "\n").encode())
