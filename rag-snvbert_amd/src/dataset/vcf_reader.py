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

Not covered: inflate on the device, a rank reading only its shard's sample columns, multi-allelic
splitting (any allele number > 0 is ALT), REF / ALT / ID strings, h5 files.
"""

from __future__ import annotations

import gzip
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


def parse_vcf_host(path_or_bytes: Union[str, os.PathLike, bytes]):
    """(samples, pos int32 [n], gt int8 [n, S, 2]) of a VCF given by path (``.gz`` by its magic bytes) or
    as bytes: allele numbers (capped at 127), -1 for missing, as ``allel.read_vcf`` documents
    ``calldata/GT``.  The specification of ``read_vcf``; ``ValueError`` names the 1-based file line."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        name, data = "<bytes>", bytes(path_or_bytes)
        if data[:2] == b"\x1f\x8b":
            data = gzip.decompress(data)
    else:
        name = str(path_or_bytes)
        with _open(path_or_bytes) as fh:
            data = fh.read()
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


def read_vcf(path, device, chunk_bytes: int = DEFAULT_CHUNK_BYTES, force_general: bool = False) -> VcfGenotypes:
    """POS and GT of the VCF at ``path`` (``.gz`` / BGZF inflated on the host, streaming), the body
    parsed on ``device``.  ``force_general`` sends every line through the general parse path (same
    result).  ``ValueError``: what ``parse_vcf_host`` raises for the file, or a line longer than
    ``chunk_bytes``."""
    import torch
    from .. import kernels as K
    from .. import native as N
    N.require_gpu()
    if not 64 <= chunk_bytes <= MAX_CHUNK_BYTES:
        raise ValueError(f"chunk_bytes must be in [64, {MAX_CHUNK_BYTES}]")
    name, dev = str(path), torch.device(device)
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
        S = len(samples)
        ld_codes = (S + 3) // 4 * 4
        # a record holds at least 8 one-byte columns, GT and S one-byte cells, each with its separator
        max_lines = chunk_bytes // (2 * S + 17) + 1
        cap = (chunk_bytes + 15) // 16 * 16
        pos_parts, flag_parts, alt_parts, miss_parts = [], [], [], []
        n_records = 0
        with torch.cuda.device(dev):
            main, side = torch.cuda.current_stream(), torch.cuda.Stream()
            pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
            text = [torch.empty(cap, device=dev, dtype=torch.uint8) for _ in range(2)]
            uploaded = [torch.cuda.Event(), torch.cuda.Event()]
            parsed = [torch.cuda.Event(), torch.cuda.Event()]
            codes = torch.empty(max_lines + 64, ld_codes, device=dev, dtype=torch.uint8)
            carry, tail, eof, c = 0, b"", False, 0
            while not eof or tail:
                b = c & 1
                buf = pinned[b].numpy()                      # chunk c - 2 left it: its parse was waited for below
                n = len(tail)
                buf[:n] = np.frombuffer(tail, np.uint8)
                view = memoryview(buf)
                while n < chunk_bytes:
                    got = fh.readinto(view[n:chunk_bytes])
                    if not got:
                        eof = True
                        break
                    n += got
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
                line_off, n_lines = K.vcf_line_index(text[b], cut, max_lines)
                nl = int(n_lines.item())                       # also: pinned[b] has left the host
                if nl > max_lines:                             # a line shorter than any record
                    parse_vcf_host(path)
                    raise ValueError(f"{name}: a body line is shorter than a record of {S} samples")
                if nl:
                    p, f = K.vcf_parse_gt(text[b], cut, line_off, nl, S, codes[carry:], force_general)
                    pos_parts.append(p)
                    flag_parts.append(f)
                parsed[b].record(main)
                total = carry + nl
                full = total if eof and not tail else total // 64 * 64
                if full:
                    ld = ((full + 7) // 8 + 7) // 8 * 8
                    alt = torch.empty(2 * S, ld, device=dev, dtype=torch.uint8)
                    miss = torch.empty(2 * S, ld, device=dev, dtype=torch.uint8)
                    K.vcf_pack_rows(codes, full, S, alt, miss)
                    alt_parts.append(alt[:, :(full + 7) // 8])
                    miss_parts.append(miss[:, :(full + 7) // 8])
                    carry = total - full
                    if carry:                                  # fewer than 64 <= full rows: no overlap
                        codes[:carry].copy_(codes[full:total])
                else:
                    carry = total
                n_records += nl
            if carry:                                          # the file ended in an empty chunk
                ld = ((carry + 7) // 8 + 7) // 8 * 8
                alt = torch.empty(2 * S, ld, device=dev, dtype=torch.uint8)
                miss = torch.empty(2 * S, ld, device=dev, dtype=torch.uint8)
                K.vcf_pack_rows(codes, carry, S, alt, miss)
                alt_parts.append(alt[:, :(carry + 7) // 8])
                miss_parts.append(miss[:, :(carry + 7) // 8])
            main.wait_stream(side)
            if n_records:
                flags = torch.cat(flag_parts).cpu().numpy().view(np.uint32)
                pos = torch.cat(pos_parts).cpu().numpy()
                alt_bits = torch.cat(alt_parts, 1).contiguous()
                miss_bits = torch.cat(miss_parts, 1).contiguous()
            else:
                flags, pos = np.zeros(0, np.uint32), np.zeros(0, np.int32)
                alt_bits = torch.zeros(2 * S, 0, device=dev, dtype=torch.uint8)
                miss_bits = torch.zeros(2 * S, 0, device=dev, dtype=torch.uint8)
            torch.cuda.synchronize(dev)
    bad = np.flatnonzero(flags & np.uint32(FLAG_ERRORS | FLAG_OFFSET))
    if bad.size:
        r = int(bad[0])
        if int(flags[r]) & FLAG_OFFSET:
            raise RuntimeError(f"{name}: record {r}: the line index gave an offset outside its chunk")
        raise flag_error(name, _record_line(path, r), int(flags[r]) & FLAG_ERRORS)
    seen = int(np.bitwise_or.reduce(flags >> np.uint32(8))) if flags.size else 0
    return VcfGenotypes(samples, pos.astype(np.int32, copy=False), alt_bits, miss_bits, n_records,
                        bool(seen & (CODE_MISS1 | CODE_MISS2)), not seen & CODE_SLASH)


def write_gt_vcf(path, samples, pos, gt, chrom: str = "1", fmt: str = "GT", extra=None, phased=True) -> None:
    """A minimal VCF of ``gt`` [n, S, 2] (allele numbers, -1 = '.'): what the tools and tests read back.
    ``fmt`` "GT" writes ``a|b`` cells; a longer FORMAT appends ``extra`` (a string per cell, or one string
    for all) behind the call.  ``.gz`` paths are gzip-compressed."""
    gt = np.asarray(gt)
    sep = "|" if phased else "/"
    sym = np.array(["."] + [str(i) for i in range(128)])
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wb") as fh:
        fh.write(b"##fileformat=VCFv4.2\n")
        fh.write(("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n").encode())
        for i in range(len(pos)):
            a, b = sym[gt[i, :, 0] + 1], sym[gt[i, :, 1] + 1]
            cells = np.char.add(np.char.add(a, sep), b)
            if extra is not None:
                cells = np.char.add(cells, extra if isinstance(extra, str) else np.asarray(extra[i]))
            fh.write((f"{chrom}\t{int(pos[i])}\t.\tA\tC\t.\tPASS\t.\t{fmt}\t" + "\t".join(cells.tolist()) + "\n").encode())
