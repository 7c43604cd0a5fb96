"""Opt-in device VCF writer (``--vcf_writer device``): the file ``infer_embedding_rag.write_vcf``
writes, byte for byte, with the records formatted on the GPU (csrc/vcf.hip, ``snvrag_vcf_format``).

The host builds what varies in width — the header and one prefix per selected site (CHROM .. FORMAT),
with the expressions ``write_vcf`` uses — and the byte offset of every line: a cell is 39 bytes plus
its separator, so line i holds ``len(prefix_i) + 40 S`` bytes.  Lines are packed into chunks of at most
``chunk_bytes``; each chunk is formatted into one of two device text buffers, copied to one of two
pinned host buffers on a side stream while the next chunk formats, and written to the file from there.

The fixed width holds for values in [0, 9.9995) only.  The kernel counts every other value (NaN,
infinity, a set sign bit, >= 9.9995); the count is read once per chunk before that chunk's bytes reach
the file, and a nonzero count discards the partial file and lets ``write_vcf`` write the whole of it.

``bgzf=True`` deflates each chunk into BGZF members on the device (csrc/deflate.hip); ``index=True`` also writes
the file's tabix index from the line offsets and the member lengths, without reading the file back.

``milli_f32`` restates the kernel's integer '%.3f' rounding in numpy (checked against Python's own
formatting without a GPU).
"""

from __future__ import annotations

import locale
import os

import numpy as np
import torch

CELL_BYTES = 40                     # "G:h1,h2:gp0,gp1,gp2:ds" = 39 bytes, plus the tab or newline
MAX_CHUNK_BYTES = 1 << 30
DEFAULT_CHUNK_BYTES = 256 << 20
BGZF_BLOCK = 0xff00                 # text bytes per BGZF member of write_vcf_device(bgzf=True)


def milli_f32(values) -> np.ndarray:
    """round-half-even(v * 1000) of the exact binary value of each float32, in integer arithmetic
    (the digits of ``f"{v:.3f}"`` without the point), as int64; -1 where the value does not print as
    d.ddd (NaN, infinity, sign bit set, >= 9.9995).  csrc/vcf.hip ``milli`` is this function."""
    u = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    e = ((u >> np.uint64(23)) & np.uint64(0xff)).astype(np.int64)
    m = (u & np.uint64(0x7fffff)) | np.uint64(0x800000)      # the implicit bit (unused when e == 0)
    P = m * np.uint64(1000)                                  # < 2^34
    s = 150 - e
    zero = (e == 0) | (s >= 35)                              # subnormal, or below 2^-11 < 0.0005
    bad = ((u >> np.uint64(31)) != 0) | (e >= 131)           # negative, -0.0, NaN, inf, >= 16
    sh = np.clip(s, 1, 34).astype(np.uint64)                 # only read where neither zero nor bad
    q = (P >> sh).astype(np.int64)
    r = P & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    q = q + ((r > half) | ((r == half) & ((q & 1) == 1)))
    q = np.where(zero, 0, q)
    return np.where(bad | (q > 9999), -1, q).astype(np.int64)


INFO_HEADER = ('##INFO=<ID=AF,Number=1,Type=Float,Description="Estimated ALT allele frequency (mean haplotype dosage)">\n'
               '##INFO=<ID=DR2,Number=1,Type=Float,Description="Dosage r2 estimated from the genotype probabilities '
               '(Beagle-style)">\n'
               '##INFO=<ID=R2,Number=1,Type=Float,Description="Haplotype-dosage variance over its binomial expectation '
               '(Minimac-style)">\n'
               '##INFO=<ID=IMP,Number=0,Type=Flag,Description="Imputed site">\n')
# with --vcf_sites all --vcf_info (a record per panel site, IMP or TYPED in its INFO): behind INFO_HEADER
TYPED_HEADER = '##INFO=<ID=TYPED,Number=0,Type=Flag,Description="Site genotyped in the target">\n'


def header_lines(samples, info: bool = False, typed: bool = False) -> str:
    """The header ``write_vcf`` writes (same expressions); ``info``: with the four ##INFO lines of ``info=``;
    ``typed``: with the ##INFO line of the TYPED flag (``write_vcf(typed=True)``)."""
    return ("##fileformat=VCFv4.2\n##source=rag-snvbert_amd\n" + (INFO_HEADER if info else "") +
            (TYPED_HEADER if typed else "") +
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype (argmax of GP)">\n'
            '##FORMAT=<ID=HDS,Number=2,Type=Float,Description="Haplotype ALT dosages">\n'
            '##FORMAT=<ID=GP,Number=3,Type=Float,Description="Genotype probabilities">\n'
            '##FORMAT=<ID=DS,Number=1,Type=Float,Description="ALT dosage">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")


def site_prefixes(chrom, pos, pos_flag=None, ref=None, alt=None, encoding=None, info=None, ids=None):
    """(rows int32 [n_lines], blob bytes, prefix_off int32 [n_lines + 1]): the selected site rows
    (``pos_flag`` as ``write_vcf`` reads it) and their line prefixes — everything ``write_vcf`` puts in
    front of the first cell, the tab included — concatenated.  ``info``: the INFO string of every site row
    (``write_vcf(info=...)``), '.' without it; ``ids``: the ID string of every site row, '.' without it."""
    encoding = encoding or locale.getpreferredencoding(False)      # what open(path, "w") encodes with
    rows, parts, off = [], [], [0]
    for i in range(len(pos)):
        if pos_flag is not None and not pos_flag[i]:
            continue
        r = ref[i] if ref is not None else "."
        a = alt[i] if alt is not None else "."
        inf = info[i] if info is not None else "."
        d = ids[i] if ids is not None else "."
        b = f"{chrom}\t{int(pos[i])}\t{d}\t{r}\t{a}\t0.0\tPASS\t{inf}\tGT:HDS:GP:DS\t".encode(encoding)
        rows.append(i)
        parts.append(b)
        off.append(off[-1] + len(b))
    if off[-1] >= 1 << 31:
        raise ValueError("the line prefixes exceed 2^31 bytes")
    return np.asarray(rows, np.int32), b"".join(parts), np.asarray(off, np.int32)


def line_lengths(prefix_off, n_samples: int) -> np.ndarray:
    """Bytes of every line: its prefix and 40 per sample (the last cell's separator is the newline)."""
    return np.diff(np.asarray(prefix_off, np.int64)) + CELL_BYTES * int(n_samples)


def plan_chunks(line_len, chunk_bytes: int):
    """[(first line, end line)] of consecutive lines packed greedily into chunks of at most
    ``chunk_bytes`` of text.  ValueError: chunk_bytes above 1 GiB or a line longer than chunk_bytes."""
    if chunk_bytes > MAX_CHUNK_BYTES:
        raise ValueError(f"chunk_bytes {chunk_bytes} exceeds 1 GiB")
    line_len = np.asarray(line_len, np.int64)
    if line_len.size and int(line_len.max()) > chunk_bytes:
        raise ValueError(f"a line of {int(line_len.max())} bytes does not fit chunk_bytes {chunk_bytes}")
    end = np.cumsum(line_len)
    chunks, lo, base = [], 0, 0
    while lo < line_len.size:
        hi = int(np.searchsorted(end, base + chunk_bytes, side="right"))     # lines [lo, hi) fit
        chunks.append((lo, hi))
        lo, base = hi, int(end[hi - 1])
    return chunks


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_vcf_device(path, chrom, pos, h1, h2, gt, samples, pos_flag=None, ref=None, alt=None, device=None,
                     chunk_bytes: int = DEFAULT_CHUNK_BYTES, bgzf: bool = False, info=None, index: bool = False,
                     ids=None, typed: bool = False) -> bool:
    """``write_vcf`` with the records formatted on ``device``: the same file, byte for byte.

    ``bgzf``: the file is bgzipped.  Each chunk's text is deflated into BGZF members of 0xff00 bytes and packed
    on the device behind the format kernel (csrc/deflate.hip); its byte total is read with the chunk's count of
    bad values, and only that many bytes cross to the host and reach the file.  Chunks are independent (a
    chunk's last member is short); the header is written as host-made members and the file ends with the EOF
    block.  It inflates to the plain file byte for byte; the fallback below then writes a bgzipped file too.

    ``info``: one INFO string per site row, as ``write_vcf(info=...)``: it takes the place of '.' in the line
    prefixes (host-built, of any width) and adds the four ##INFO header lines.  ``ids`` / ``ref`` / ``alt``: one
    string per site row for the ID, REF and ALT columns, as ``write_vcf`` takes them ('.' without).  ``typed``: the
    header also declares the TYPED flag, as ``write_vcf(typed=True)``; no record changes.

    ``index`` (needs ``bgzf``): also write the tabix index ``path + ".tbi"`` (dataset/tbi.py) without reading the
    file back.  The byte offset of every line in its chunk's text is known on the host; each chunk's member lengths
    (4 bytes per 0xff00 bytes of text) cross with its packed bytes, on the same stream and event, and a prefix sum
    over them turns the line offsets into virtual offsets.  A position >= 2^29 raises ``ValueError`` before
    anything is written; the fallback below removes the partial file and the host writer writes both files.

    h1 / h2 [n, S] and gt [n, S, 4] are float32 numpy arrays, host tensors or device tensors.  Device
    tensors are formatted in place; host arrays are uploaded one chunk of selected rows at a time.
    Returns True when the device text was written; False when a value did not fit the fixed-width cell
    (NaN, infinity, negative or -0.0, >= 9.9995) and the host writer wrote the file instead."""
    from . import kernels as K
    from .infer_embedding_rag import write_vcf
    if not torch.cuda.is_available():
        raise RuntimeError("write_vcf_device needs a HIP device (the host writer is write_vcf)")
    for name, a in (("h1", h1), ("h2", h2), ("gt", gt)):
        if not (a.dtype == torch.float32 if torch.is_tensor(a) else np.asarray(a).dtype == np.float32):
            raise TypeError(f"{name} must be float32")
    on_device = all(torch.is_tensor(a) and a.is_cuda for a in (h1, h2, gt))
    if on_device:
        dev = h1.device
        h1, h2, gt = h1.contiguous(), h2.contiguous(), gt.contiguous()
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        h1, h2, gt = _host(h1), _host(h2), _host(gt)
    n, S = h1.shape
    if h2.shape != (n, S) or gt.shape != (n, S, 4) or len(samples) != S or len(pos) != n:
        raise ValueError("h1 / h2 [n, S], gt [n, S, 4], pos [n] and samples [S] do not agree")
    if info is not None and len(info) != n:
        raise ValueError("info must hold one string per site row")
    flag = None if pos_flag is None else _host(pos_flag)
    if index:
        if not bgzf:
            raise ValueError("index=True needs bgzf=True: a .tbi indexes a bgzipped file")
        from .dataset import tbi
        beg, end = tbi.vcf_intervals(pos, flag, ref)
    rows, blob, prefix_off = site_prefixes(chrom, pos, flag, ref, alt, info=info, ids=ids)
    length = line_lengths(prefix_off, S)
    chunks = plan_chunks(length, chunk_bytes)
    if bgzf:
        from .dataset.bgzf import EOF_BLOCK, write_bgzf
        with open(path, "wb") as f:
            write_bgzf(f, header_lines(samples, info is not None, typed).encode(locale.getpreferredencoding(False)),
                       eof=not chunks)
    else:
        with open(path, "w") as f:
            f.write(header_lines(samples, info is not None, typed))
    if not chunks:
        if index:
            tbi.build([], [], [], [], [], []).write(str(path) + ".tbi")
        return True

    cap = max(int(length[lo:hi].sum()) for lo, hi in chunks)
    blob_np = np.frombuffer(blob, np.uint8).copy()
    with torch.cuda.device(dev):
        main, side = torch.cuda.current_stream(), torch.cuda.Stream()
        text = [torch.empty(cap + 16, device=dev, dtype=torch.uint8) for _ in range(2)]
        slots = -(-cap // BGZF_BLOCK)                  # members per chunk, at most; each at most BGZF_BLOCK + 31 bytes
        pinned = [torch.empty(slots * (BGZF_BLOCK + 31) if bgzf else cap, dtype=torch.uint8).pin_memory()
                  for _ in range(2)]
        bad = torch.zeros(2, device=dev, dtype=torch.int32)
        bad_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        copied = [torch.cuda.Event(), torch.cuda.Event()]
        if bgzf:
            members = [torch.empty(slots, K.BGZF_SLOT, device=dev, dtype=torch.uint8) for _ in range(2)]
            member_len = [torch.empty(slots, device=dev, dtype=torch.int32) for _ in range(2)]
            packed = [torch.empty(slots * (BGZF_BLOCK + 31), device=dev, dtype=torch.uint8) for _ in range(2)]
            small = torch.zeros(2, 4, device=dev, dtype=torch.int32)     # per buffer: bad count, -, total (i64)
            small_host = torch.zeros(2, 4, dtype=torch.int32).pin_memory()
            counted, totals = [torch.cuda.Event(), torch.cuda.Event()], [0, 0]
        if index:
            mlen_host = [torch.zeros(slots, dtype=torch.int32).pin_memory() for _ in range(2)]
            file_off, v_beg = [os.path.getsize(path)], []     # of the next chunk's first member; per chunk, of its lines
        ok = True
        with open(path, "ab") as f:

            def finish(c):
                """Chunk c has left the device: its count first, then its bytes to the file."""
                b = c & 1
                copied[b].synchronize()
                if bgzf:                               # start_copy saw its count
                    f.write(memoryview(pinned[b].numpy())[:totals[b]])
                    if index:
                        lo, hi = chunks[c]
                        text_off = np.concatenate([[0], np.cumsum(length[lo:hi])])
                        nm = -(-int(text_off[-1]) // BGZF_BLOCK)
                        mlen = mlen_host[b].numpy()[:nm].astype(np.int64)
                        assert int(mlen.sum()) == totals[b], "the member lengths of a chunk do not add up to its bytes"
                        member_off = file_off[0] + np.cumsum(mlen) - mlen
                        v_beg.append(member_off[text_off[:-1] // BGZF_BLOCK] << 16 | text_off[:-1] % BGZF_BLOCK)
                        file_off[0] += totals[b]
                    return True
                if int(bad_host[b]) != 0:
                    return False
                lo, hi = chunks[c]
                f.write(memoryview(pinned[b].numpy())[:int(length[lo:hi].sum())])
                return True

            def start_copy(c):
                """bgzf: chunk c's count and byte total have arrived; its members follow, that many bytes."""
                b = c & 1
                counted[b].synchronize()
                if int(small_host[b, 0]) != 0:
                    return False
                totals[b] = int(small_host[b, 2:4].view(torch.int64))
                assert 0 <= totals[b] <= packed[b].numel(), "the members of a chunk exceed their bound"
                with torch.cuda.stream(side):
                    pinned[b][:totals[b]].copy_(packed[b][:totals[b]], non_blocking=True)
                    if index:
                        lo, hi = chunks[c]
                        nm = -(-int(length[lo:hi].sum()) // BGZF_BLOCK)
                        mlen_host[b][:nm].copy_(member_len[b][:nm], non_blocking=True)
                    copied[b].record(side)
                return True

            for c, (lo, hi) in enumerate(chunks):
                b = c & 1
                nbytes = int(length[lo:hi].sum())
                line_off = np.concatenate([[0], np.cumsum(length[lo:hi])]).astype(np.int64)
                p_off = (prefix_off[lo:hi + 1] - prefix_off[lo]).astype(np.int32)
                p_blob = blob_np[int(prefix_off[lo]):int(prefix_off[hi])]
                if on_device:
                    a1, a2, ag, r = h1, h2, gt, rows[lo:hi]
                else:                                  # this chunk's rows only, gathered: row i of the upload = line i
                    sel = rows[lo:hi]
                    a1, a2, ag = (torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev) for a in (h1, h2, gt))
                    r = np.arange(hi - lo, dtype=np.int32)
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                count = small[b, 0:1] if bgzf else bad[b:b + 1]
                count.zero_()
                # text[b] / pinned[b] last held chunk c - 2, which finish() saw copied and wrote out
                K.vcf_format(a1, a2, ag, up(r), up(line_off), up(p_off), up(p_blob), text[b], nbytes, count)
                if bgzf:
                    mem, mlen = K.bgzf_deflate(text[b], nbytes, BGZF_BLOCK, members[b], member_len[b])
                    K.bgzf_pack(mem, mlen, packed[b], small[b, 2:4].view(torch.int64))
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    if bgzf:
                        small_host[b].copy_(small[b], non_blocking=True)
                        counted[b].record(side)
                    else:
                        bad_host[b:b + 1].copy_(bad[b:b + 1], non_blocking=True)
                        pinned[b][:nbytes].copy_(text[b][:nbytes], non_blocking=True)
                        copied[b].record(side)
                if c >= 1 and not finish(c - 1):       # overlaps chunk c's format and copy
                    ok = False
                    break
                if bgzf and not start_copy(c):
                    ok = False
                    break
            if ok:
                ok = finish(len(chunks) - 1)
            if ok and bgzf:
                f.write(EOF_BLOCK)
        main.wait_stream(side)                         # the buffers go back to the allocator behind the copies
        torch.cuda.synchronize(dev)
    if ok:
        if index:                                      # a line ends where the next begins; the last at the EOF block
            v = np.concatenate(v_beg + [[file_off[0] << 16]]).astype(np.uint64)
            tbi.build([str(chrom)], np.zeros(v.size - 1, np.int64), beg, end, v[:-1], v[1:]).write(str(path) + ".tbi")
        return True
    os.remove(path)
    print("write_vcf_device: a value does not fit the fixed-width cell (NaN, infinite, negative or >= 9.9995); "
          "the host writer writes the file", flush=True)
    write_vcf(path, chrom, pos, _host(h1), _host(h2), _host(gt), samples, pos_flag=flag, ref=ref, alt=alt, bgzf=bgzf,
              info=info, index=index, ids=ids, typed=typed)
    return False
