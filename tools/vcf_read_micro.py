"""The VCF readers on the same seeded files in one process (GPU only).

  python tools/vcf_read_micro.py [SITESxSAMPLES]      default 4096x2000
  python tools/vcf_read_micro.py --inflate [SITESxSAMPLES]     the BGZF twins: host zlib against the device inflate
  python tools/vcf_read_micro.py --columns [SITESxSAMPLES]     read_vcf with and without columns=True, and its kernels

Writes a GT-only file (every line fixed-width) and a GT:DS:GP file (every line on the general path) from
seeded 0/1 arrays into a local temporary directory, then times

  parse_vcf_host   on the first HOST_LINES records, extrapolated to the file (labelled so);
  read_vcf         end to end for .vcf and .vcf.gz (a host clock around the call; it ends synchronised),
                   beside the file read (and inflate) alone, streamed in the same pieces, and the pinned
                   host-to-device copy of the same bytes alone;
  the kernels      line index, parse (fixed-width and general path) and pack rows by device events around
                   REPS launches on one resident chunk.

Text GB/s = bytes of the text the kernel reads per second of kernel time; beside it a device-to-device
copy of 400 MB measured here (read + write bytes per second) and the HBM peak of the datasheet (8 TB/s).
Every device path is warmed on the same shapes first."""
import gzip
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")
HOST_LINES, REPS, HBM_PEAK_TBS = 64, 20, 8.0


def events_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stream_read_s(path, piece):
    from src.dataset.vcf_reader import _open
    buf = bytearray(piece)
    t0 = time.perf_counter()
    with _open(path) as fh:
        while fh.readinto(buf):
            pass
    return time.perf_counter() - t0


def body_chunk(path):
    """The body of the file as one padded device chunk (text, nbytes)."""
    with open(path, "rb") as fh:
        data = fh.read()
    body = data[data.index(b"\n", data.index(b"#CHROM")) + 1:]
    buf = np.full((len(body) + 15) // 16 * 16, 10, np.uint8)
    buf[:len(body)] = np.frombuffer(body, np.uint8)
    return torch.from_numpy(buf).to(DEV), len(body)


def kernels(path, n, S, label):
    from src import kernels as K
    text, nbytes = body_chunk(path)
    line_off, n_lines = K.vcf_line_index(text, nbytes, n)
    assert int(n_lines) == n
    ld = (S + 3) // 4 * 4
    codes = torch.empty(n, ld, device=DEV, dtype=torch.uint8)
    ldb = ((n + 7) // 8 + 7) // 8 * 8
    alt = torch.empty(2 * S, ldb, device=DEV, dtype=torch.uint8)
    miss = torch.empty_like(alt)
    gbs = lambda ms: nbytes / ms / 1e6
    t = events_ms(lambda: K.vcf_line_index(text, nbytes, n))
    print(f"  {label}: line index      {t:8.3f} ms   {gbs(t):8.1f} text GB/s   ({nbytes / 1e6:.1f} MB, {n} lines)")
    for force, name in ((False, "parse as written"), (True, "parse forced general")):
        t = events_ms(lambda: K.vcf_parse_gt(text, nbytes, line_off, n, S, codes, force))
        print(f"  {label}: {name:<20} {t:8.3f} ms   {gbs(t):8.1f} text GB/s")
    t = events_ms(lambda: K.vcf_pack_rows(codes, n, S, alt, miss))
    print(f"  {label}: pack rows       {t:8.3f} ms   {n * S / t / 1e6:8.1f} code GB/s   ({n * S / 1e6:.1f} MB of codes)")


def inflate_arm(files, n, S, gt):
    """BGZF twins (0xff00-byte blocks, level 6): read_vcf with inflate="host" first (the default path), then
    "device", alternating for ROUNDS rounds; then the stages of the device path alone."""
    from src import kernels as K
    from src.dataset import bgzf, vcf_reader as V
    ROUNDS = 4
    for k, path in files.items():
        p = path + ".bgzf.gz"
        with open(path, "rb") as fh:
            text = fh.read()
        bgzf.write_bgzf(p, text)
        best = {"host": None, "device": None}
        for mode in ("host", "device"):
            V.read_vcf(p, DEV, inflate=mode)                     # warm
        for _ in range(ROUNDS):
            for mode in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                vg = V.read_vcf(p, DEV, inflate=mode)
                dt = time.perf_counter() - t0
                best[mode] = dt if best[mode] is None else min(best[mode], dt)
                assert vg.n_sites == n
        assert (vg.gt() == gt).all()
        size = os.path.getsize(p)
        print(f"read_vcf {k:<8} BGZF {size / 1e6:7.1f} MB on disk, {len(text) / 1e6:7.1f} MB of text: inflate=host "
              f"{best['host']:.3f} s, inflate=device {best['device']:.3f} s (best of {ROUNDS}, alternating)")
        t0 = time.perf_counter()
        with open(p, "rb") as fh:
            raw = fh.read()
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        blocks, used = bgzf.bgzf_blocks(raw)
        t_walk = time.perf_counter() - t0
        assert used == len(raw)
        out_off = np.cumsum([0] + [b.isize for b in blocks])
        table = K.bgzf_table([b.payload_off for b in blocks], out_off[:-1], [b.payload_len for b in blocks],
                             [b.isize for b in blocks], [b.crc for b in blocks])
        pin = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        comp = torch.empty(len(raw), device=DEV, dtype=torch.uint8)
        t_up = events_ms(lambda: comp.copy_(pin, non_blocking=True), 5)
        out = torch.empty((len(text) + 15) // 16 * 16, device=DEV, dtype=torch.uint8)
        st = K.bgzf_inflate(comp, table, out)
        assert not st.any().item() and bytes(out[:len(text)].cpu().numpy()) == text
        status, tdev = torch.empty(len(blocks), device=DEV, dtype=torch.int32), torch.empty(len(blocks), 4, device=DEV, dtype=torch.int64)
        t_inf = events_ms(lambda: K.bgzf_inflate(comp, table, out, status, tdev))
        one = max(range(len(blocks)), key=lambda i: blocks[i].payload_len)       # the block with the most input
        t_one = events_ms(lambda: K.bgzf_inflate(comp, table[one:one + 1].contiguous(), out, status, tdev))
        nl = torch.empty(1, device=DEV, dtype=torch.int64)
        t_nl = events_ms(lambda: K.text_last_newline(out, len(text), nl))
        print(f"  {k}: file read {t_read * 1e3:.2f} ms, header walk of {len(blocks)} blocks {t_walk * 1e3:.2f} ms, pinned upload "
              f"{t_up:.3f} ms, inflate + CRC kernel {t_inf:.3f} ms = {len(text) / t_inf / 1e6:.1f} text GB/s out, "
              f"{len(raw) / t_inf / 1e6:.2f} GB/s in (the CRC is folded into the kernel), the block with the most input ({blocks[one].payload_len} -> "
              f"{blocks[one].isize} bytes) alone {t_one:.3f} ms, last newline {t_nl:.3f} ms")


def columns_arm(path, n, S):
    """read_vcf of the GT file with columns=False and columns=True, alternating for ROUNDS rounds (min / median /
    max: the spread is the run-to-run noise a difference has to exceed); then, on the file's body as one resident
    chunk, the two site-column kernels and the scan between them beside snvrag_vcf_parse_gt.  On a build whose
    read_vcf has no ``columns`` only the columns=False rows are printed (the same rows, for a comparison)."""
    import inspect
    from src import kernels as K
    from src.dataset import vcf_reader as V
    ROUNDS = 7
    modes = [False] + ([True] if "columns" in inspect.signature(V.read_vcf).parameters else [])
    read = lambda m: V.read_vcf(path, DEV, **({"columns": True} if m else {}))
    times = {m: [] for m in modes}
    for m in modes:
        read(m)                                                  # warm
    for _ in range(ROUNDS):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vg = read(m)
            times[m].append(time.perf_counter() - t0)
            assert vg.n_sites == n
    size = os.path.getsize(path)
    for m in modes:
        t = sorted(times[m])
        print(f"read_vcf columns={m!s:<5} {size / 1e6:7.1f} MB of text, {n} x {S}: min {t[0]:.4f} s, median "
              f"{t[len(t) // 2]:.4f} s, max {t[-1]:.4f} s over {ROUNDS} alternating rounds")
    if len(modes) == 1:
        print("this build's read_vcf has no columns=: nothing else to time")
        return
    with open(path, "rb") as fh:
        head = b"".join(fh.readline() for _ in range(2 + HOST_LINES))
    want = V.site_columns_host(head)
    for name in V.COLUMN_NAMES:
        assert vg.columns.column(name)[:HOST_LINES] == want.column(name), name
    assert len(vg.columns) == n
    over = sorted(times[True])[ROUNDS // 2] - sorted(times[False])[ROUNDS // 2]
    print(f"columns=True costs {over * 1e3:+.2f} ms at the median ({100 * over / sorted(times[False])[ROUNDS // 2]:+.1f} %); "
          f"the spread of columns=False alone is {(max(times[False]) - min(times[False])) * 1e3:.2f} ms")
    text, nbytes = body_chunk(path)
    line_off, n_lines = K.vcf_line_index(text, nbytes, n)
    codes = torch.empty(n, (S + 3) // 4 * 4, device=DEV, dtype=torch.uint8)
    t_parse = events_ms(lambda: K.vcf_parse_gt(text, nbytes, line_off, n, S, codes))
    spans = K.vcf_cols_span(text, nbytes, line_off, n)
    t_span = events_ms(lambda: K.vcf_cols_span(text, nbytes, line_off, n, out=spans))
    off = torch.zeros(4 * n + 1, device=DEV, dtype=torch.int64)

    def scan():
        torch.cumsum(spans[:, 1::2].t().reshape(-1).to(torch.int64), 0, out=off[1:])
    t_scan = events_ms(scan)
    blob = torch.empty(max(int(off[-1].item()), 16), device=DEV, dtype=torch.uint8)
    t_gather = events_ms(lambda: K.vcf_cols_gather(text, nbytes, spans, off, blob))
    print(f"  one chunk of {nbytes / 1e6:.1f} MB, {n} lines: snvrag_vcf_parse_gt {t_parse:.3f} ms, snvrag_vcf_cols_span "
          f"{t_span:.3f} ms, the scan of the lengths (torch) {t_scan:.3f} ms, snvrag_vcf_cols_gather {t_gather:.3f} ms "
          f"({int(off[-1].item())} bytes of strings)")


def main():
    from src.dataset import vcf_reader as V
    inflate = "--inflate" in sys.argv
    if inflate:
        sys.argv.remove("--inflate")
    columns = "--columns" in sys.argv
    if columns:
        sys.argv.remove("--columns")
    n, S = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "4096x2000").lower().split("x"))
    rng = np.random.default_rng(0)
    gt = (rng.random((n, S, 2)) < 0.2).astype(np.int8)
    pos = (np.cumsum(rng.integers(1, 2000, n)) + 10_000_000).astype(np.int32)
    names = [f"S{i}" for i in range(S)]
    print(f"device: {torch.cuda.get_device_name(0)}; {n} sites x {S} samples = {n * S / 1e6:.1f} M cells")
    x = torch.empty(400 << 20, device=DEV, dtype=torch.uint8)
    y = torch.empty_like(x)
    t = events_ms(lambda: y.copy_(x))
    print(f"device copy of 400 MB: {2 * x.numel() / t / 1e9:.2f} TB/s read + write (datasheet HBM peak {HBM_PEAK_TBS} TB/s)")
    del x, y
    with tempfile.TemporaryDirectory() as d:
        files = {"GT": os.path.join(d, "gt.vcf"), "GT:DS:GP": os.path.join(d, "gp.vcf")}
        V.write_gt_vcf(files["GT"], names, pos, gt)
        V.write_gt_vcf(files["GT:DS:GP"], names, pos, gt, fmt="GT:DS:GP", extra=":1.25:0.100,0.650,0.250")
        if inflate:
            inflate_arm(files, n, S, gt)
            return
        if columns:
            columns_arm(files["GT"], n, S)
            return
        for k in list(files):
            with open(files[k], "rb") as src, gzip.open(files[k] + ".gz", "wb", compresslevel=6) as dst:
                dst.write(src.read())
        # host specification on a slice, extrapolated
        with open(files["GT"], "rb") as fh:
            head = b"".join(fh.readline() for _ in range(2 + HOST_LINES))
        t0 = time.perf_counter()
        V.parse_vcf_host(head)
        th = (time.perf_counter() - t0) / (HOST_LINES * S)
        print(f"parse_vcf_host: {th * 1e6:.3f} us per cell on {HOST_LINES} records; EXTRAPOLATED to the file: "
              f"{th * n * S:.1f} s")
        pin = torch.empty(os.path.getsize(files["GT"]), dtype=torch.uint8).pin_memory()
        dst = torch.empty(pin.numel(), device=DEV, dtype=torch.uint8)
        t = events_ms(lambda: dst.copy_(pin, non_blocking=True), 5)
        print(f"pinned upload of {pin.numel() / 1e6:.1f} MB: {pin.numel() / t / 1e6:.1f} GB/s")
        del pin, dst
        for k, path in files.items():
            for p in (path, path + ".gz"):
                size = os.path.getsize(p)
                text_bytes = os.path.getsize(path)
                V.read_vcf(p, DEV)                                   # warm: code objects, the page cache
                best, vg = None, None
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    vg = V.read_vcf(p, DEV)
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                tr = min(stream_read_s(p, V.DEFAULT_CHUNK_BYTES) for _ in range(3))
                assert vg.n_sites == n and not vg.any_missing
                print(f"read_vcf {k:<8} {os.path.basename(p):<10} {size / 1e6:8.1f} MB on disk, {text_bytes / 1e6:8.1f} MB of "
                      f"text: {best:7.3f} s end to end = {best / (n * S) * 1e6:.4f} us per cell, {text_bytes / best / 1e9:.2f} "
                      f"text GB/s; file read{' + inflate' if p.endswith('.gz') else ''} alone {tr:.3f} s "
                      f"({100 * tr / best:.0f} % of it)")
            got = vg.gt()
            assert (got == gt).all(), "read_vcf differs from the arrays written"
        for k, path in files.items():
            kernels(path, n, S, k)


if __name__ == "__main__":
    main()
