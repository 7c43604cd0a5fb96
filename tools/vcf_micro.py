"""The two VCF writers on the same arrays in one process (GPU only).

  python tools/vcf_micro.py [SITESxSAMPLES]      default 2000x10000

Per writer: microseconds per cell (site and sample) for the complete file, written to a local temporary
directory — the host ``write_vcf`` (the Python loop), ``write_vcf_device`` from host arrays (upload path)
and from device arrays (in place).  For the device writer also the kernel alone: device events around
the launches of every chunk, no copy, against the 72 bytes per cell it moves and a device copy of 400 MB
(tools/bw_micro.py's figure) measured here.  The files are compared as bytes.

Times: a host clock around each complete write (it ends with the file closed); device events around the
kernel launches.  The device paths are warmed on a small shape first."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")


def make(n, S, seed=0):
    rng = np.random.default_rng(seed)
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    gt = rng.random((n, S, 4), dtype=np.float32)
    gt /= gt.sum(-1, keepdims=True)
    pos = np.cumsum(rng.integers(1, 2000, n)).astype(np.int64) + 10_000_000
    return h1, h2, gt, pos, [f"S{i}" for i in range(S)]


def kernel_only(h1, h2, gt, pos, S, reps):
    """ms per pass over every chunk's launch (arguments uploaded before the timed window)."""
    from src import kernels as K
    from src import vcf_device as V
    rows, blob, p_off = V.site_prefixes("21", pos)
    length = V.line_lengths(p_off, S)
    chunks = V.plan_chunks(length, V.DEFAULT_CHUNK_BYTES)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    text = torch.empty(max(int(length[lo:hi].sum()) for lo, hi in chunks) + 16, device=DEV, dtype=torch.uint8)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    blob = np.frombuffer(blob, np.uint8).copy()
    args = []
    for lo, hi in chunks:
        line_off = np.concatenate([[0], np.cumsum(length[lo:hi])]).astype(np.int64)
        args.append((up(rows[lo:hi]), up(line_off), up((p_off[lo:hi + 1] - p_off[lo]).astype(np.int32)),
                     up(blob[int(p_off[lo]):int(p_off[hi])]), int(length[lo:hi].sum())))

    def once():
        for r, lo_, po, pb, nb in args:
            K.vcf_format(h1, h2, gt, r, lo_, po, pb, text, nb, bad)

    once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        once()
    b.record()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    return a.elapsed_time(b) / reps, len(chunks), int(length.sum())


def copy_tbs():
    x = torch.empty(400 << 20, device=DEV, dtype=torch.uint8).fill_(1)
    y = torch.empty_like(x)
    y.copy_(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    return 2 * (400 << 20) / (a.elapsed_time(b) / 20 * 1e-3) / 1e12


def copy_and_file_gbs(tmp, nbytes):
    """What the complete write does besides the kernel, each alone on one chunk's bytes: the device-to-host
    copy into a pinned buffer (device events) and the file write from that buffer (host clock, closed file)."""
    text = torch.empty(nbytes, device=DEV, dtype=torch.uint8).fill_(65)
    pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    pinned.copy_(text)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        pinned.copy_(text, non_blocking=True)
    b.record()
    torch.cuda.synchronize()
    d2h = nbytes / (a.elapsed_time(b) / 3 * 1e-3) / 1e9
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        with open(os.path.join(tmp, "raw.bin"), "wb") as f:
            f.write(memoryview(pinned.numpy()))
        ts.append(time.perf_counter() - t0)
    os.remove(os.path.join(tmp, "raw.bin"))
    return d2h, nbytes / min(ts) / 1e9


def main():
    from src.infer_embedding_rag import write_vcf, write_vcf_device
    shape = sys.argv[1] if len(sys.argv) > 1 else "2000x10000"
    n, S = (int(v) for v in shape.lower().split("x"))
    cells = n * S
    print(f"vcf_micro: {n} sites x {S} samples = {cells} cells, chunk_bytes {256 << 20}, "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        w = make(64, 300, seed=1)                                   # warm-up: code object, pinned allocations
        write_vcf_device(os.path.join(tmp, "warm.vcf"), "21", w[3], w[0], w[1], w[2], w[4], device=DEV)
        h1, h2, gt, pos, samples = make(n, S)
        d1, d2, dg = (torch.from_numpy(a).to(DEV) for a in (h1, h2, gt))
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        write_vcf(os.path.join(tmp, "host.vcf"), "21", pos, h1, h2, gt, samples)
        t_host = time.perf_counter() - t0
        size = os.path.getsize(os.path.join(tmp, "host.vcf"))
        print(f"host write_vcf            complete file {t_host:9.3f} s  {t_host / cells * 1e6:8.4f} us per cell  "
              f"({size} bytes, {size / cells:.2f} per cell)", flush=True)

        res = {}
        for label, arrs in (("device, host arrays", (h1, h2, gt)), ("device, device arrays", (d1, d2, dg))):
            ts = []
            for rep in range(3):
                path = os.path.join(tmp, "dev.vcf")
                t0 = time.perf_counter()
                ok = write_vcf_device(path, "21", pos, *arrs, samples, device=DEV)
                ts.append(time.perf_counter() - t0)
                assert ok
            with open(path, "rb") as fa, open(os.path.join(tmp, "host.vcf"), "rb") as fb:
                same = fa.read() == fb.read()
            res[label] = min(ts)
            print(f"{label:25s} complete file {min(ts):9.3f} s  {min(ts) / cells * 1e6:8.4f} us per cell  "
                  f"(3 runs: {' '.join(f'{t:.3f}' for t in ts)}; bytes equal the host file: {same})", flush=True)
            assert same

        ms, n_chunks, text_bytes = kernel_only(d1, d2, dg, pos, S, reps=10)
        moved = 72 * cells
        tbs = moved / (ms * 1e-3) / 1e12
        cp = copy_tbs()
        print(f"kernel alone              {n_chunks} launches {ms:9.3f} ms  {ms * 1e3 / cells:8.6f} us per cell  "
              f"72 B per cell = {tbs:.3f} TB/s = {tbs / cp:.2f} of a 400 MB device copy ({cp:.3f} TB/s)", flush=True)
        for label, t in res.items():
            print(f"ratio complete file, host writer / {label}: {t_host / t:.1f}x "
                  f"({t_host / cells * 1e6:.4f} vs {t / cells * 1e6:.4f} us per cell)")
        t = res["device, device arrays"]
        print(f"complete file from device arrays: {text_bytes / t / 1e9:.3f} GB/s of text; "
              f"the kernel is {ms * 1e-3 / t * 100:.1f} % of it (the rest: device-to-host copy, file write, host prefixes)")
        d2h, fw = copy_and_file_gbs(tmp, min(text_bytes, 256 << 20))
        print(f"alone, on {min(text_bytes, 256 << 20)} bytes: device-to-host copy into pinned memory {d2h:.2f} GB/s "
              f"= {text_bytes / d2h / 1e9:.3f} s for this file; file write from the pinned buffer (local temporary directory) "
              f"{fw:.2f} GB/s = {text_bytes / fw / 1e9:.3f} s for this file")


if __name__ == "__main__":
    main()
