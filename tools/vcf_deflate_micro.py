"""The bgzipped VCF writers on the same arrays in one process (GPU only).

  python tools/vcf_deflate_micro.py [SITESxSAMPLES]      default 2000x10000

Two sets of values: tools/vcf_micro.py's random probabilities (the worst case for compression) and mostly
confident calls (0.9 of the cells hold 0 / 1 probabilities).  Per set, for the complete file written to a local
temporary directory: the host ``write_vcf(bgzf=True)`` (zlib level 6 through BgzfWriter), ``write_vcf_device``
plain, ``write_vcf_device(bgzf=True)`` and ``write_vcf_device(bgzf=True, index=True)`` (the last two alternate,
so that the cost of the tabix index shows against the same process's spread), all from device arrays; the file
sizes and the ``.tbi``'s; the deflate and the pack
kernels alone (device events around the launches of one chunk's members, no copy); and the device file's size
over zlib level 1 and level 6 at the same member size, on the first 64 members of the text.

Times: a host clock around each complete write (it ends with the file closed), best of 3 with all three listed;
device events around the kernel launches, 5 passes after one warm pass.  Not measured: a file system other than
the local temporary directory, host arrays (the upload path), more than one GPU."""
import gzip
import os
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")


def make(n, S, confident, seed=0):
    rng = np.random.default_rng(seed)
    gt = rng.random((n, S, 4), dtype=np.float32)
    gt /= gt.sum(-1, keepdims=True)
    if confident > 0:
        sure = rng.random((n, S)) < confident
        cls = rng.choice(4, (n, S), p=[0.8, 0.08, 0.08, 0.04])
        gt[sure] = np.eye(4, dtype=np.float32)[cls[sure]]
        h1, h2 = gt[..., 2] + gt[..., 3], gt[..., 1] + gt[..., 3]
    else:
        h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    pos = np.cumsum(rng.integers(1, 2000, n)).astype(np.int64) + 10_000_000
    return h1, h2, gt, pos, [f"S{i}" for i in range(S)]


def events_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels_alone(text_bytes: bytes):
    """(deflate ms, pack ms, members, packed bytes) over at most 256 MiB of the file's text."""
    from src import kernels as K
    nbytes = min(len(text_bytes), 256 << 20)
    text = torch.frombuffer(bytearray(text_bytes[:nbytes]), dtype=torch.uint8).to(DEV)
    nb = -(-nbytes // 0xff00)
    members = torch.empty(nb, K.BGZF_SLOT, device=DEV, dtype=torch.uint8)
    mlen = torch.empty(nb, device=DEV, dtype=torch.int32)
    out = torch.empty(nb * (0xff00 + 31), device=DEV, dtype=torch.uint8)
    total = torch.empty(1, device=DEV, dtype=torch.int64)
    t_def = events_ms(lambda: K.bgzf_deflate(text, nbytes, 0xff00, members, mlen))
    t_pack = events_ms(lambda: K.bgzf_pack(members, mlen, out, total))
    return t_def, t_pack, nb, int(total.item()), nbytes


def main():
    from src.dataset import bgzf as B
    from src.infer_embedding_rag import write_vcf, write_vcf_device
    shape = sys.argv[1] if len(sys.argv) > 1 else "2000x10000"
    n, S = (int(v) for v in shape.lower().split("x"))
    print(f"vcf_deflate_micro: {n} sites x {S} samples, member 0xff00, device {torch.cuda.get_device_name(0)}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        w = make(64, 300, 0.5, seed=1)                              # warm-up: code objects, pinned allocations
        for bg in (False, True):
            write_vcf_device(os.path.join(tmp, "warm"), "21", w[3], w[0], w[1], w[2], w[4], device=DEV, bgzf=bg)
        for confident in (0.0, 0.9):
            h1, h2, gt, pos, samples = make(n, S, confident)
            d1, d2, dg = (torch.from_numpy(a).to(DEV) for a in (h1, h2, gt))
            torch.cuda.synchronize()
            print(f"--- confident cells {confident}", flush=True)
            t0 = time.perf_counter()
            write_vcf(os.path.join(tmp, "host.vcf.gz"), "21", pos, h1, h2, gt, samples, bgzf=True)
            t_host = time.perf_counter() - t0
            print(f"host write_vcf(bgzf=True)        complete file {t_host:9.3f} s  "
                  f"{os.path.getsize(os.path.join(tmp, 'host.vcf.gz'))} bytes (zlib level 6)", flush=True)
            arms = (("device writer, plain", "dev.vcf", False, False), ("device writer, bgzf=True", "dev.vcf.gz", True, False),
                    ("device writer, bgzf + index", "dev.vcf.gz", True, True))
            ts = {arm[0]: [] for arm in arms}
            for _ in range(3):                                          # the arms alternate
                for label, name, bg, ix in arms:
                    t0 = time.perf_counter()
                    assert write_vcf_device(os.path.join(tmp, name), "21", pos, d1, d2, dg, samples, device=DEV, bgzf=bg,
                                            index=ix)
                    ts[label].append(time.perf_counter() - t0)
            for label, name, bg, ix in arms:
                print(f"{label:32s} complete file {min(ts[label]):9.3f} s  {os.path.getsize(os.path.join(tmp, name))} bytes  "
                      f"(3 runs: {' '.join(f'{t:.3f}' for t in ts[label])})", flush=True)
            print(f"{'':32s} dev.vcf.gz.tbi {os.path.getsize(os.path.join(tmp, 'dev.vcf.gz.tbi'))} bytes for {n} records",
                  flush=True)
            with open(os.path.join(tmp, "dev.vcf"), "rb") as f:
                plain = f.read()
            with open(os.path.join(tmp, "dev.vcf.gz"), "rb") as f:
                assert gzip.decompress(f.read()) == plain
            with open(os.path.join(tmp, "host.vcf.gz"), "rb") as f:
                assert gzip.decompress(f.read()) == plain
            body = plain[plain.index(b"\n21\t") + 1:]
            t_def, t_pack, nb, packed, nbytes = kernels_alone(body)
            print(f"kernels alone, {nbytes} bytes of text in {nb} members: deflate {t_def:9.3f} ms = "
                  f"{nbytes / t_def / 1e6:.2f} GB/s of text; pack {t_pack:7.3f} ms; {packed} bytes, ratio {nbytes / packed:.2f}",
                  flush=True)
            part = body[:64 * 0xff00]
            dev = len(B.deflate_device(part, device=DEV))
            z = {lv: sum(len(B.bgzf_member(part[o:o + 0xff00], lv)) for o in range(0, len(part), 0xff00)) for lv in (1, 6)}
            print(f"first {len(part)} bytes of text: device {dev}, zlib level 1 {z[1]} (device / zlib = {dev / z[1]:.3f}), "
                  f"zlib level 6 {z[6]} (device / zlib = {dev / z[6]:.3f})", flush=True)
            for name in ("host.vcf.gz", "dev.vcf", "dev.vcf.gz", "dev.vcf.gz.tbi"):
                os.remove(os.path.join(tmp, name))
            del d1, d2, dg


if __name__ == "__main__":
    main()
