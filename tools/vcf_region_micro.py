"""A region read through the tabix index against the whole-file read, in both inflate modes (GPU only).

  python tools/vcf_region_micro.py [SITESxSAMPLES [PERCENT]]      default 6000x10000 1

Writes a bgzipped VCF and its ``.tbi`` with ``write_vcf_device(bgzf=True, index=True)`` (mostly confident calls,
as tools/vcf_deflate_micro.py makes them) into a local temporary directory, then times ``read_vcf`` of the whole
file and of a region of PERCENT of its records from the middle, with ``inflate="host"`` and ``inflate="device"``.

Times: a host clock around each call (it ends synchronised), one warm call per arm, then 3 rounds with the arms
alternating; the best and all three are listed, beside the members each call inflated (``READ_STATS``).  The file
is in the page cache for every arm.  Not measured: a cold file system, a foreign index."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def main():
    from vcf_deflate_micro import make
    from src.dataset import vcf_reader as V
    from src.infer_embedding_rag import write_vcf_device
    n, S = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "6000x10000").lower().split("x"))
    percent = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    print(f"vcf_region_micro: {n} sites x {S} samples, region of {percent} % of the records, "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "big.vcf.gz")
        h1, h2, gt, pos, samples = make(n, S, 0.9)
        t0 = time.perf_counter()
        assert write_vcf_device(path, "21", pos, *(torch.from_numpy(a).to(DEV) for a in (h1, h2, gt)), samples,
                                device=DEV, bgzf=True, index=True)
        del h1, h2, gt
        torch.cuda.empty_cache()
        print(f"written in {time.perf_counter() - t0:.2f} s: {os.path.getsize(path) / 1e6:.1f} MB .vcf.gz, "
              f"{os.path.getsize(path + '.tbi')} bytes .tbi", flush=True)
        k = max(1, round(n * percent / 100))
        lo = (n - k) // 2
        region = ("21", int(pos[lo]), int(pos[lo + k - 1]))
        arms = [(f"{what:6s} inflate={mode}", mode, reg) for what, reg in (("whole", None), ("region", region))
                for mode in ("host", "device")]
        ts, info = {a[0]: [] for a in arms}, {}
        for rnd in range(4):
            for label, mode, reg in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                vg = V.read_vcf(path, DEV, inflate=mode, region=reg)
                dt = time.perf_counter() - t0
                if rnd:                                              # round 0 warms
                    ts[label].append(dt)
                info[label] = (vg.n_sites, V.READ_STATS["members_inflated"])
                assert vg.n_sites == (k if reg else n)
                del vg
        for label, _, _ in arms:
            print(f"read_vcf {label:24s} {min(ts[label]):8.4f} s  ({' '.join(f'{t:.4f}' for t in ts[label])})  "
                  f"{info[label][0]} records, " +
                  (f"{info[label][1]} members inflated" if info[label][1] else "one gzip stream (members not counted)"),
                  flush=True)


if __name__ == "__main__":
    main()
