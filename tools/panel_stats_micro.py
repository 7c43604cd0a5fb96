"""Panel counting kernel (csrc/panel_stats.hip) at a 1000-Genomes-sized panel: what it costs (GPU only).

  python tools/panel_stats_micro.py [n_samples n_sites]        default 2504 1000000 (5 008 haplotypes x 1M sites)

The bit rows are generated on the device (ALT bits uniform, 1.6 % of the alleles missing), five populations
interleaved in sample order.  Three timings in one process:

  kernel   device events around 100 launches (10 warm-up launches first); the rate is the bytes of the two bit
           matrices (2 x 2 S x ceil(n_sites / 8), each read once) over that time, and its fraction of
  read     the read bandwidth measured here by the method of tools/bw_micro.py (a bf16 sum over 400 and
           1600 MiB, device events around 20 launches);
  host     ``panel_counts_host`` (numpy, the specification) on the first HOST_SITES sites, cut into 16 chunks on
           16 threads, by a host clock; it is linear in the sites and is scaled to n_sites.  The same slice is
           compared with the kernel's counts bit for bit."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")
HOST_SITES, THREADS = 131072, 16


def ev_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    from src import kernels as K
    from src.dataset import panel_stats as PS
    S, n = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (2504, 1000000)
    P, nb = 5, (n + 7) // 8
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda: torch.randint(0, 256, (2 * S, nb), device=DEV, dtype=torch.uint8, generator=g)
    miss = rnd() & rnd() & rnd() & rnd() & rnd() & rnd()                 # 1 / 64 of the alleles
    alt = rnd() & ~miss
    key = np.arange(S) % P
    order = np.argsort(key, kind="stable").astype(np.int32)
    pop_start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=P))]).astype(np.int32)
    d_order, d_start = torch.from_numpy(order).to(DEV), torch.from_numpy(pop_start).to(DEV)
    out = torch.empty(6, 5, n, device=DEV, dtype=torch.int32)
    nbytes = 2 * 2 * S * nb
    print(f"{torch.cuda.get_device_name(0)}; {2 * S} haplotypes x {n} sites, {P} populations: "
          f"{nbytes / 1e6:.0f} MB of bit rows, {out.numel() * 4 / 1e6:.0f} MB of counts")

    read = {}
    for mb in (400, 1600):
        x = torch.randn(mb * (1 << 20) // 2, device=DEV).to(torch.bfloat16)
        t = ev_ms(lambda: x.sum(), 20)
        read[mb] = mb * 1.048576 / t
        print(f"read bandwidth, bf16 sum over {mb} MiB  {t:.3f} ms  {read[mb]:.0f} GB/s")
        del x
    bw = max(read.values())

    t = ev_ms(lambda: K.panel_counts(alt, miss, n, d_order, d_start, out=out), 100, warm=10)
    rate = nbytes / t / 1e6
    print(f"panel_counts  {t:.3f} ms  {rate:.0f} GB/s over the bit rows  = {rate / bw:.2f} of the measured read "
          f"bandwidth ({bw:.0f} GB/s)")

    h = min(HOST_SITES, n) // 8 * 8
    gt = K.vcf_unpack_gt(alt[:, :h // 8].contiguous(), miss[:, :h // 8].contiguous(), h).cpu().numpy()
    cuts = np.linspace(0, h, THREADS + 1).astype(int)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(lambda i: PS.panel_counts_host(gt[cuts[i]:cuts[i + 1]], order, pop_start, P),
                              range(THREADS)))
    t_host = time.perf_counter() - t0
    want = np.concatenate(parts, axis=2)
    same = np.array_equal(out[:, :, :h].cpu().numpy(), want)
    print(f"panel_counts_host (numpy, {THREADS} threads) on {h} sites  {t_host * 1e3:.0f} ms  -> "
          f"{t_host * n / h * 1e3:.0f} ms scaled to {n} sites  = {t_host * n / h * 1e3 / t:.0f} x the kernel; "
          f"counts equal on the slice: {same}")
    assert same


if __name__ == "__main__":
    main()
