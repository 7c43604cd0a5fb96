"""Per-site statistics kernel (csrc/quality.hip) at the VCF writer's shape: what it costs (GPU only).

  python tools/site_stats_micro.py [n_sites n_samples]        default 2000 10000

Kernel: device events around 50 launches (warmed), with and without truth; the rate is the bytes the kernel
must read — 24 per site and sample (h1, h2, gt), 2 more with truth (the truth pair; the 4-byte truth_col is
shared by every site and stays in cache) — over that time, beside a 400 MB device copy and read taken in the
same process (the method of tools/bw_micro.py).  Host arm: ``site_stats_host`` (numpy) on the same arrays by a
host clock, and the chunked upload path of ``site_stats`` from host arrays (copies included)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")


def ev_ms(fn, reps):
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
    from src import quality as Q
    n, S = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (2000, 10000)
    rng = np.random.default_rng(0)
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    truth = rng.integers(0, 2, (n, S, 2)).astype(np.int8)
    truth[rng.random((n, S)) < 0.02] = -1
    row, col = rng.permutation(n).astype(np.int32), rng.permutation(S).astype(np.int32)
    d = lambda a: torch.from_numpy(a).to(DEV)
    dh1, dh2, dgt, dtruth, drow, dcol = d(h1), d(h2), d(gt), d(truth), d(row), d(col)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    print(f"{torch.cuda.get_device_name(0)}; {n} sites x {S} samples: {24 * n * S / 1e6:.0f} MB of results, "
          f"{2 * n * S / 1e6:.0f} MB of truth")

    mb = 400
    x = torch.randn(mb * (1 << 20) // 4, device=DEV)
    y = torch.empty_like(x)
    t_copy, t_sum = ev_ms(lambda: y.copy_(x), 50), ev_ms(lambda: x.sum(), 50)
    print(f"{mb} MiB device copy  {t_copy:.3f} ms  {2 * mb * 1.048576 / t_copy:.0f} GB/s (read + write);  "
          f"sum {t_sum:.3f} ms  {mb * 1.048576 / t_sum:.0f} GB/s (read)")
    del x, y

    t_est = ev_ms(lambda: K.site_stats(dh1, dh2, dgt), 50)
    t_acc = ev_ms(lambda: K.site_stats(dh1, dh2, dgt, dtruth, drow, dcol, bad), 50)
    print(f"site_stats, est only    {t_est:.3f} ms  {24 * n * S / t_est / 1e6:.0f} GB/s  (24 B per cell)")
    print(f"site_stats, with truth  {t_acc:.3f} ms  {26 * n * S / t_acc / 1e6:.0f} GB/s  (26 B per cell)")
    assert int(bad.item()) == 0

    t0 = time.perf_counter()
    got = Q.site_stats(h1, h2, gt, truth, row, col, device=DEV)
    t_up = time.perf_counter() - t0
    print(f"site_stats from host arrays (chunked upload, pageable memory)  {t_up * 1e3:.0f} ms")
    t0 = time.perf_counter()
    want = Q.site_stats_host(h1, h2, gt, truth, row, col)
    t_host = time.perf_counter() - t0
    print(f"site_stats_host (numpy, {os.environ.get('OMP_NUM_THREADS', '?')} threads allowed)  {t_host * 1e3:.0f} ms  "
          f"= {t_host * 1e3 / t_acc:.0f} x the kernel with truth")
    rel = max(float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))) for g, w in zip(got[:2], want[:2]))
    print(f"kernel vs numpy: tables equal {np.array_equal(got[2], want[2])}, largest relative difference of a sum "
          f"{rel:.2e}")


if __name__ == "__main__":
    main()
