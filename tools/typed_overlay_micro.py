"""Typed-site overlay kernel (csrc/typed.hip) at a whole-chromosome size: what it costs (GPU only).

  python tools/typed_overlay_micro.py [n_sites n_samples]        default 200000 2048 (half the sites typed)

The target's bit rows are generated on the device (ALT bits uniform, 1.6 % of the alleles missing); every second
site row is typed, in increasing record order; the columns map one to one.  Three things are timed in one process,
by device events around REPS launches each, in ROUNDS alternating rounds after a warm-up round (the median round is
reported, with the fastest and slowest):

  kernel   ``kernels.typed_overlay`` on h1 / h2 [n, S] and gt [n, S, 4] in place; the bytes are the 24 bytes stored
           per typed cell with both alleles called (the bit rows read are 4 bits per typed cell);
  fill     the store floor: ``fill_`` of the same number of bytes, as three contiguous blocks in the proportions
           1 : 1 : 4 (what h1, h2 and gt receive);
  torch    the plain formulation: ``kernels.vcf_unpack_gt`` of the whole target, ``index_select`` of the typed
           records, ``where`` against the typed rows of the three arrays, ``index_copy_`` back.

The kernel's result is compared with the torch formulation's bit for bit, and the missing count with the bit rows."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rag-snvbert_amd"))
DEV = torch.device("cuda")
REPS, ROUNDS = 5, 5


def ev_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    from src import kernels as K
    n, S = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (200000, 2048)
    n_target = n // 2
    nb = (n_target + 7) // 8
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda: torch.randint(0, 256, (2 * S, nb), device=DEV, dtype=torch.uint8, generator=g)
    miss = rnd() & rnd() & rnd() & rnd() & rnd() & rnd()                 # 1 / 64 of the alleles
    alt = rnd() & ~miss
    site_row = np.full(n, -1, np.int32)
    site_row[1::2] = np.arange(n // 2, dtype=np.int32)[:len(site_row[1::2])]
    typed = torch.from_numpy(np.flatnonzero(site_row >= 0)).to(DEV)
    records = torch.from_numpy(site_row[site_row >= 0].astype(np.int64)).to(DEV)
    d_row, d_col = torch.from_numpy(site_row).to(DEV), torch.arange(S, device=DEV, dtype=torch.int32)
    h1, h2 = torch.rand(n, S, device=DEV), torch.rand(n, S, device=DEV)
    gt = torch.rand(n, S, 4, device=DEV)
    missing = torch.empty(n, device=DEV, dtype=torch.int32)

    def torch_overlay(h1, h2, gt):
        sel = K.vcf_unpack_gt(alt, miss, n_target).index_select(0, records)          # i8 [typed, S, 2]
        ok = (sel >= 0).all(-1)
        a1, a2 = sel[..., 0] > 0, sel[..., 1] > 0
        h1.index_copy_(0, typed, torch.where(ok, a1.float(), h1.index_select(0, typed)))
        h2.index_copy_(0, typed, torch.where(ok, a2.float(), h2.index_select(0, typed)))
        hot = torch.nn.functional.one_hot(2 * a1.long() + a2.long(), 4).float()
        gt.index_copy_(0, typed, torch.where(ok[..., None], hot, gt.index_select(0, typed)))
        return (~ok).sum(1)

    # the same answer first, on copies
    c1, c2, cg = h1.clone(), h2.clone(), gt.clone()
    miss_rows = torch_overlay(c1, c2, cg)
    K.typed_overlay(h1, h2, gt, alt, miss, n_target, d_row, d_col, missing=missing)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((h1, c1), (h2, c2), (gt, cg)))
    same = same and torch.equal(missing.index_select(0, typed), miss_rows.int()) and int(missing.sum()) == int(miss_rows.sum())
    cells = int(typed.numel()) * S - int(missing.sum())
    nbytes = 24 * cells
    del c1, c2, cg, miss_rows
    print(f"{torch.cuda.get_device_name(0)}; {n} sites ({typed.numel()} typed) x {S} samples: {cells} cells overlaid, "
          f"{nbytes / 1e9:.3f} GB stored, {int(missing.sum())} cells left (a call missing); kernel == torch: {same}")
    assert same

    parts = [torch.empty(cells * k, device=DEV) for k in (1, 1, 4)]
    runs = dict(kernel=lambda: K.typed_overlay(h1, h2, gt, alt, miss, n_target, d_row, d_col, missing=missing),
                fill=lambda: [p.fill_(1.0) for p in parts],
                torch=lambda: torch_overlay(h1, h2, gt))
    times = {k: [] for k in runs}
    for r in range(ROUNDS + 1):
        for k, fn in runs.items():
            t = ev_ms(fn, REPS)
            if r:                                                        # round 0 warms every shape up
                times[k].append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:7s} {med[k]:9.3f} ms  (fastest {min(v):.3f}, slowest {max(v):.3f} of {ROUNDS} rounds x {REPS} launches)  "
              f"{nbytes / med[k] / 1e6:8.0f} GB/s over the {nbytes / 1e9:.3f} GB stored")
    print(f"kernel / fill = {med['kernel'] / med['fill']:.2f}   torch / kernel = {med['torch'] / med['kernel']:.2f}")


if __name__ == "__main__":
    main()
