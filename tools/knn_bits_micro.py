"""u8 vs bit-packed panel scan at the bench shape (1 M haplotypes x 1024 sites, k = 32).

For 48 / 96 / 128 / 512 queries the two forms are timed alternately in one process, round after
round: the bare full-panel scan launch (``knn_scan`` / ``knn_scan_bits``) and the product search
(``PanelIndex.scan_keys``: threshold pre-pass, scan, merges).  Every launch reads another copy of
the panel than the one before it (hash-generated panels of consecutive seeds), with enough copies
that their footprint exceeds the 256 MB Infinity Cache, so each launch streams from HBM.  The bit
panels come from ``panel_synth_bits``; the u8 panels exist only for the u8 arm.

Per form and query count: median (min .. max over the rounds) time per launch, the launch's
algorithmic bytes (panel once + LUT + partial keys), their rate as a fraction of the 8 TB/s HBM
peak, and int8 TOPS (2 N n_sites_pad nq per limb the scan ran; the aligned-mask LUT of this
workload reduces to one limb, read back from the LUT's flag).  Also checks, once per query count,
that the two forms return identical keys on the same panel, and prints how many windows of each
form a 64 GiB dataset cache and the 288 GB HBM hold, computed from ``PanelIndex.nbytes``.

usage: python tools/knn_bits_micro.py [--n_ref N] [--queries 48,96,128,512] [--rounds R] [--reps M]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "rag-snvbert_amd"))
from src import kernels as K  # noqa: E402
from src.retrieval import PanelIndex  # noqa: E402

HBM_PEAK = 8.0e12           # B/s, HBM3E spec (bench.py's HBM_PEAK_GBS)
MALL = 256 << 20


def timed(fns, reps):
    """ms per call of the rotation ``fns`` (call i runs fns[i % len(fns)]), device events."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fns[i % len(fns)]()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_ref", type=int, default=1 << 20)
    ap.add_argument("--sites", type=int, default=1024)
    ap.add_argument("--queries", default="48,96,128,512")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=120)
    args = ap.parse_args()
    dev, S, L, k = "cuda", args.sites, args.sites + 6, args.k
    rng = np.random.default_rng(0)
    af = torch.from_numpy(rng.beta(0.3, 3.0, S).astype(np.float32)).to(dev)
    ref_af = torch.zeros(L, device=dev)
    one = PanelIndex.synthetic(args.n_ref, S, af, ref_af, 7, packed=True)
    n_bits = max(2, -(-2 * MALL // one.nbytes))              # copies: footprint >= 2 x Infinity Cache
    n_u8 = max(2, -(-2 * MALL // (8 * one.nbytes)))
    bits = [one] + [PanelIndex.synthetic(args.n_ref, S, af, ref_af, 7 + i, packed=True) for i in range(1, n_bits)]
    u8 = [PanelIndex.synthetic(args.n_ref, S, af, ref_af, 7 + i) for i in range(n_u8)]
    pad = one.n_sites_pad
    print(f"panel {args.n_ref} x {S} (pad {pad}), k={k}; u8 {u8[0].nbytes / 1e6:.1f} MB x {n_u8} copies, "
          f"bits {one.nbytes / 1e6:.1f} MB x {n_bits} copies; rounds={args.rounds} reps={args.reps}")
    for name, nb in (("u8", u8[0].nbytes), ("bits", one.nbytes)):
        print(f"resident windows (computed from nbytes): {name}: {(64 << 30) // nb} in a 64 GiB dataset cache, "
              f"{int(288e9) // nb} in 288 GB of HBM")
    W = torch.randn(12, 384, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    mask = (rng.random(S) < 0.6).astype(np.uint8)
    smask = torch.from_numpy(mask).to(dev)
    rows = []
    for nq in (int(x) for x in args.queries.split(",")):
        alle = (rng.random((nq, S)) < af.cpu().numpy()[None]).astype(np.int64)
        tok = np.zeros((nq, L), np.int64)
        tok[:, 0], tok[:, S + 1] = 2, 3
        tok[:, 1:S + 1] = np.where(mask[None] == 1, 4, 5 + alle)
        lut, _, _ = one.lut(torch.from_numpy(tok).to(dev), W, smask, 2)
        nqt, KS = (nq + 15) // 16, pad // 64
        wide = int(lut[nqt * 3 * KS * 1024 + nqt * 64:][:4].cpu().numpy().view(np.int32)[0])
        limbs_run = 2 if wide else 1
        same = torch.equal(bits[0].scan_keys(lut, nq, 2, k), u8[0].scan_keys(lut, nq, 2, k))
        forms = {
            "u8": dict(scan=[(lambda i=i: K.knn_scan(i.codes, pad, lut, nq, 2, k)) for i in u8],
                       search=[(lambda i=i: i.scan_keys(lut, nq, 2, k)) for i in u8], row=pad),
            "bits": dict(scan=[(lambda i=i: K.knn_scan_bits(i.bits, pad, lut, nq, 2, k)) for i in bits],
                         search=[(lambda i=i: i.scan_keys(lut, nq, 2, k)) for i in bits], row=pad // 8),
        }
        parts = forms["u8"]["scan"][0]().shape[0]
        t = {f: dict(scan=[], search=[]) for f in forms}
        for _ in range(args.rounds):                      # alternate the forms inside every round
            for f, d in forms.items():
                for what in ("scan", "search"):
                    t[f][what].append(timed(d[what], args.reps))
        for f, d in forms.items():
            byts = args.n_ref * d["row"] + nq * pad * 2 + parts * nq * k * 8
            ms = statistics.median(t[f]["scan"])
            ops = 2.0 * args.n_ref * pad * nq * limbs_run
            rows.append(dict(form=f, queries=nq, limbs_run=limbs_run, keys_equal_u8=bool(same), n_parts=parts,
                             scan_ms=round(ms, 4), scan_ms_min=round(min(t[f]["scan"]), 4),
                             scan_ms_max=round(max(t[f]["scan"]), 4), alg_bytes=int(byts),
                             frac_hbm_peak=round(byts / (ms * 1e-3) / HBM_PEAK, 4),
                             int8_tops=round(ops / (ms * 1e-3) / 1e12, 1),
                             search_ms=round(statistics.median(t[f]["search"]), 4),
                             search_ms_min=round(min(t[f]["search"]), 4),
                             search_ms_max=round(max(t[f]["search"]), 4)))
    print(f"{'form':>5} {'nq':>4} {'limbs':>5} {'scan ms (min..max)':>26} {'alg MB':>8} {'HBM frac':>8} "
          f"{'i8 TOPS':>8} {'search ms (min..max)':>28} keys==u8")
    for r in rows:
        print(f"{r['form']:>5} {r['queries']:>4} {r['limbs_run']:>5} "
              f"{r['scan_ms']:>9.4f} ({r['scan_ms_min']:.4f}..{r['scan_ms_max']:.4f}) {r['alg_bytes'] / 1e6:>8.1f} "
              f"{r['frac_hbm_peak']:>8.3f} {r['int8_tops']:>8.1f} "
              f"{r['search_ms']:>11.4f} ({r['search_ms_min']:.4f}..{r['search_ms_max']:.4f}) {r['keys_equal_u8']}")
    print(json.dumps(dict(tool="knn_bits_micro", device=torch.cuda.get_device_name(0), n_ref=args.n_ref, sites=S,
                          k=k, rounds=args.rounds, reps=args.reps, rows=rows)))
    if not all(r["keys_equal_u8"] for r in rows):
        raise SystemExit("bit scan keys differ from the u8 scan's")


if __name__ == "__main__":
    main()
