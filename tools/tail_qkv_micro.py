"""Block tail + next layer's QKV in one launch (snvrag_tail_qkv_forward, csrc/tailw.hip) against the
two launches it replaces, at the bench shape (M = 512 x 1030, override GM_M): launch times after a
cache flush (as in the encoder, where attention streams GBs between two tails), alternating, and the
per-wave phase breakdown of the fused launch from the stamped instantiation (tail_wide = 2), the
projection phase included (stamp slot 7; slot 6 holds the cycles parked in the FFN's barriers)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "rag-snvbert_amd"))
from src import kernels as K  # noqa: E402
from src import native as N  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from tailw_micro_case import case  # noqa: E402

D = 384
dev, bf = "cuda", torch.bfloat16
M = int(os.environ.get("GM_M", 512 * 1030))
c = case(M, 1)
ts = K.tail_pack(c["w_o"], c["w1"], c["w2g"])
g = torch.Generator(device="cpu").manual_seed(2)
w_qkv = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(dev, bf)
b_qkv = torch.randn(3 * D, generator=g).to(dev)
pw, sg, sgv = K.proj_pack(w_qkv), K.sgemm_pack(w_qkv), K.sgemm_vec(b_qkv)
xs = c["x"].clone()
qkv = torch.empty(M, 3 * D, device=dev, dtype=bf)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
K.set_option("tail_wide", 1)


def tail():
    K.tail_forward(c["att"], xs, ts, c["b_o"], c["g1"], c["be1"], c["vec"])


def fused():
    K.tail_qkv_forward(c["att"], xs, ts, c["b_o"], c["g1"], c["be1"], c["vec"], pw, b_qkv, qkv_out=qkv)


def tail_sgemm():
    tail()
    K.sgemm(xs, sg, 3 * D, sgv, out=qkv)


def tail_projw():
    tail()
    K.proj_forward(xs, pw, b_qkv, 3, out=qkv)


def cold(fn, reps=6):
    tot = []
    for _ in range(reps):
        flush.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        tot.append(a.elapsed_time(b))
    return tot


arms = {"tail + stream GEMM (2 launches)": tail_sgemm, "tail + wide-row projection (2 launches)": tail_projw,
        "tail alone": tail, "fused tail + QKV (1 launch)": fused}
for fn in arms.values():
    for _ in range(3):
        fn()
res = {k: [] for k in arms}
for it in range(3):
    for k, fn in arms.items():
        res[k] += cold(fn, 4)
for k, v in res.items():
    print(f"{k:42s} median {np.median(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  (n = {len(v)})", flush=True)

# phase stamps of the fused launch (tail_wide = 2)
nwg = (M + 31) // 32                                   # >= the workgroups of a split launch
st = torch.zeros(nwg * 4 * 8, dtype=torch.int64, device=dev)
N.lib().snvrag_tail_stamps(st.data_ptr())
K.set_option("tail_wide", 2)
flush.fill_(1)
fused()
torch.cuda.synchronize()
K.set_option("tail_wide", 1)
N.lib().snvrag_tail_stamps(None)
n_full = (M + 127) // 128
n_full = n_full - n_full % 256 if (n_full > 256 and 0 < n_full % 256 <= 64) else n_full
s = st.view(nwg * 4, 8)[:n_full * 4].cpu().numpy().astype(np.float64)    # the 128-row workgroups
names = ["prologue (att DMA, residual, tables)", "out-projection (288 MFMA)", "LN1 (2 barriers)",
         "FFN 6 rounds (2304 MFMA)", "LN_f + LN2 + stores (+ X images)"]
tot = s[:, 7] - s[:, 0]
for i, nm in enumerate(names):
    dd = s[:, i + 1] - s[:, i]
    print(f"  {nm:40s} median {np.median(dd):9.0f} cyc  p10 {np.percentile(dd, 10):9.0f}  p90 "
          f"{np.percentile(dd, 90):9.0f}  ({np.median(dd) / np.median(tot):.3f})", flush=True)
dd = s[:, 7] - s[:, 5]
print(f"  {'QKV projection (864 MFMA, 3 epilogues)':40s} median {np.median(dd):9.0f} cyc  p10 "
      f"{np.percentile(dd, 10):9.0f}  p90 {np.percentile(dd, 90):9.0f}  ({np.median(dd) / np.median(tot):.3f})", flush=True)
print(f"  {'of the FFN: parked in its barriers':40s} median {np.median(s[:, 6]):9.0f} cyc", flush=True)
print(f"  {'wave total':40s} median {np.median(tot):9.0f} cyc  (MFMA floor (2592 + 864) x 32 = {3456 * 32})", flush=True)
