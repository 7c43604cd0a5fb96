"""Device-resident featurisation: what it costs and what it saves (GPU only).

  python tools/features_micro.py kernel        batch_features launch time vs bytes written / fill bandwidth
  python tools/features_micro.py infer [W ...]  run() loop seconds, d384/L12, batch 256, 8 batches:
                                               host path with num_workers W ... (default 0 8), then device features
  python tools/features_micro.py train         training step ms at B = 24, DataLoader vs DeviceBatchLoader

Times: device events around the launches (kernel), a host clock around loops that end in a device
synchronise (infer, train).  Every timed shape is warmed first."""
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


def kernel():
    from src import kernels as K
    from src.dataset.device_features import DeviceFeatures
    from src.dataset.synthetic import make_rag_dataset
    np.random.seed(0)
    ds, _ = make_rag_dataset(n_samples=256, n_sites=1020, n_windows=2, n_ref_samples=32, name="train")
    df = DeviceFeatures(ds, DEV)
    print(f"tables: {df.nbytes} bytes on the device (256 samples x 2040 sites, 2 windows)")
    L = 1030
    for B in (256, 24):
        rows = torch.tensor(np.stack([np.arange(B) % 256, np.arange(B) % 2, np.zeros(B, np.int64)]),
                            dtype=torch.int32)                                   # both windows
        rows_dev = rows.to(DEV)
        for labels in (True, False):
            nbytes = B * L * (72 if labels else 48)
            fill = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
            t_fill = ev_ms(lambda: fill.fill_(1), 200)
            t = ev_ms(lambda: K.batch_features(df.tables, rows_dev, rows, B, L, df.token_ids, labels=labels), 200)
            print(f"B={B:3d} L={L} labels={int(labels)}: {t * 1e3:7.1f} us per launch (allocations included), "
                  f"{nbytes / 1e6:6.2f} MB written = {nbytes / t / 1e9:7.3f} TB/s; "
                  f"fill_ of the same bytes {t_fill * 1e3:6.1f} us = {nbytes / t_fill / 1e9:7.3f} TB/s; "
                  f"ratio fill / kernel {t_fill / t:.2f}")
    big = torch.empty(400 << 20, device=DEV, dtype=torch.uint8)
    t_big = ev_ms(lambda: big.fill_(1), 20)
    print(f"fill_ 400 MiB (tools/bw_micro.py's write figure): {(400 << 20) / t_big / 1e9:.3f} TB/s")


def infer(workers):
    from src.dataset.embedding_rag_infer_dataset import EmbeddingRAGInferDataset
    from src.dataset.synthetic import POPS, make_infer_arrays
    from src.dataset.vocab import WordVocab
    from src.engine import engine_for
    from src.infer_embedding_rag import run
    from src.model import build_model
    n_ref = 2048
    a = make_infer_arrays(n_sites=4080, n_samples=512, n_ref_samples=n_ref, missing_rate=0.3, seed=11)
    vocab = WordVocab(POPS)
    ds = EmbeddingRAGInferDataset.from_arrays(vocab, a["vcf"], a["pos"], a["pops"], a["freq"], a["pop_to_idx"],
                                              a["pos_to_idx"], a["ref_gt"], a["ref_pos"])
    torch.manual_seed(0)
    m = build_model(len(vocab), 384, 12, 12).to(DEV).eval()
    engine_for(m).set_dtype(torch.bfloat16)
    n_b = len(ds) // 256
    print(f"infer: d384/L12 bf16, batch 256, {n_b} batches ({len(ds)} sample-windows, 4 windows of 1020 sites), "
          f"panel {2 * n_ref} haplotypes (the 1 M-haplotype panel was not used)")
    ref = None
    for label, kw in [(f"host num_workers={w}", dict(num_workers=w)) for w in workers] + \
                     [("device_features", dict(device_features=True))]:
        secs = []
        for rep in range(3):                       # the first repetition warms (index builds, code objects)
            res = run(ds, m, DEV, 256, 1, **kw)
            secs.append(res["seconds"])
        same = "" if ref is None else f" outputs equal host: {all(np.array_equal(res[k], ref[k]) for k in ('h1', 'h2', 'gt', 'mask', 'idx1', 'idx2'))}"
        ref = ref if ref is not None else res
        print(f"  {label:24s} loop s (3 runs, first = warm-up): {' '.join(f'{s:.3f}' for s in secs)}  "
              f"-> {min(secs[1:]) / n_b * 1e3:.1f} ms per batch{same}", flush=True)


def train():
    from src.dataset.device_features import DeviceBatchLoader
    from src.dataset.embedding_rag_dataset import embedding_rag_collate_fn
    from src.dataset.sampler import WindowGroupedSampler
    from src.dataset.synthetic import make_rag_dataset
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized
    from src.model import build_model
    print("train: d384/L12, B = 24, 1020-site windows, panel 512 haplotypes, k = 1")
    for label in ("DataLoader num_workers=0", "DeviceBatchLoader"):
        np.random.seed(0)
        torch.manual_seed(0)
        ds, vocab = make_rag_dataset(n_samples=96, n_sites=1020, n_windows=2, n_ref_samples=256, seed=5, name="train")
        sampler = WindowGroupedSampler(ds, shuffle=True, seed=42)
        if label == "DeviceBatchLoader":
            loader = DeviceBatchLoader(ds, sampler, 24, DEV)
        else:
            loader = torch.utils.data.DataLoader(ds, batch_size=24, sampler=sampler,
                                                 collate_fn=embedding_rag_collate_fn)
        m = build_model(len(vocab), 384, 12, 12).to(DEV)
        tr = BERTTrainerWithValidationOptimized(m, loader, None, vocab, lr=1e-4, warmup_steps=10, grad_accum_steps=1,
                                                log_freq=0)
        tr.rag_k = 1
        out = []
        for ep in range(4):                        # 8 steps per pass; the first pass warms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for batch in loader:
                tr.train_step(batch)
                n += 1
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / n * 1e3)
        print(f"  {label:26s} ms per step over 4 passes of {n} steps (first = warm-up): "
              f"{' '.join(f'{t:.2f}' for t in out)}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what == "kernel":
        kernel()
    elif what == "infer":
        infer([int(w) for w in sys.argv[2:]] or [0, 8])
    elif what == "train":
        train()
    else:
        raise SystemExit(__doc__)
