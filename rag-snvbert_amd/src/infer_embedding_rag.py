"""v18 embedding-RAG imputation entry point (reference: src/infer_embedding_rag.py:53-257).

Data: ``EmbeddingRAGInferDataset`` (InferDataset items over the panel's full site list;
the sites absent from the target are masked and imputed).  Per batch (window-major order,
WindowMajorSampler): retrieval on the HBM token index (exact int8-MFMA kNN, no FAISS, no
host round trip), the native eval forward, then the reference's post-processing on the
device (snvrag_infer_post: second softmax of the head probabilities, genotype products).
Results stay on the GPU until the end of the run; one device->host copy feeds the
geometry step ([W, S, L] -> [W*L, S], slice [1, 1+window), fit to the panel's site count —
infer_embedding_rag.py:166-203) and the writers.

Outputs (``--output_path``): ``imputed.npz`` (hap1/hap2 ALT probabilities, GP, mask,
positions) and ``imputed.vcf`` (the imputed sites = mask of the first sample, as
infer_embedding_rag.py:237; GT phased argmax, HDS, GP = (p00, p01 + p10, p11), DS,
``%.3f``).  The reference's VCF call fails with a TypeError, so the
writer here defines the output instead of mirroring it.  ``--vcf_writer device`` writes the same
file, byte for byte, with the records formatted on the GPU (vcf_device.py, csrc/vcf.hip).

Windows: query windows are INFER_WINDOW_LEN = 1020 sites; ``--index_window_len`` 510
(default) reproduces the reference's 510-site index windows and infer masks
(embedding_rag_infer_dataset.py:16), 1020 aligns them with the query windows.

``--vcf_sites all`` writes one record per panel site: the typed sites carry the target's observed genotypes,
overlaid on the result arrays on the GPU before anything is written (typed_sites.py, csrc/typed.hip).
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

INFER_WINDOW_LEN = 1020
MAX_SEQ_LEN = 1030


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="v18 embedding-RAG imputation (MI355X)")
    for name in ("ref_panel", "infer_dataset", "infer_panel", "freq_path", "type_path", "pop_path", "pos_path"):
        p.add_argument(f"--{name}", type=str, default=None)
    p.add_argument("-c", "--check_point", type=str, default=None,
                   help="the reference's pickled model or a state_dict (read without executing pickled code)")
    p.add_argument("-o", "--output_path", type=str, default="output/infer")
    p.add_argument("--chrom", type=str, default="21")
    p.add_argument("-d", "--dims", type=int, default=384)
    p.add_argument("-l", "--layers", type=int, default=12)
    p.add_argument("-a", "--attn_heads", type=int, default=12)
    p.add_argument("-b", "--infer_batch_size", type=int, default=32)
    p.add_argument("-n", "--num_workers", type=int, default=0)
    p.add_argument("--k_retrieve", type=int, default=1)
    p.add_argument("--cuda_devices", type=int, nargs="+", default=None)
    p.add_argument("--window_len", type=int, default=INFER_WINDOW_LEN)
    p.add_argument("--index_window_len", type=int, default=510,
                   help="510: the reference's index windows (compat); 1020: aligned with the query windows")
    p.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    p.add_argument("--synthetic", type=int, default=0, help="samples of in-memory synthetic data")
    p.add_argument("--synthetic_sites", type=int, default=2040, help="synthetic: panel sites")
    p.add_argument("--synthetic_ref", type=int, default=256, help="synthetic: panel samples")
    p.add_argument("--mask_rate", type=float, default=0.3,
                   help="synthetic: fraction of panel sites absent from the target (C5 sweep 0.1..0.9)")
    p.add_argument("--no_vcf", action="store_true")
    p.add_argument("--vcf_writer", default="host", choices=["host", "device"],
                   help="host: the Python writer; device: the records formatted on the GPU (vcf_device.py), the same "
                        "file byte for byte")
    p.add_argument("--vcf_bgzf", action="store_true",
                   help="write imputed.vcf.gz (bgzipped: BGZF members and the EOF block) instead of imputed.vcf; with "
                        "--vcf_writer host through zlib, with --vcf_writer device deflated on the GPU (csrc/deflate.hip)")
    p.add_argument("--vcf_index", action="store_true",
                   help="with --vcf_bgzf: also write imputed.vcf.gz.tbi, the tabix index of the file (dataset/tbi.py), "
                        "from the offsets the writer already knows: no second pass over the file")
    p.add_argument("--vcf_info", action="store_true",
                   help="write AF, DR2, R2 and the IMP flag into the INFO column of imputed.vcf (per-site sums on the "
                        "GPU, csrc/quality.hip; quality.py); off: INFO stays '.'")
    p.add_argument("--truth_vcf", type=str, default=None,
                   help="a .vcf / .vcf.gz with the true genotypes: the imputed sites it holds are scored against it "
                        "(dosage r2, concordance, non-reference concordance by MAF bin) into quality.npz and accuracy.tsv")
    p.add_argument("--truth_region", default="all", choices=["all", "imputed"],
                   help="all: read the whole --truth_vcf; imputed: read only --chrom over the span of the imputed "
                        "positions, through the file's .tbi index (BGZF only).  The same scores either way; "
                        "quality.npz's truth_row counts from the first record read")
    p.add_argument("--maf_bins", type=str, default=None,
                   help="MAF bin edges of accuracy.tsv, comma separated (default 0,0.001,0.005,0.01,0.05,0.1,0.2,0.5)")
    p.add_argument("--panel_codes", default="u8", choices=["u8", "bits"],
                   help="layout of the HBM panel index: one byte per site, or bit-packed (1/8 of the memory, "
                        "identical neighbours)")
    p.add_argument("--device_features", action="store_true",
                   help="build the batches on the GPU from device-resident tables (dataset/device_features.py) and, "
                        "with one process, write the results straight into the site-major arrays; off by default, "
                        "identical outputs (0/1 genotypes only)")
    p.add_argument("--seed", type=int, default=0, help="weight init without --check_point (synthetic runs)")
    p.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                   help="WORLD_SIZE > 1 (torch.distributed.run, one process per GPU): nccl (= RCCL) or gloo "
                        "(host-staged: the multi-rank tests with every rank on one GPU)")
    p.add_argument("--vcf_inflate", default="host", choices=["host", "device"],
                   help="where BGZF .vcf.gz inputs are inflated: host (zlib) or device (csrc/inflate.hip, one wave "
                        "per block); the same arrays either way, files that are not BGZF stay on the host")
    p.add_argument("--ref_panel_pops", type=str, default=None,
                   help="the .panel file of --ref_panel (a .vcf / .vcf.gz): Freq.npy and the pos / pop maps are counted "
                        "from the panel's genotypes on the GPU (dataset/panel_stats.py) in place of --freq_path, "
                        "--pop_path, --pos_path and --type_path; nothing is written (build_panel_stats writes them)")
    p.add_argument("--vcf_site_columns", action="store_true",
                   help="carry CHROM, ID, REF and ALT of --ref_panel (a .vcf / .vcf.gz, read once with its strings cut "
                        "out on the GPU) and the sample names of a VCF --infer_dataset into imputed.vcf; the panel's "
                        "CHROM replaces --chrom; with --truth_vcf, a truth record with other alleles is not scored")
    p.add_argument("--vcf_sites", default="imputed", choices=["imputed", "all"],
                   help="imputed: imputed.vcf holds the sites the target lacks; all: one record per panel site, the "
                        "typed sites with the target's observed genotypes (overlaid on the GPU, csrc/typed.hip; "
                        "typed_sites.py) and, with --vcf_info, TYPED in place of IMP; needs --index_window_len equal "
                        "to --window_len")
    args = p.parse_args(argv)
    if args.vcf_sites == "all" and args.index_window_len != args.window_len:
        p.error("--vcf_sites all needs --index_window_len equal to --window_len: with other index windows the mask "
                "does not describe the sites the target lacks")
    if args.vcf_site_columns:
        if args.synthetic:
            p.error("--vcf_site_columns does not go with --synthetic")
        from .dataset.vcf_reader import is_vcf_path
        if not args.ref_panel or not is_vcf_path(args.ref_panel):
            p.error("--vcf_site_columns needs --ref_panel, a .vcf or .vcf.gz file")
    if args.vcf_index and not args.vcf_bgzf:
        p.error("--vcf_index needs --vcf_bgzf: a .tbi indexes a bgzipped file")
    if args.ref_panel_pops:
        given = [f"--{n}" for n in ("freq_path", "pop_path", "pos_path", "type_path") if getattr(args, n) is not None]
        if given:
            p.error(f"--ref_panel_pops builds the tables from --ref_panel: it does not go with {', '.join(given)}")
        if args.synthetic:
            p.error("--ref_panel_pops does not go with --synthetic")
        from .dataset.vcf_reader import is_vcf_path
        if not args.ref_panel or not is_vcf_path(args.ref_panel):
            p.error("--ref_panel_pops needs --ref_panel, a .vcf or .vcf.gz file")
    return args


def postprocess(probs_h1: torch.Tensor, probs_h2: torch.Tensor):
    """Device post-processing of one batch -> (p1 [B, L], p2 [B, L], gt [B, L, 4])."""
    from . import kernels as K
    return K.infer_post(probs_h1, probs_h2)


def geometry(h1, h2, gt, mask, n_windows: int, n_variants: int, window_len: int):
    """infer_embedding_rag.py:171-203 on stacked [W*S, L] arrays (window-major order)."""
    h1, h2 = h1[:, 1:1 + window_len], h2[:, 1:1 + window_len]
    gt, mask = gt[:, 1:1 + window_len], mask[:, 1:1 + window_len]
    S = h1.shape[0] // n_windows
    Lw = h1.shape[1]
    tr = lambda a: a.reshape(n_windows, S, Lw, *a.shape[2:]).swapaxes(1, 2).reshape(n_windows * Lw, S, *a.shape[2:])
    h1, h2, gt, mask = tr(h1), tr(h2), tr(gt), tr(mask)
    if h1.shape[0] >= n_variants:
        return h1[:n_variants], h2[:n_variants], gt[:n_variants], mask[:n_variants]
    pad = n_variants - h1.shape[0]
    padf = lambda a: np.pad(a, ((0, pad),) + ((0, 0),) * (a.ndim - 1))
    return padf(h1), padf(h2), padf(gt), padf(mask)


GT_MAP = ("0|0", "0|1", "1|0", "1|1")       # src/dataset/utils.py:15-20


def vcf_cells(h1, h2, gt):
    """Per-sample FORMAT cells GT:HDS:GP:DS of one site, as generate_vcf_efficient_optimized
    writes them (src/dataset/utils.py:406-461): GT = GT_MAP[argmax gt], HDS = (p1, p2),
    GP = (p00, p01 + p10, p11), DS = GP1 + 2 GP2, all '%.3f'."""
    g = np.argmax(gt, -1)
    gp0, gp1, gp2 = gt[..., 0], gt[..., 1] + gt[..., 2], gt[..., 3]
    ds = gp1 + 2 * gp2
    return [f"{GT_MAP[g[s]]}:{h1[s]:.3f},{h2[s]:.3f}:{gp0[s]:.3f},{gp1[s]:.3f},{gp2[s]:.3f}:{ds[s]:.3f}"
            for s in range(len(h1))]


class _BgzfText:
    """``open(path, "w")`` over ``BgzfWriter``: the same text, encoded the same way, as bgzipped members."""

    def __init__(self, path):
        import locale
        from .dataset.bgzf import BgzfWriter
        self.fh, self.encoding = BgzfWriter(path), locale.getpreferredencoding(False)

    def write(self, s: str) -> int:
        self.fh.write(s.encode(self.encoding))
        return len(s)

    def tell_virtual(self) -> int:
        return self.fh.tell_virtual()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fh.close()


def write_vcf(path, chrom, pos, h1, h2, gt, samples, pos_flag=None, ref=None, alt=None, bgzf=False, info=None,
              index=False, ids=None, typed=False):
    """VCF 4.2 records of the imputed sites (utils.py:378-479 layout: FORMAT GT:HDS:GP:DS,
    ID and REF/ALT '.' unless ``ids`` / ``ref`` / ``alt`` give one string per site row, QUAL 0, FILTER PASS).  ``pos_flag`` selects the sites
    written (the reference writes only flagged = imputed positions, infer_embedding_rag.py:237).
    ``bgzf``: the same text as a bgzipped file (BGZF members of 0xff00 bytes, zlib level 6, the EOF block).
    ``info``: one INFO string per site row (``quality.info_strings``: AF, DR2, R2, IMP) in place of '.', and the
    four ##INFO header lines that declare them.  ``typed`` (``--vcf_sites all``): the header also declares the
    TYPED flag (``vcf_device.TYPED_HEADER``); no record changes.
    ``index`` (needs ``bgzf``): also write the tabix index ``path + ".tbi"`` (dataset/tbi.py) from the virtual
    offsets the BGZF writer reports around every record: no second pass over the file, and no byte of the file
    itself changes.  A position >= 2^29 raises ``ValueError`` before anything is written."""
    if info is not None and len(info) != len(pos):
        raise ValueError("info must hold one string per site row")
    if index:
        if not bgzf:
            raise ValueError("index=True needs bgzf=True: a .tbi indexes a bgzipped file")
        from .dataset import tbi
        beg, end = tbi.vcf_intervals(pos, pos_flag, ref)
        voff = []
    with (_BgzfText(path) if bgzf else open(path, "w")) as f:
        f.write("##fileformat=VCFv4.2\n##source=rag-snvbert_amd\n")
        if info is not None:
            from .vcf_device import INFO_HEADER
            f.write(INFO_HEADER)
        if typed:
            from .vcf_device import TYPED_HEADER
            f.write(TYPED_HEADER)
        f.write('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype (argmax of GP)">\n')
        f.write('##FORMAT=<ID=HDS,Number=2,Type=Float,Description="Haplotype ALT dosages">\n')
        f.write('##FORMAT=<ID=GP,Number=3,Type=Float,Description="Genotype probabilities">\n')
        f.write('##FORMAT=<ID=DS,Number=1,Type=Float,Description="ALT dosage">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for i in range(len(pos)):
            if pos_flag is not None and not pos_flag[i]:
                continue
            r = ref[i] if ref is not None else "."
            a = alt[i] if alt is not None else "."
            inf = info[i] if info is not None else "."
            d = ids[i] if ids is not None else "."
            if index:
                voff.append(f.tell_virtual())
            f.write(f"{chrom}\t{int(pos[i])}\t{d}\t{r}\t{a}\t0.0\tPASS\t{inf}\tGT:HDS:GP:DS\t" +
                    "\t".join(vcf_cells(h1[i], h2[i], gt[i])) + "\n")
    if index:
        voff.append(f.tell_virtual())                      # closed: the EOF block's offset
        n = len(voff) - 1
        tbi.build([str(chrom)] if n else [], np.zeros(n, np.int64), beg, end, voff[:-1], voff[1:]).write(str(path) + ".tbi")


from .vcf_device import milli_f32, write_vcf_device  # noqa: E402  (the opt-in device writer of the same file)


def build_dataset(args):
    from .dataset.embedding_rag_infer_dataset import EmbeddingRAGInferDataset
    from .dataset.vocab import WordVocab
    if not args.synthetic:
        from .dataset.dataset import PanelData
        vocab = WordVocab(list(PanelData.from_file(args.infer_panel).pop_class_dict.keys()))
        extra = {}
        want_columns = bool(getattr(args, "vcf_site_columns", False))
        if getattr(args, "ref_panel_pops", None) or want_columns:
            # the panel VCF is read once: the same bit rows give the tables here and the kNN index later, and
            # with --vcf_site_columns the same read cuts out the strings of the output's CHROM / ID / REF / ALT
            from .dataset import vcf_reader
            dev = torch.device("cuda", torch.cuda.current_device())
            panel_vg = vcf_reader.read_vcf(args.ref_panel, dev, **({"columns": True} if want_columns else {}))
            extra = dict(ref_panel_vcf=panel_vg)
            if getattr(args, "ref_panel_pops", None):
                from .dataset.panel_stats import build_tables
                extra["tables"] = build_tables(panel_vg, args.ref_panel_pops, dev)
        ds = EmbeddingRAGInferDataset.from_file(vocab, args.infer_dataset, args.infer_panel, args.freq_path,
                                                args.type_path, args.pop_path, args.pos_path,
                                                ref_vcf_path=args.ref_panel, window_len=args.window_len,
                                                index_window_len=args.index_window_len, **extra)
        ds.set_panel_codes(args.panel_codes)
        return ds, vocab
    from .dataset.synthetic import make_infer_arrays, make_infer_dataset
    a = make_infer_arrays(args.synthetic_sites, args.synthetic, args.synthetic_ref, missing_rate=args.mask_rate,
                          seed=11)
    return make_infer_dataset(a, index_window_len=args.index_window_len, panel_codes=args.panel_codes)


def rank_rows(n_rows: int, rank: int, world: int):
    """The contiguous slice of the window-major sampler stream rank ``rank`` imputes: whole
    sample-windows, ranks in stream order, so each rank touches few windows (few panel-index
    builds) and the gather is a concatenation in rank order."""
    return n_rows * rank // world, n_rows * (rank + 1) // world


def _gather_rows(t: torch.Tensor, sizes, group=None) -> torch.Tensor:
    """Concatenate every rank's rows (ragged counts ``sizes``) in rank order."""
    from .retrieval.shards import _all_gather
    pad = max(sizes)
    if t.shape[0] < pad:
        t = torch.cat([t, t.new_zeros((pad - t.shape[0],) + tuple(t.shape[1:]))])
    g = _all_gather(t.contiguous(), group)
    return torch.cat([g[r, :n] for r, n in enumerate(sizes)])


OUTPUT_BUDGET_BYTES = 16 << 30      # device result arrays of the device_features output path


def run(ds, model, dev, batch_size: int, k: int, num_workers: int = 0, window_len: int = INFER_WINDOW_LEN,
        group=None, device_features: bool = False, output_budget_bytes: int = OUTPUT_BUDGET_BYTES,
        keep_site_dev: bool = False):
    """The inference loop (infer_embedding_rag.py:132-157) and geometry (:165-203) over ``ds``
    with an eval ``model`` on ``dev``.  Returns host arrays h1/h2 [n_sites, S], gt
    [n_sites, S, 4], mask [n_sites, S], the neighbour indices per sampler row and the time.

    Several ranks (``torch.distributed`` initialised, configs[4]): the panel is replicated,
    rank r imputes rows ``rank_rows`` of the window-major stream (batches formed inside its
    slice), and the per-row outputs are all-gathered in stream order before the geometry — the
    same arrays as one process (every row's retrieval and forward depend on that row alone).
    ``seconds`` is the slowest rank's loop time.

    ``device_features``: the batches come from ``DeviceBatchLoader`` (built on the GPU, same sampler
    rows).  With one process the per-batch outputs also go through ``kernels.infer_scatter`` into
    device result arrays [n_sites, S] (32 bytes per site and sample), copied to the host once — in
    place of the concatenation and the host ``geometry``; the per-row ``batch_*`` entries are then
    None.  If the arrays would exceed ``output_budget_bytes`` (default 16 GiB), or with several
    ranks, the existing output path runs (with a printed note) and only the input side changes.
    ``keep_site_dev``: when that scatter path ran, the device arrays h1 / h2 / gt are also returned under
    ``site_dev`` (for ``write_vcf_device``, which formats from them in place); the caller frees them."""
    from . import kernels as K
    from .dataset.embedding_rag_dataset import embedding_rag_collate_fn
    from .dataset.sampler import WindowMajorSampler
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    emb = model.bert.embedding
    order = list(iter(WindowMajorSampler(ds)))
    lo, hi = rank_rows(len(order), rank, world)
    site = None                      # device result arrays of the scatter output path
    if device_features:
        from .dataset.device_features import DeviceBatchLoader
        loader = DeviceBatchLoader(ds, order[lo:hi], batch_size, dev)
        n_sites, S = len(ds.ori_pos), len(order) // max(ds.window_count, 1)
        need = 32 * n_sites * S
        if world > 1:
            pass                     # ranks hold disjoint rows: the per-row gather and host geometry stay
        elif need > output_budget_bytes:
            print(f"device_features: site-major result arrays need {need} bytes > output_budget_bytes "
                  f"{output_budget_bytes}; keeping the per-batch outputs and the host geometry", flush=True)
        else:
            site = dict(h1=torch.zeros(n_sites, S, device=dev), h2=torch.zeros(n_sites, S, device=dev),
                        gt=torch.zeros(n_sites, S, 4, device=dev),
                        mask=torch.zeros(n_sites, S, device=dev, dtype=torch.long))
            masked = torch.zeros((), device=dev, dtype=torch.long)
    else:
        loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=order[lo:hi],
                                             num_workers=num_workers, collate_fn=embedding_rag_collate_fn)
    outs = {"h1": [], "h2": [], "gt": [], "mask": [], "idx1": [], "idx2": []}
    t0 = time.perf_counter()
    with torch.no_grad():
        for batch in loader:
            batch = ds.process_batch_retrieval(batch, emb, dev, k)
            x = {key: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for key, v in batch.items()}
            out = model(x)
            if site is not None:
                K.infer_scatter(out[0].float().contiguous(), out[1].float().contiguous(), x["mask"], batch.rows_dev,
                                batch.rows_host, min(window_len, MAX_SEQ_LEN - 1), site["h1"], site["h2"],
                                site["gt"], site["mask"])
                masked += x["mask"].sum()
            else:
                p1, p2, gt = postprocess(out[0], out[1])
                outs["h1"].append(p1)
                outs["h2"].append(p2)
                outs["gt"].append(gt)
                outs["mask"].append(x["mask"])
            outs["idx1"].append(x["rag_idx_h1"])
            outs["idx2"].append(x["rag_idx_h2"])
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if site is not None:
        host = {key: v.cpu().numpy() for key, v in site.items()}
        for key in ("idx1", "idx2"):
            host[key] = torch.cat(outs[key]).cpu().numpy()
        res = dict(h1=host["h1"], h2=host["h2"], gt=host["gt"], mask=host["mask"], idx1=host["idx1"],
                   idx2=host["idx2"], seconds=elapsed, masked_snvs=int(masked.item()) * 2, batch_mask=None,
                   batch_h1=None, batch_h2=None)
        if keep_site_dev:
            res["site_dev"] = dict(h1=site["h1"], h2=site["h2"], gt=site["gt"])
        return res
    if world > 1:
        sizes = [rank_rows(len(order), r, world)[1] - rank_rows(len(order), r, world)[0] for r in range(world)]
        full = {}
        for key, v in outs.items():
            loc = torch.cat(v) if v else _empty_rows(key, dev, k)
            loc = loc.long() if key in ("idx1", "idx2", "mask") else loc.float()   # one dtype on every rank
            full[key] = _gather_rows(loc, sizes, group)
        outs = {key: [t] for key, t in full.items()}
        from .retrieval.shards import _all_reduce
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        elapsed = float(_all_reduce(t, dist.ReduceOp.MAX, group).item())
    host = {key: torch.cat(v).cpu().numpy() for key, v in outs.items()}
    h1, h2, gt, mask = geometry(host["h1"], host["h2"], host["gt"], host["mask"], ds.window_count,
                                len(ds.ori_pos), window_len)
    return dict(h1=h1, h2=h2, gt=gt, mask=mask, idx1=host["idx1"], idx2=host["idx2"], seconds=elapsed,
                masked_snvs=int(host["mask"].sum()) * 2, batch_mask=host["mask"], batch_h1=host["h1"],
                batch_h2=host["h2"])


def _empty_rows(key, dev, k):
    """A rank with no rows (more ranks than sample-windows) contributes zero-row tensors."""
    shape = {"gt": (0, MAX_SEQ_LEN, 4), "idx1": (0, k), "idx2": (0, k)}.get(key, (0, MAX_SEQ_LEN))
    dt = torch.long if key in ("idx1", "idx2", "mask") else torch.float32
    return torch.zeros(shape, device=dev, dtype=dt)


def panel_site_columns(ds, default_chrom: str):
    """``--vcf_site_columns``: the output's CHROM and, per row of ``ds.ori_pos``, the ID, REF and ALT strings of
    the first panel record at that POS (the rule ``_build_embedding_indexes`` maps genotypes by); '.' where the
    panel VCF does not hold the site.  Returns dict(chrom, ids, ref, alt (lists of str), rows (the panel record
    of each row, -1 none), columns (the panel's ``SiteColumns``)).  The bytes are decoded with the encoding the
    writers encode with.  ``ValueError``: two CHROM values among the mapped records, or a record that does
    not decode (names its POS)."""
    import locale
    vg = ds.ref_panel_vcf
    if vg is None or vg.columns is None:
        raise ValueError("--vcf_site_columns: the panel was not read from a VCF with columns=True")
    cols, encoding = vg.columns, locale.getpreferredencoding(False)
    first = {}
    for i, p in enumerate(np.asarray(vg.pos).tolist()):
        first.setdefault(p, i)
    ori_pos = np.asarray(ds.ori_pos).tolist()
    rows = np.array([first.get(p, -1) for p in ori_pos], dtype=np.int64)
    chrom, out = None, dict(ids=[], ref=[], alt=[])
    for p, r in zip(ori_pos, rows.tolist()):
        if r < 0:
            for v in out.values():
                v.append(".")
            continue
        try:
            c = cols.chrom(r).decode(encoding)
            strings = [cols.get(name, r).decode(encoding) for name in ("id", "ref", "alt")]
        except UnicodeDecodeError as e:
            raise ValueError(f"--vcf_site_columns: the panel record at POS {p} does not decode as {encoding}: {e}") from None
        if chrom is None:
            chrom = c
        elif c != chrom:
            raise ValueError(f"--vcf_site_columns: the panel records at the imputed sites name two sequences, "
                             f"{chrom!r} and {c!r} (POS {p}); one output file holds one CHROM")
        for v, t in zip(out.values(), strings):
            v.append(t)
    return dict(out, chrom=default_chrom if chrom is None else chrom, rows=rows, columns=cols)


def site_quality(args, ds, dev, src, flag, chrom=None, site_cols=None):
    """``--vcf_info`` / ``--truth_vcf`` on rank 0: the per-site sums of ``src`` (h1 / h2 / gt, device tensors or
    host arrays) by the kernel (quality.py).  Returns the INFO strings for the writers (None without
    ``--vcf_info``); with ``--truth_vcf`` also writes quality.npz and accuracy.tsv and prints the ALL row.  The
    imputed sites (``flag``, what the VCF writer selects) that the truth file holds are the ones evaluated.
    ``chrom``: the sequence ``--truth_region imputed`` asks for (default ``--chrom``).  ``site_cols``
    (``panel_site_columns``, with ``--vcf_site_columns``): the truth file is read with its strings, and a matched
    site whose (REF, ALT) differs from the panel's is not scored (``truth_row`` -1; counted in quality.npz's
    ``allele_mismatch`` and on the printed ALL line)."""
    chrom = args.chrom if chrom is None else chrom
    from . import kernels as K
    from . import quality as Q
    S = src["h1"].shape[1]
    ori_pos = np.asarray(ds.ori_pos)
    truth = row = col = None
    if args.truth_vcf:
        from .dataset.vcf_reader import read_vcf
        region = None
        if args.truth_region == "imputed":               # through the .tbi: only the members that span touches
            imputed = ori_pos[np.asarray(flag, bool)]
            region = (chrom, int(imputed.min()), int(imputed.max())) if imputed.size else (chrom, 1, 0)
        tv = read_vcf(args.truth_vcf, dev, region=region, **({} if site_cols is None else {"columns": True}))
        vg = getattr(ds, "vcf_genotypes", None)
        row, col = Q.truth_maps(tv, ori_pos, None if vg is None else list(vg.samples), n_samples=S)
        row = np.where(flag, row, -1).astype(np.int32)
        extra = {}
        if site_cols is not None:                        # the same position, other alleles: another variant
            pc, tc, mismatch = site_cols["columns"], tv.columns, 0
            for i in np.flatnonzero((row >= 0) & (site_cols["rows"] >= 0)).tolist():
                r, t = int(site_cols["rows"][i]), int(row[i])
                if (pc.ref(r), pc.alt(r)) != (tc.ref(t), tc.alt(t)):
                    row[i] = -1
                    mismatch += 1
            extra["allele_mismatch"] = np.int64(mismatch)
        if tv.n_sites and (row >= 0).any():
            truth = K.vcf_unpack_gt(tv.alt_bits, tv.miss_bits, tv.n_sites)      # device i8, no host round trip
    est, acc, table = Q.site_stats(src["h1"], src["h2"], src["gt"], truth, row, col, device=dev)
    af, r2, dr2 = Q.estimates(est, S)
    if args.truth_vcf:
        if truth is None:
            acc, table = np.zeros((len(ori_pos), 3)), np.zeros((len(ori_pos), 9), np.int32)
        cols = np.asarray(getattr(ds, "_freq_col", np.arange(len(ori_pos))))
        gaf = np.asarray(ds.freq[3][5], np.float64)[cols]
        maf = np.minimum(gaf, 1 - gaf)
        site = Q.accuracy(acc, table)
        sel = row >= 0
        rows = Q.aggregate(acc[sel], table[sel], maf[sel], Q.parse_maf_bins(args.maf_bins))
        np.savez_compressed(os.path.join(args.output_path, "quality.npz"), pos=ori_pos, flag=flag, est=est, af=af,
                            r2=r2, dr2=dr2, acc=acc, table=table, truth_row=row, maf=maf, acc_n=site["n"],
                            acc_r2=site["r2"], concordance=site["concordance"],
                            nonref_concordance=site["nonref_concordance"], **extra)
        text = Q.accuracy_tsv(rows)
        with open(os.path.join(args.output_path, "accuracy.tsv"), "w") as f:
            f.write(text)
        print("accuracy vs truth  " + text.splitlines()[0].replace("\t", " "), flush=True)
        print("accuracy vs truth  " + text.splitlines()[-1].replace("\t", " ") +
              "".join(f"  {k}={int(v)}" for k, v in extra.items()), flush=True)
    if not (args.vcf_info and not args.no_vcf):
        return None
    # --vcf_sites all: every row is written, the typed ones flagged TYPED in place of IMP
    return Q.info_strings(af, r2, dr2, imputed=flag if getattr(args, "vcf_sites", "imputed") == "all" else None)


def overlay_typed_sites(ds, dev, h1, h2, gt, mask, site_dev=None):
    """``--vcf_sites all`` on rank 0: the target's observed genotypes over the rows of the typed sites
    (typed_sites.py, csrc/typed.hip).  With ``site_dev`` (the scatter path's device arrays) the overlay runs on
    them in place and the typed rows of the host arrays h1 / h2 / gt are refreshed from them; else the host arrays
    go through the kernel in chunks of their typed rows.  Returns (typed bool [n], typed_missing int32 [n]: the
    cells of each typed row left as the model's output because a call is missing).  ``ValueError`` when the mask
    of the first sample is not the sites the target lacks (names the first site that differs)."""
    from . import typed_sites as T
    flag, need = mask[:, 0].astype(bool), np.asarray(ds.position_needed, bool)
    if flag.shape != need.shape or (flag != need).any():
        i = int(np.flatnonzero(flag != need)[0]) if flag.shape == need.shape else min(len(flag), len(need))
        raise ValueError(f"--vcf_sites all: the mask does not describe the sites the target lacks (first at site row "
                         f"{i}, POS {int(np.asarray(ds.ori_pos)[i]) if i < len(ds.ori_pos) else -1})")
    site_row, col = T.target_maps(ds)
    target = T.target_bit_rows(ds, dev)
    if site_dev is not None:
        missing = T.typed_overlay(site_dev["h1"], site_dev["h2"], site_dev["gt"], target, site_row, col)
        rows = np.flatnonzero(site_row >= 0)
        d_rows = torch.from_numpy(rows).to(dev)
        for host, key in ((h1, "h1"), (h2, "h2"), (gt, "gt")):
            host[rows] = site_dev[key].index_select(0, d_rows).cpu().numpy()
    else:
        missing = T.typed_overlay(h1, h2, gt, target, site_row, col, device=dev)
    typed = ~flag
    print(f"--vcf_sites all: {int(typed.sum())} typed sites of {len(typed)} carry the target's genotypes; "
          f"{int(missing.sum())} cells keep the model's output because a call is missing", flush=True)
    return typed, missing


def infer(argv=None):
    args = parse_args(argv)
    from .dataset.vcf_reader import set_default_inflate
    set_default_inflate(args.vcf_inflate)
    if not torch.cuda.is_available():
        raise SystemExit("imputation runs on the MI355X kernels only (no CPU fallback)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        dev = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
    else:
        dev = torch.device(f"cuda:{args.cuda_devices[0] if args.cuda_devices else torch.cuda.current_device()}")
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    from .engine import engine_for
    from .model import build_model
    ds, vocab = build_dataset(args)
    torch.manual_seed(args.seed)          # every rank (and every run) builds the same random-init weights
    model = build_model(len(vocab), args.dims, args.layers, args.attn_heads)
    if args.check_point:
        # a trainer checkpoint of either build: the reference's pickled module (its classes
        # stubbed, nothing executed), a state_dict / {'state_dict'} / {'model'} (model/checkpoint.py)
        from .model.checkpoint import load_state_dict_any
        sd = load_state_dict_any(args.check_point)
        # strict: a missing or renamed key must not silently impute with random-init weights
        # (the reference loads with strict=False, infer_embedding_rag.py:99)
        model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    engine_for(model).set_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    want_quality = bool(args.truth_vcf) or (args.vcf_info and not args.no_vcf)
    all_sites = args.vcf_sites == "all"
    res = run(ds, model, dev, args.infer_batch_size, args.k_retrieve, args.num_workers, args.window_len,
              device_features=args.device_features,
              keep_site_dev=(args.vcf_writer == "device" and not args.no_vcf) or want_quality or all_sites)
    h1, h2, gt, mask = res["h1"], res["h2"], res["gt"], res["mask"]
    site_dev = res.pop("site_dev", None)
    if rank != 0:                      # the gathered arrays are written once
        return res
    os.makedirs(args.output_path, exist_ok=True)
    extra_keys = {}
    if all_sites:
        # before anything reads the arrays: the npz, both writers and the quality kernel see the overlaid values
        typed, typed_missing = overlay_typed_sites(ds, dev, h1, h2, gt, mask, site_dev)
        extra_keys = dict(typed=typed, typed_missing=typed_missing)
    np.savez_compressed(os.path.join(args.output_path, "imputed.npz"), hap1=h1, hap2=h2, gp=gt, mask=mask,
                        pos=np.asarray(ds.ori_pos), **extra_keys)
    flag = mask[:, 0].astype(bool)
    info = None
    chrom, site_cols, written = args.chrom, None, {}
    if args.vcf_site_columns:
        site_cols = panel_site_columns(ds, args.chrom)
        chrom = site_cols["chrom"]
        if chrom != args.chrom:
            print(f"--vcf_site_columns: CHROM is the panel's {chrom!r}, not --chrom {args.chrom!r}", flush=True)
        written = dict(ids=site_cols["ids"], ref=site_cols["ref"], alt=site_cols["alt"])
    if want_quality:
        # in place from the scatter path's device arrays when there are any, else the host arrays through the
        # chunked upload (several ranks: the gathered ones)
        info = site_quality(args, ds, dev, site_dev if site_dev is not None else dict(h1=h1, h2=h2, gt=gt), flag,
                            chrom, site_cols)
    if not args.no_vcf:
        samples = [f"S{i}" for i in range(h1.shape[1])]
        target = getattr(ds, "vcf_genotypes", None)
        if args.vcf_site_columns and target is not None and len(target.samples) == len(samples):
            samples = list(target.samples)
        vcf_path = os.path.join(args.output_path, "imputed.vcf.gz" if args.vcf_bgzf else "imputed.vcf")
        if all_sites:                  # one record per row of ds.ori_pos; the TYPED flag is declared where it is used
            written = dict(written, typed=info is not None)
        pos_flag = None if all_sites else flag
        if args.vcf_writer == "device":
            # in place from the scatter path's device arrays when there are any, else the host arrays
            # (several ranks: the gathered ones) uploaded chunk by chunk
            src = site_dev if site_dev is not None else dict(h1=h1, h2=h2, gt=gt)
            write_vcf_device(vcf_path, chrom, ds.ori_pos, src["h1"], src["h2"], src["gt"], samples,
                             pos_flag=pos_flag, device=dev, bgzf=args.vcf_bgzf, info=info, index=args.vcf_index, **written)
            src = None
        else:
            write_vcf(vcf_path, chrom, ds.ori_pos, h1, h2, gt, samples, pos_flag=pos_flag, bgzf=args.vcf_bgzf,
                      info=info, index=args.vcf_index, **written)
    site_dev = None                    # the device result arrays are freed after the last reader
    print(f"imputed {len(ds)} sample-windows in {res['seconds']:.2f}s "
          f"({res['masked_snvs'] / res['seconds']:.0f} masked SNVs/s)", flush=True)
    return res


if __name__ == "__main__":
    infer(sys.argv[1:])
