"""Freq.npy and the mapping pickles of a reference panel, from its VCF and its ``.panel`` file
(reference: prepare_data_v4_0411.py:116-231, which needs scikit-allel, h5py, pandas and four per-population
frequency CSVs that nothing in the reference writes).

    python -m src.build_panel_stats --ref_panel panel.vcf.gz --ref_panel_pops panel.panel -o tables/

The panel is read once by the device VCF reader and its genotypes are counted per site and population on the
GPU (dataset/panel_stats.py, csrc/panel_stats.hip).  Written into the output directory, in the formats the
datasets' ``from_file`` reads (``--freq_path`` / ``--pop_path`` / ``--pos_path`` / ``--type_path`` of
``infer_embedding_rag`` and ``train_embedding_rag``):

    Freq.npy         float32 [4, 6, n_sites]: REF / HET / HOM / AF per population row and 'Global' (row 5)
    pop_to_idx.bin   pickle {population: row, 'Global': 5}
    pos_to_idx.bin   pickle {POS: column}, in file order
    type_to_idx.bin  pickle {} (read by no code path)
    counts.npy       int32 [6, 5, n_sites]: n_ref, n_het, n_hom, n_alt, n_called behind every quotient
"""

from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np

FILES = dict(freq="Freq.npy", pop_to_idx="pop_to_idx.bin", pos_to_idx="pos_to_idx.bin",
             type_to_idx="type_to_idx.bin", counts="counts.npy")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="panel frequency tables from a VCF (MI355X)")
    p.add_argument("--ref_panel", type=str, required=True, help="the panel's .vcf / .vcf.gz")
    p.add_argument("--ref_panel_pops", type=str, required=True,
                   help="the panel's .panel file: a header line, then sample pop super_pop (the label is column 3)")
    p.add_argument("-o", "--output_dir", type=str, required=True)
    p.add_argument("--vcf_inflate", default="host", choices=["host", "device"],
                   help="where a BGZF .vcf.gz is inflated: host (zlib) or device (csrc/inflate.hip)")
    args = p.parse_args(argv)
    from .dataset.vcf_reader import is_vcf_path
    if not is_vcf_path(args.ref_panel):
        p.error("--ref_panel must be a .vcf or .vcf.gz file")
    return args


def write_tables(tables: dict, output_dir) -> dict:
    """The five files of ``tables`` (``panel_stats.build_tables``) in ``output_dir``; returns their paths by key."""
    os.makedirs(output_dir, exist_ok=True)
    paths = {k: os.path.join(str(output_dir), name) for k, name in FILES.items()}
    np.save(paths["freq"], tables["freq"])
    np.save(paths["counts"], tables["counts"])
    for k in ("pop_to_idx", "pos_to_idx", "type_to_idx"):
        with open(paths[k], "wb") as f:
            pickle.dump(tables[k], f)
    return paths


def main(argv=None) -> dict:
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("the panel is parsed and counted by the MI355X kernels only (no CPU fallback)")
    from .dataset.panel_stats import build_tables
    from .dataset.vcf_reader import read_vcf
    dev = torch.device("cuda", torch.cuda.current_device())
    vg = read_vcf(args.ref_panel, dev, inflate=args.vcf_inflate)
    tables = build_tables(vg, args.ref_panel_pops, dev)
    paths = write_tables(tables, args.output_dir)
    print(f"[build_panel_stats] {vg.n_sites} sites, {len(vg.samples)} samples, "
          f"{len(tables['pop_to_idx']) - 1} populations -> {args.output_dir}", flush=True)
    return paths


if __name__ == "__main__":
    main(sys.argv[1:])
