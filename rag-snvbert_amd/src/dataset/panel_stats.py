"""Freq.npy and the pos / pop maps of a reference panel, counted from its VCF on the GPU.

The reference builds these tables in ``prepare_data_v4_0411.py:116-231`` from four per-population CSVs of allele
and genotype frequencies that no program of the reference produces.  Every number in them is a count over the
panel's genotypes, and ``read_vcf`` already leaves those on the device as bit rows, so they are counted here
(``csrc/panel_stats.hip``, one pass over the rows) and divided:

``counts``  int32 [6, 5, n_sites]: row p < P is population p of ``sorted(unique labels)``, rows P..4 are zero,
            row 5 (``dataset.GLOBAL``) is the whole panel.  Columns per site: ``n_ref``, ``n_het``, ``n_hom`` = the
            samples with both alleles called and 0, 1 or 2 ALT alleles (any allele number > 0 is ALT); ``n_alt`` =
            the called alleles that are ALT; ``n_called`` = the called alleles.  A haploid or half-missing call
            adds to ``n_alt`` / ``n_called`` only.
``freq``    float32 [4, 6, n_sites], layers REF / HET / HOM / AF: ``n_ref``, ``n_het``, ``n_hom`` over their sum, and
            ``n_alt / n_called``; each quotient in float64, rounded once to float32; 0.0 over a zero denominator.

``panel_counts_host`` is the specification of the kernel; ``build_tables`` is what the entry points call.
"""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

N_REF, N_HET, N_HOM, N_ALT, N_CALLED = range(5)
GLOBAL = 5                                   # dataset.GLOBAL: the whole-panel row of Freq.npy
MAX_POPS = GLOBAL


def read_panel_file(path) -> Tuple[List[str], List[str]]:
    """(sample names, population labels) of a ``.panel`` file: one header line, then ``sample pop super_pop ...``;
    the label is the third column, as ``PanelData.from_file`` takes it."""
    names, pops = [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if lineno == 1 or not line.strip():
                continue
            cols = line.split()
            if len(cols) < 3:
                raise ValueError(f"{path}: line {lineno}: expected sample, pop and super_pop columns")
            names.append(cols[0])
            pops.append(cols[2])
    return names, pops


def population_order(vcf_samples: Sequence[str], names: Sequence[str], pops: Sequence[str]):
    """(pop_list, order int32 [S], pop_start int32 [P + 1]) for the samples of a VCF: ``pop_list`` =
    ``sorted(unique)`` of the labels of the samples present in the VCF (prepare_data_v4_0411.py:181), ``order``
    the VCF's sample numbers sorted by population (stable), population p owning
    ``order[pop_start[p]:pop_start[p + 1]]``.  Samples are matched by name; panel-file samples absent from the
    VCF are ignored."""
    label: Dict[str, str] = {}
    for n, p in zip(names, pops):
        if n in label:
            raise ValueError(f"sample {n!r} is listed twice in the panel file")
        label[n] = p
    seen = set()
    for n in vcf_samples:
        if n in seen:
            raise ValueError(f"sample {n!r} is listed twice in the VCF header")
        seen.add(n)
        if n not in label:
            raise ValueError(f"sample {n!r} of the VCF is not in the panel file")
    pop_list = sorted({label[n] for n in vcf_samples})
    if len(pop_list) > MAX_POPS:
        raise ValueError(f"{len(pop_list)} populations ({', '.join(pop_list)}): at most {MAX_POPS} fit, row "
                         f"{GLOBAL} of the tables is 'Global'")
    idx = {p: i for i, p in enumerate(pop_list)}
    key = np.array([idx[label[n]] for n in vcf_samples], np.int64)
    order = np.argsort(key, kind="stable").astype(np.int32)
    pop_start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=len(pop_list)))]).astype(np.int32)
    return pop_list, order, pop_start


def panel_counts_host(gt: np.ndarray, order: np.ndarray, pop_start: np.ndarray, P: int) -> np.ndarray:
    """The specification of ``snvrag_panel_counts``: int32 [6, 5, n_sites] from allele numbers ``gt`` int8
    [n_sites, S, 2] (any allele > 0 is ALT, -1 is missing)."""
    gt = np.asarray(gt)
    n = gt.shape[0]
    out = np.zeros((6, 5, n), np.int32)
    called, alt = gt >= 0, gt > 0
    both = called.all(-1)
    n_alt_s = alt.sum(-1)
    rows = [(p, np.asarray(order[pop_start[p]:pop_start[p + 1]], np.int64)) for p in range(P)]
    rows.append((GLOBAL, np.concatenate([r for _, r in rows]) if rows else np.zeros(0, np.int64)))
    for row, s in rows:
        b, k = both[:, s], n_alt_s[:, s]
        out[row, N_REF] = (b & (k == 0)).sum(1)
        out[row, N_HET] = (b & (k == 1)).sum(1)
        out[row, N_HOM] = (b & (k == 2)).sum(1)
        out[row, N_ALT] = alt[:, s].sum((1, 2))
        out[row, N_CALLED] = called[:, s].sum((1, 2))
    return out


def freq_from_counts(counts: np.ndarray) -> np.ndarray:
    """float32 [4, 6, n_sites] (REF, HET, HOM, AF) of ``counts`` int32 [6, 5, n_sites]: each quotient in float64,
    rounded once to float32; 0.0 where the denominator is 0."""
    c = np.asarray(counts).astype(np.float64)
    geno = c[:, N_REF] + c[:, N_HET] + c[:, N_HOM]
    out = np.zeros((4,) + geno.shape, np.float64)
    for layer, num, den in ((0, c[:, N_REF], geno), (1, c[:, N_HET], geno), (2, c[:, N_HOM], geno),
                            (3, c[:, N_ALT], c[:, N_CALLED])):
        np.divide(num, den, out=out[layer], where=den > 0)
    return out.astype(np.float32)


def maps(pop_list: Sequence[str], pos) -> Tuple[Dict[str, int], Dict[int, int]]:
    """(pop_to_idx, pos_to_idx): ``{pop: i}`` plus ``'Global': 5``, and ``{int(POS): row}`` in file order
    (prepare_data_v4_0411.py:185-186, :201).  A POS that occurs twice raises: the reader does not split
    multi-allelic records, the panel index would take the first row and a dict the last."""
    pop_to_idx = {str(p): i for i, p in enumerate(pop_list)}
    pop_to_idx["Global"] = GLOBAL
    pos_to_idx: Dict[int, int] = {}
    for i, p in enumerate(np.asarray(pos).tolist()):
        if p in pos_to_idx:
            raise ValueError(f"POS {p} occurs twice in the panel (records {pos_to_idx[p]} and {i}): split or drop "
                             "multi-allelic records first")
        pos_to_idx[int(p)] = i
    return pop_to_idx, pos_to_idx


def build_tables(vg, panel_file, device=None) -> dict:
    """The tables of a panel from its ``VcfGenotypes`` (already on the device; the file is not read again) and its
    ``.panel`` file: ``dict(freq, pop_to_idx, pos_to_idx, type_to_idx={}, counts)``, ``freq`` and ``counts`` host
    arrays.  One kernel launch over the bit rows and one copy of the counts to the host."""
    import torch
    from .. import kernels as K
    names, pops = read_panel_file(panel_file)
    pop_list, order, pop_start = population_order(vg.samples, names, pops)
    pop_to_idx, pos_to_idx = maps(pop_list, vg.pos)
    dev = vg.alt_bits.device
    want = dev if device is None else torch.device(device)
    if want.type != dev.type or (want.index is not None and want.index != dev.index):
        raise ValueError(f"the panel's bit rows are on {dev}, not on {want}")
    if vg.n_sites:
        counts = K.panel_counts(vg.alt_bits, vg.miss_bits, vg.n_sites, torch.from_numpy(order).to(dev),
                                torch.from_numpy(pop_start).to(dev)).cpu().numpy()
    else:
        counts = np.zeros((6, 5, 0), np.int32)
    return dict(freq=freq_from_counts(counts), pop_to_idx=pop_to_idx, pos_to_idx=pos_to_idx, type_to_idx={},
                counts=counts)
