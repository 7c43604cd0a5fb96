"""Per-site imputation quality (opt-in: ``--vcf_info``, ``--truth_vcf``): the INFO fields AF / DR2 / R2 of the
imputed VCF, and accuracy against a truth VCF by minor-allele frequency.

Both are one reduction over the samples of every site of the site-major result arrays h1 / h2 [n, S] and
gt [n, S, 4] (csrc/quality.hip ``snvrag_site_stats``).  ``site_stats_host`` is its specification in numpy;
``site_stats`` runs the kernel on device tensors in place or on host arrays uploaded in row chunks.  What
follows the sums is float64 arithmetic on [n]-sized arrays on the host: ``estimates`` (AF, Minimac-style R2,
Beagle-style DR2), ``accuracy`` (dosage r2, concordance, non-reference concordance per site) and ``aggregate``
(the same per MAF bin).

Per sample of a site, in float32 exactly as the VCF writers compute them: gp1 = gt[1] + gt[2],
ds = gp1 + 2 gt[3]; then in float64 e = ds and f = gp1 + 4 gt[3] (the second moment of the dosage under GP).

  est   [n, 5]  sum h1 + h2, sum h1^2 + h2^2, sum e, sum e^2, sum f                     over the S samples
  table [n, 9]  table[3 t + c] += 1: t the true ALT count, c the ALT count of the called genotype (the G the
                writers print: the scan best = gt[0], k wins when gt[k] > best — the first maximum, never a NaN)
  acc   [n, 3]  sum e, sum e^2, sum e t
table and acc run over the samples with a truth column whose two truth alleles are called, at the sites with
a truth row; a site without one gets zeros.  A multi-allelic truth record counts any ALT allele as 1 (the
reader maps it so).
"""

from __future__ import annotations

import numpy as np

DEFAULT_MAF_EDGES = (0.0, 0.001, 0.005, 0.01, 0.05, 0.1, 0.2, 0.5)
DEFAULT_CHUNK_BYTES = 256 << 20
CELL_BYTES = 24                     # h1, h2 and the four gt values of one site and sample
TSV_COLUMNS = ("maf_bin", "sites", "genotypes", "mean_r2", "pooled_r2", "concordance", "nonref_concordance")


def _f32(a, name):
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name} must be float32")
    return a


def _index(a, count, bound, name):
    """An index array as int64 with everything outside [0, bound) set to -1."""
    a = np.asarray(a).astype(np.int64).reshape(-1)
    if a.shape[0] != count:
        raise ValueError(f"{name} must hold {count} entries, not {a.shape[0]}")
    return np.where((a >= 0) & (a < bound), a, -1)


def called_alt_count(gt) -> np.ndarray:
    """ALT count (0, 1, 1, 2) of the genotype the writers print for gt [..., 4]: the first maximum."""
    gt = np.asarray(gt)
    best, am = gt[..., 0].copy(), np.zeros(gt.shape[:-1], np.int64)
    for k in (1, 2, 3):
        win = gt[..., k] > best
        best = np.where(win, gt[..., k], best)
        am = np.where(win, k, am)
    return (am >> 1) + (am & 1)


def site_stats_host(h1, h2, gt, truth=None, truth_row=None, truth_col=None, block_rows: int = 64):
    """The specification of ``snvrag_site_stats`` (module docstring) in numpy float64, without a GPU call:
    (est f64 [n, 5], acc f64 [n, 3], table i32 [n, 9]); acc and table are None without ``truth``
    (i8 [n_truth, S_truth, 2]: 0 / 1, -1 missing; ``truth_row`` [n], ``truth_col`` [S], -1 or out of range: none)."""
    h1, h2, gt = _f32(h1, "h1"), _f32(h2, "h2"), _f32(gt, "gt")
    n, S = h1.shape
    if h2.shape != (n, S) or gt.shape != (n, S, 4):
        raise ValueError("h1 / h2 [n, S] and gt [n, S, 4] do not agree")
    est = np.zeros((n, 5), np.float64)
    if truth is None:
        acc = table = None
    else:
        if truth_row is None or truth_col is None:
            raise ValueError("truth needs truth_row and truth_col")
        truth = np.asarray(truth)
        if truth.ndim != 3 or truth.shape[2] != 2:
            raise ValueError("truth must be [n_truth, S_truth, 2]")
        row = _index(truth_row, n, truth.shape[0], "truth_row")
        col = _index(truth_col, S, truth.shape[1], "truth_col")
        acc, table = np.zeros((n, 3), np.float64), np.zeros((n, 9), np.int32)
    for lo in range(0, n, block_rows):
        sl = slice(lo, min(lo + block_rows, n))
        g = gt[sl]
        gp1 = g[..., 1] + g[..., 2]                                   # float32, as the writers
        ds = gp1 + np.float32(2) * g[..., 3]                          # 2 gt[3] is exact: one rounding
        e = ds.astype(np.float64)
        f = gp1.astype(np.float64) + 4.0 * g[..., 3].astype(np.float64)
        d1, d2 = h1[sl].astype(np.float64), h2[sl].astype(np.float64)
        est[sl, 0] = np.concatenate([d1, d2], 1).sum(1)
        est[sl, 1] = np.concatenate([d1 * d1, d2 * d2], 1).sum(1)
        est[sl, 2], est[sl, 3], est[sl, 4] = e.sum(1), (e * e).sum(1), f.sum(1)
        if truth is None or truth.shape[0] == 0 or truth.shape[1] == 0:
            continue
        tv = truth[np.maximum(row[sl], 0)][:, np.maximum(col, 0)]     # [rows, S, 2]
        ok = (row[sl] >= 0)[:, None] & (col >= 0)[None, :] & (tv[..., 0] >= 0) & (tv[..., 1] >= 0)
        t = (tv[..., 0] > 0).astype(np.int64) + (tv[..., 1] > 0)
        cell = 3 * t + called_alt_count(g)
        ez = np.where(ok, e, 0.0)
        acc[sl, 0], acc[sl, 1], acc[sl, 2] = ez.sum(1), (ez * ez).sum(1), (ez * t).sum(1)
        for k in range(9):
            table[sl, k] = (ok & (cell == k)).sum(1)
    return est, acc, table


def site_stats(h1, h2, gt, truth=None, truth_row=None, truth_col=None, device=None,
               chunk_bytes: int = DEFAULT_CHUNK_BYTES):
    """``site_stats_host`` computed by the kernel: (est, acc, table) as host arrays.  h1 / h2 / gt are float32
    device tensors (read in place) or host arrays / tensors (uploaded in chunks of whole site rows of at most
    ``chunk_bytes``, at least one row); ``truth`` is a device or host int8 array.  ValueError when a truth_row
    or truth_col lies outside the truth array (the kernel counts it and treats it as -1)."""
    import torch
    from . import kernels as K
    if not torch.cuda.is_available():
        raise RuntimeError("site_stats needs a HIP device (the host specification is site_stats_host)")
    for name, a in (("h1", h1), ("h2", h2), ("gt", gt)):
        if not (a.dtype == torch.float32 if torch.is_tensor(a) else np.asarray(a).dtype == np.float32):
            raise TypeError(f"{name} must be float32")
    on_device = all(torch.is_tensor(a) and a.is_cuda for a in (h1, h2, gt))
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if on_device:
        dev = h1.device
        h1, h2, gt = h1.contiguous(), h2.contiguous(), gt.contiguous()
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        h1, h2, gt = host(h1), host(h2), host(gt)
    n, S = h1.shape
    if tuple(h2.shape) != (n, S) or tuple(gt.shape) != (n, S, 4):
        raise ValueError("h1 / h2 [n, S] and gt [n, S, 4] do not agree")
    up = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()
    with torch.cuda.device(dev):
        bad = None
        if truth is not None:
            if truth_row is None or truth_col is None:
                raise ValueError("truth needs truth_row and truth_col")
            truth, truth_row, truth_col = up(truth, torch.int8), up(truth_row, torch.int32), up(truth_col, torch.int32)
            if truth_row.numel() != n or truth_col.numel() != S:
                raise ValueError("truth_row must hold n and truth_col S entries")
            bad = torch.zeros(1, device=dev, dtype=torch.int32)
        rows = n if on_device else max(1, min(n, int(chunk_bytes) // (CELL_BYTES * S)))
        parts = []
        for lo in range(0, n, rows):
            hi = min(lo + rows, n)
            if on_device:
                a1, a2, ag = h1, h2, gt
            else:
                a1, a2, ag = (torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(dev) for a in (h1, h2, gt))
            parts.append(K.site_stats(a1, a2, ag, truth, None if truth is None else truth_row[lo:hi], truth_col, bad))
        est = torch.cat([p[0] for p in parts]).cpu().numpy()
        if truth is None:
            return est, None, None
        acc, table = torch.cat([p[1] for p in parts]).cpu().numpy(), torch.cat([p[2] for p in parts]).cpu().numpy()
        if int(bad.item()) != 0:
            raise ValueError(f"{int(bad.item())} truth_row / truth_col entries lie outside the truth array")
    return est, acc, table


def _ratio(num, den):
    """num / den clipped to [0, 1]; 0 where the denominator is not positive."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, np.clip(num / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)


def estimates(est, n_samples: int):
    """(af, r2, dr2) float64 [n] from ``est`` [n, 5] over ``n_samples`` samples:
    af  = sum(h1 + h2) / 2S, the estimated ALT allele frequency;
    r2  = (sum(h1^2 + h2^2) / 2S - af^2) / (af (1 - af)), the Minimac-style ratio of the haplotype-dosage
          variance to its binomial expectation;
    dr2 = (sum e^2 - (sum e)^2 / S) / (sum f - (sum e)^2 / S), the Beagle-style dosage r2 from the genotype
          probabilities.  Both clipped to [0, 1], and 0 where the denominator is not positive."""
    est = np.asarray(est, np.float64)
    S = float(n_samples)
    af = est[:, 0] / (2 * S)
    r2 = _ratio(est[:, 1] / (2 * S) - af * af, af * (1 - af))
    m = est[:, 2] * est[:, 2] / S
    dr2 = _ratio(est[:, 3] - m, est[:, 4] - m)
    return af, r2, dr2


def _truth_moments(table):
    """(n, sum t, sum t^2) of the true ALT counts from the 3 x 3 tables [..., 9], float64."""
    t = np.asarray(table, np.float64)
    one, two = t[..., 3:6].sum(-1), t[..., 6:9].sum(-1)
    return t.sum(-1), one + 2 * two, one + 4 * two


def _accuracy(acc, table):
    acc = np.asarray(acc, np.float64)
    tab = np.asarray(table, np.float64)
    n, st, stt = _truth_moments(tab)
    se, see, set_ = acc[..., 0], acc[..., 1], acc[..., 2]
    cov, ve, vt = n * set_ - se * st, n * see - se * se, n * stt - st * st
    with np.errstate(divide="ignore", invalid="ignore"):
        good = (ve > 0) & (vt > 0)
        r2 = np.where(good, cov * cov / np.where(good, ve * vt, 1.0), np.nan)
        conc = np.where(n > 0, (tab[..., 0] + tab[..., 4] + tab[..., 8]) / np.where(n > 0, n, 1.0), np.nan)
        nonref = tab[..., 3:9].sum(-1)
        nrc = np.where(nonref > 0, (tab[..., 4] + tab[..., 8]) / np.where(nonref > 0, nonref, 1.0), np.nan)
    return n, r2, conc, nrc


def accuracy(acc, table):
    """Per site, from ``acc`` [n, 3] and ``table`` [n, 9]: dict of ``n`` (genotypes compared, int64),
    ``r2`` (squared Pearson correlation of the dosage with the true ALT count, from the sums; NaN where either
    variance is 0), ``concordance`` (called = true genotype class, trace / n) and ``nonref_concordance``
    (the matches with t = c >= 1 over the entries with t >= 1); NaN where nothing was compared."""
    n, r2, conc, nrc = _accuracy(acc, table)
    return dict(n=n.astype(np.int64), r2=r2, concordance=conc, nonref_concordance=nrc)


def aggregate(acc, table, maf, edges=DEFAULT_MAF_EDGES):
    """One row (dict with the keys ``TSV_COLUMNS``) per MAF bin and a last row ``ALL`` over every site given.
    Bins are [edges[i], edges[i + 1]), the last one closed.  ``sites`` / ``genotypes``: the sites of the bin
    and the genotypes compared at them; ``mean_r2``: the mean per-site r2 over the sites where it is defined;
    ``pooled_r2`` / ``concordance`` / ``nonref_concordance``: from the sums and tables added over the bin."""
    acc, table = np.asarray(acc, np.float64).reshape(-1, 3), np.asarray(table, np.int64).reshape(-1, 9)
    maf, edges = np.asarray(maf, np.float64).reshape(-1), np.asarray(edges, np.float64)
    if edges.ndim != 1 or edges.size < 2 or not (np.diff(edges) > 0).all():
        raise ValueError("MAF bin edges must be increasing, at least two")
    if maf.shape[0] != acc.shape[0] or table.shape[0] != acc.shape[0]:
        raise ValueError("acc, table and maf must describe the same sites")
    b = np.searchsorted(edges, maf, side="right") - 1
    b = np.where(maf == edges[-1], edges.size - 2, b)              # the last bin is closed
    site_r2 = _accuracy(acc, table)[1]

    def row(label, sel):
        n, r2, conc, nrc = _accuracy(acc[sel].sum(0), table[sel].sum(0))
        defined = site_r2[sel][~np.isnan(site_r2[sel])]
        return dict(maf_bin=label, sites=int(sel.sum()), genotypes=int(n),
                    mean_r2=float(defined.mean()) if defined.size else float("nan"), pooled_r2=float(r2),
                    concordance=float(conc), nonref_concordance=float(nrc))

    rows = []
    for i in range(edges.size - 1):
        close = "]" if i == edges.size - 2 else ")"
        rows.append(row(f"[{edges[i]:g},{edges[i + 1]:g}{close}", b == i))
    rows.append(row("ALL", np.ones(maf.shape[0], bool)))
    return rows


def accuracy_tsv(rows) -> str:
    """The text of accuracy.tsv: a header and one line per ``aggregate`` row, floats '%.6f' (NaN as ``nan``)."""
    out = ["\t".join(TSV_COLUMNS)]
    for r in rows:
        out.append("\t".join([r["maf_bin"], str(r["sites"]), str(r["genotypes"])] +
                             ["%.6f" % r[k] for k in TSV_COLUMNS[3:]]))
    return "\n".join(out) + "\n"


def truth_maps(truth, ori_pos, sample_names=None, n_samples=None):
    """(truth_row int32 [n], truth_col int32 [S]) for a truth ``VcfGenotypes`` (anything with ``pos`` and
    ``samples``): the truth record of each position of ``ori_pos`` (the first occurrence of a duplicated
    position, -1 when the file does not hold it) and the truth column of each of the S imputed samples — by name
    when ``sample_names`` is given and the truth file holds every one of them, else by column order, which needs
    S (``len(sample_names)`` or ``n_samples``) to equal the truth file's sample count (ValueError if not)."""
    first = {}
    for i, p in enumerate(np.asarray(truth.pos).tolist()):
        first.setdefault(int(p), i)
    row = np.asarray([first.get(int(p), -1) for p in np.asarray(ori_pos).tolist()], np.int32).reshape(-1)
    names = list(truth.samples)
    if sample_names is not None:
        col_of = {}
        for i, s in enumerate(names):
            col_of.setdefault(s, i)
        if all(s in col_of for s in sample_names):
            return row, np.asarray([col_of[s] for s in sample_names], np.int32).reshape(-1)
        n_samples = len(sample_names)
    if n_samples is None:
        raise ValueError("truth_maps needs sample_names or n_samples")
    if int(n_samples) != len(names):
        raise ValueError(f"the truth file holds {len(names)} samples, the imputed arrays {int(n_samples)}: "
                         "columns can be matched by order only when the counts agree")
    return row, np.arange(int(n_samples), dtype=np.int32)


def info_strings(af, r2, dr2, imputed=None):
    """The INFO column of every site: ``AF=%.4f;DR2=%.3f;R2=%.3f;IMP``.  ``imputed`` (bool per site, with
    ``--vcf_sites all``): ``IMP`` where true and ``TYPED`` where false; None: every site ``IMP``."""
    out = ["AF=%.4f;DR2=%.3f;R2=%.3f;IMP" % (a, d, r) for a, r, d in zip(np.asarray(af).tolist(),
                                                                        np.asarray(r2).tolist(),
                                                                        np.asarray(dr2).tolist())]
    if imputed is None:
        return out
    imputed = np.asarray(imputed).astype(bool).reshape(-1)
    if imputed.shape[0] != len(out):
        raise ValueError("imputed must hold one flag per site")
    return [s if f else s[:-3] + "TYPED" for s, f in zip(out, imputed.tolist())]


def parse_maf_bins(text):
    """``--maf_bins a,b,c,...`` as a tuple of floats (None: the default edges)."""
    if not text:
        return DEFAULT_MAF_EDGES
    return tuple(float(v) for v in str(text).split(","))
