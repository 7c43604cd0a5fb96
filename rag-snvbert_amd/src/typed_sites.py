"""Typed sites in the imputed VCF (opt-in: ``--vcf_sites all``): the observed genotypes of the target written
over the model's output in the site-major result arrays, so that the writers emit one record per panel site.

The result arrays h1 / h2 [n, S] and gt [n, S, 4] hold a row for every panel site; at a site the target was
genotyped at, that row is the model's output at an unmasked token.  The overlay (csrc/typed.hip
``snvrag_typed_overlay``) replaces it with the target's call, read from the target's bit rows (``alt_bits`` /
``miss_bits`` u8 [2 S_target, ld_bits]: haplotype h of sample c in row 2 c + h, record r at bit r & 7 of byte
r >> 3 — the ``VcfGenotypes`` layout).  For the site row i with r = site_row[i] in [0, n_target) and the column s
with c = col[s] in [0, S_target):

  a1, m1 = ALT and missing bit r of row 2 c;  a2, m2 = those of row 2 c + 1;
  m1 | m2   the cell keeps every byte it had (the model's output) and missing[i] counts it;
  else      h1 = a1, h2 = a2 (0.0 / 1.0), gt = one-hot at 2 a1 + a2 (0|0, 0|1, 1|0, 1|1: ``GT_MAP``'s order).

Every other cell is untouched.  No float arithmetic: the result is exact.  ``typed_overlay_host`` is the
specification in numpy; ``typed_overlay`` runs the kernel, on device tensors in place or on host arrays whose
typed rows are uploaded in chunks; ``target_bit_rows`` / ``target_maps`` give the bit rows and the maps of an infer
dataset.
"""

from __future__ import annotations

import numpy as np

DEFAULT_CHUNK_BYTES = 256 << 20
CELL_BYTES = 24                     # h1, h2 and the four gt values of one site and sample


def _f32(a, name, shape=None):
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise TypeError(f"{name} must be a float32 numpy array (it is changed in place)")
    if shape is not None and a.shape != shape:
        raise ValueError("h1 / h2 [n, S] and gt [n, S, 4] do not agree")
    return a


def _index(a, count, bound, name):
    """An index array as int64 with everything outside [0, bound) set to -1."""
    a = np.asarray(a).astype(np.int64).reshape(-1)
    if a.shape[0] != count:
        raise ValueError(f"{name} must hold {count} entries, not {a.shape[0]}")
    return np.where((a >= 0) & (a < bound), a, -1)


def typed_overlay_host(h1, h2, gt, alt_bits, miss_bits, n_target, site_row, col):
    """The specification of ``snvrag_typed_overlay`` (module docstring) in numpy, without a GPU call.  h1 / h2
    float32 [n, S] and gt float32 [n, S, 4] are changed in place; returns ``missing`` int32 [n]."""
    h1 = _f32(h1, "h1")
    n, S = h1.shape
    h2, gt = _f32(h2, "h2", (n, S)), _f32(gt, "gt", (n, S, 4))
    alt_bits, miss_bits = np.asarray(alt_bits), np.asarray(miss_bits)
    if alt_bits.dtype != np.uint8 or miss_bits.dtype != np.uint8 or alt_bits.ndim != 2 or \
            alt_bits.shape != miss_bits.shape or alt_bits.shape[0] % 2 or alt_bits.shape[0] == 0:
        raise ValueError("alt_bits / miss_bits must be uint8 [2 S_target, ld_bits]")
    n_target = int(n_target)
    if n_target < 0 or 8 * alt_bits.shape[1] < n_target:
        raise ValueError("the bit rows do not hold n_target records")
    row = _index(site_row, n, n_target, "site_row")
    cl = _index(col, S, alt_bits.shape[0] // 2, "col")
    missing = np.zeros(n, np.int32)
    I, J = np.flatnonzero(row >= 0), np.flatnonzero(cl >= 0)
    if I.size == 0 or J.size == 0:
        return missing
    r, c = row[I], cl[J]
    bit = lambda bits, h: ((bits[np.ix_(2 * c + h, r >> 3)] >> (r & 7)[None, :].astype(np.uint8)) & 1).T.astype(bool)
    a1, a2 = bit(alt_bits, 0), bit(alt_bits, 1)                       # [typed rows, mapped columns]
    miss = bit(miss_bits, 0) | bit(miss_bits, 1)
    missing[I] = miss.sum(1)
    ii, jj = np.broadcast_to(I[:, None], miss.shape)[~miss], np.broadcast_to(J[None, :], miss.shape)[~miss]
    b1, b2 = a1[~miss], a2[~miss]
    h1[ii, jj] = b1
    h2[ii, jj] = b2
    onehot = np.zeros((ii.size, 4), np.float32)
    onehot[np.arange(ii.size), 2 * b1.astype(np.int64) + b2] = 1.0
    gt[ii, jj] = onehot
    return missing


def typed_overlay(h1, h2, gt, target, site_row, col=None, device=None, chunk_bytes: int = DEFAULT_CHUNK_BYTES):
    """``typed_overlay_host`` computed by the kernel; returns ``missing`` as a host int32 [n].  ``target`` is
    ``(alt_bits, miss_bits, n_target, S_target)`` as ``target_bit_rows`` returns it (device tensors or host
    arrays).  h1 / h2 / gt are float32 device tensors, overlaid in place, or host numpy arrays: then only the rows
    with a valid ``site_row`` are gathered, uploaded in chunks of whole site rows of at most ``chunk_bytes`` (at
    least one row), overlaid, downloaded and scattered back in place.  ``col`` None is the identity."""
    import torch
    from . import kernels as K
    if not torch.cuda.is_available():
        raise RuntimeError("typed_overlay needs a HIP device (the host specification is typed_overlay_host)")
    alt_bits, miss_bits, n_target, S_target = target
    n_target, S_target = int(n_target), int(S_target)
    on_device = all(torch.is_tensor(a) and a.is_cuda for a in (h1, h2, gt))
    if on_device:
        dev = h1.device
        if not (h1.is_contiguous() and h2.is_contiguous() and gt.is_contiguous()):
            raise ValueError("device result arrays must be contiguous (they are overlaid in place)")
        if not h1.dtype == h2.dtype == gt.dtype == torch.float32:
            raise TypeError("h1 / h2 / gt must be float32")
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        h1 = _f32(h1, "h1")
    n, S = h1.shape
    if not on_device:
        h2, gt = _f32(h2, "h2", (n, S)), _f32(gt, "gt", (n, S, 4))
    elif tuple(h2.shape) != (n, S) or tuple(gt.shape) != (n, S, 4):
        raise ValueError("h1 / h2 [n, S] and gt [n, S, 4] do not agree")
    row = _index(site_row, n, n_target, "site_row").astype(np.int32)
    cl = np.arange(S) if col is None else col
    cl = _index(cl, S, S_target, "col").astype(np.int32)
    up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
    with torch.cuda.device(dev):
        alt_bits, miss_bits, d_col = up(alt_bits), up(miss_bits), up(cl)
        if on_device:
            return K.typed_overlay(h1, h2, gt, alt_bits, miss_bits, n_target, up(row), d_col).cpu().numpy()
        missing = np.zeros(n, np.int32)
        typed = np.flatnonzero(row >= 0)
        rows = max(1, int(chunk_bytes) // (CELL_BYTES * S))
        for lo in range(0, typed.size, rows):
            sel = typed[lo:lo + rows]
            a1, a2, ag = (up(a[sel]) for a in (h1, h2, gt))
            missing[sel] = K.typed_overlay(a1, a2, ag, alt_bits, miss_bits, n_target, up(row[sel]), d_col).cpu().numpy()
            h1[sel], h2[sel], gt[sel] = a1.cpu().numpy(), a2.cpu().numpy(), ag.cpu().numpy()
    return missing


def pack_bit_rows(vcf):
    """Genotypes [n_target, S, 2] (> 0: ALT, < 0: missing) as host bit rows ``(alt_bits, miss_bits)`` u8
    [2 S, ld_bits] in the ``VcfGenotypes`` layout, ld_bits a multiple of 8 (at least 8); an ALT bit is 0 where the
    call is missing (numpy.packbits, little-endian)."""
    vcf = np.asarray(vcf)
    if vcf.ndim != 3 or vcf.shape[2] != 2:
        raise ValueError(f"genotypes must be [sites, samples, 2], got {vcf.shape}")
    rows, S = vcf.shape[:2]
    nb = (rows + 7) // 8
    ld = max(8, (nb + 7) // 8 * 8)
    alt, miss = np.zeros((2 * S, ld), np.uint8), np.zeros((2 * S, ld), np.uint8)
    step = max(1, (64 << 20) // max(1, 2 * rows))                # ~64 MiB of genotypes at a time
    for s0 in range(0, S if rows else 0, step):
        g = np.ascontiguousarray(vcf[:, s0:s0 + step].transpose(1, 2, 0)).reshape(-1, rows)
        alt[2 * s0:2 * s0 + g.shape[0], :nb] = np.packbits(g > 0, axis=1, bitorder="little")
        miss[2 * s0:2 * s0 + g.shape[0], :nb] = np.packbits(g < 0, axis=1, bitorder="little")
    return alt, miss


def target_bit_rows(ds, device=None):
    """``(alt_bits, miss_bits, n_target, S)`` of the target of an infer dataset: the device bit rows of
    ``ds.vcf_genotypes`` when the target came from a VCF (and still holds the file's records), else ``ds.vcf``
    ([n_target, S, 2]) packed by ``pack_bit_rows`` — on ``device``, or as host arrays without one."""
    vcf = ds.vcf
    n_target, S = int(vcf.shape[0]), int(vcf.shape[1])
    vg = getattr(ds, "vcf_genotypes", None)
    if vg is not None and vg.n_sites == n_target and tuple(vg.alt_bits.shape)[0] == 2 * S and \
            8 * tuple(vg.alt_bits.shape)[1] >= n_target:
        return vg.alt_bits, vg.miss_bits, n_target, S
    alt, miss = pack_bit_rows(vcf)
    if device is None:
        return alt, miss, n_target, S
    import torch
    return torch.from_numpy(alt).to(device), torch.from_numpy(miss).to(device), n_target, S


def target_maps(ds):
    """``(site_row int32 [n], col int32 [S])`` of an infer dataset: the target record the model's input of each
    row of ``ds.ori_pos`` was built from (``ds._vcf_row``: the last occurrence of a duplicated target position,
    -1 where the target lacks the site) and the identity over the samples."""
    return np.asarray(ds._vcf_row).astype(np.int32), np.arange(int(ds.vcf.shape[1]), dtype=np.int32)
