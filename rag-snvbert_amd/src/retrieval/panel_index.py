"""HBM-resident panel index of one window and its exact kNN search.

Reference behaviour replaced (src/dataset/embedding_rag_dataset.py):
  * JIT index build (:334-377): masked panel tokens -> fp32 embeddings [N, 1030, D]
    (15.8 GB at N = 10k, 1.58 TB at N = 1M).  Here: allele codes u8 [N, n_sites_pad]
    (1.03 GB at N = 1M), independent of the model weights and of the mask, so it
    never goes stale and is built once per window.
  * distance + top-k (:390-402): torch.cdist + topk(largest=False).  Here:
    LUT -> int8 MFMA scan -> exact (distance, index) top-k.

Two layouts of the same 0/1 alleles: u8 codes, one byte per site (the default),
and ``packed`` bits u8 [N, n_sites_pad / 8], site s of a row = bit s & 7 of byte s >> 3
(``np.packbits(bitorder="little")``), padding sites 0 — an eighth of the HBM, of the upload and of
the bytes the scan streams.  Search results are bit for bit the same in both.
"""

from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import kernels as K


def pad_sites(n_sites: int) -> int:
    """Index row length: a multiple of 256 B so the scan's 16-row LDS swizzle stays inside a row."""
    return max(256, ((n_sites + 255) // 256) * 256)


class PanelIndex:
    def __init__(self, codes: torch.Tensor, n_sites: int, ref_af: torch.Tensor, ref_offset: int = 0,
                 n_total: Optional[int] = None, packed: bool = False):
        """``packed``: ``codes`` is the bit-packed panel, u8 [n_ref, ld / 8]."""
        if codes.dtype != torch.uint8 or codes.dim() != 2:
            raise ValueError("codes must be uint8 [n_ref, ld]" if not packed else "bits must be uint8 [n_ref, ld / 8]")
        self.packed = bool(packed)
        self.bits = codes if self.packed else None
        self._codes = None if self.packed else codes
        self.n_ref = codes.shape[0]
        self.ld = codes.shape[1] * (8 if self.packed else 1)      # sites per row, padding included
        self.n_sites = int(n_sites)
        self.n_sites_pad = pad_sites(n_sites)
        if self.ld < self.n_sites_pad:
            raise ValueError("codes row shorter than padded window")
        self.ref_af = ref_af            # f32 [L] padded AF of the window (ref_af_windows[w])
        self.ref_offset = int(ref_offset)
        self.n_total = int(n_total if n_total is not None else self.n_ref + ref_offset)

    @property
    def codes(self) -> torch.Tensor:
        if self.packed:
            raise AttributeError("a packed PanelIndex holds bits, not u8 codes: gather the rows you need with "
                                 "rows(idx) (kernels.panel_unpack_rows) — nothing unpacks the whole panel")
        return self._codes

    @property
    def data(self) -> torch.Tensor:
        """The device tensor of the index: ``bits`` when packed, else ``codes``."""
        return self.bits if self.packed else self._codes

    @property
    def device(self) -> torch.device:
        return self.data.device

    @classmethod
    def from_alleles(cls, alleles: np.ndarray, ref_af: np.ndarray, device, ref_offset: int = 0,
                     n_total: Optional[int] = None, packed: bool = False) -> "PanelIndex":
        """alleles: int [n_ref, n_sites] in {0, 1} (the panel's GT of this window).  ``packed``:
        the rows are bit-packed on the host and the bits uploaded (an eighth of the copy)."""
        a = np.asarray(alleles)
        if a.size and (a.min() < 0 or a.max() > 1):
            raise ValueError("panel index supports biallelic 0/1 genotypes (got values outside {0,1}); "
                             "binarise multi-allelic/missing calls first")
        n_ref, n_sites = a.shape
        ld = pad_sites(n_sites)
        codes = np.zeros((n_ref, ld), np.uint8)
        codes[:, :n_sites] = a
        if packed:
            bits = np.packbits(codes, axis=1, bitorder="little")
            return cls(torch.from_numpy(bits).to(device), n_sites,
                       torch.as_tensor(np.asarray(ref_af, np.float32), device=device), ref_offset, n_total,
                       packed=True)
        return cls(torch.from_numpy(codes).to(device), n_sites,
                   torch.as_tensor(np.asarray(ref_af, np.float32), device=device), ref_offset, n_total)

    @classmethod
    def from_bit_rows(cls, bits: torch.Tensor, site_idx, ref_af, packed: bool = False, ref_offset: int = 0,
                      n_total: Optional[int] = None, n_src_sites: Optional[int] = None) -> "PanelIndex":
        """The index of the window whose sites are ``site_idx`` (any order, not contiguous; -1 = a zero
        site) of the haplotype bit rows ``bits`` u8 [n_ref, ld_bits] on the device (``read_vcf``'s
        ``alt_bits``, or a contiguous row range of them): ``snvrag_panel_gather_bits``, either layout.
        Equal to ``from_alleles`` of the same columns."""
        site_idx = torch.as_tensor(np.ascontiguousarray(site_idx, np.int32)).to(bits.device)
        n_sites = site_idx.numel()
        n_src = 8 * bits.shape[1] if n_src_sites is None else int(n_src_sites)
        data = K.panel_gather_bits(bits.contiguous(), n_src, site_idx, pad_sites(n_sites), packed)
        return cls(data, n_sites, torch.as_tensor(np.asarray(ref_af, np.float32), device=bits.device), ref_offset,
                   n_total, packed=packed)

    @classmethod
    def synthetic(cls, n_ref: int, n_sites: int, site_af: torch.Tensor, ref_af: torch.Tensor,
                  seed: int, packed: bool = False) -> "PanelIndex":
        if packed:    # generated straight as bits: the u8 form never exists
            return cls(K.panel_synth_bits(n_ref, n_sites, site_af.float().contiguous(), seed), n_sites, ref_af,
                       packed=True)
        codes = K.panel_synth(n_ref, n_sites, site_af.float().contiguous(), seed)
        return cls(codes, n_sites, ref_af)

    def pack(self) -> "PanelIndex":
        """The packed twin of a u8 index, packed on the device (a packed index returns itself)."""
        if self.packed:
            return self
        return PanelIndex(K.panel_pack_bits(self._codes), self.n_sites, self.ref_af, self.ref_offset, self.n_total,
                          packed=True)

    @property
    def nbytes(self) -> int:
        return self.data.numel()

    # --------------------------------------------------------------- consumers --
    def rows(self, idx: torch.Tensor) -> torch.Tensor:
        """u8 [len(idx), ld] allele codes of the local rows ``idx`` (int64), either layout.  A
        packed index gives zero rows for indices outside [0, n_ref)."""
        if self.packed:
            return K.panel_unpack_rows(self.bits, idx.long().contiguous())
        return self._codes[idx]

    def rag_mean(self, idx: torch.Tensor, W, pe, Ar, L: int, dtype, out=None, counts=None) -> torch.Tensor:
        """``kernels.rag_mean`` over this index's rows (read in place in either layout)."""
        return K.rag_mean(idx, self.data, self.n_sites, W, pe, Ar, L, dtype, out=out, counts=counts,
                          bits=self.packed)

    def neighbor_counts(self, idx: torch.Tensor) -> torch.Tensor:
        """``kernels.neighbor_counts`` of the global neighbours ``idx`` that this index owns."""
        return K.neighbor_counts(idx, self.data, self.ref_offset, bits=self.packed)

    # ------------------------------------------------------------------ search --
    def lut(self, tok_q: torch.Tensor, W: torch.Tensor, site_mask: torch.Tensor, limbs: int = 2,
            Aq: Optional[torch.Tensor] = None, aq_period: int = 0, Ar: Optional[torch.Tensor] = None,
            Wp: Optional[torch.Tensor] = None):
        return K.knn_lut(tok_q.long().contiguous(), W, site_mask, self.n_sites, self.n_sites_pad, limbs,
                         Aq, aq_period, Ar, Wp=Wp)

    SAMPLE_MIN = 1 << 17       # panels at least this large get a threshold pre-pass

    def scan_keys(self, lut: torch.Tensor, nq: int, limbs: int, k: int, presample: Optional[bool] = None) -> torch.Tensor:
        """Exact local top-k keys [nq, k] (uint64 in int64 storage) with global indices.

        Large panels first scan a 1/64 prefix of the panel: its k-th best distance is an
        upper bound on the panel's, so the full scan can start from it (strictly above it
        nothing can enter the top-k) and keeps far fewer candidates; the result is the
        same exact top-k.  (1/64 measured best for the whole search on the bench panel:
        1M x 1024, 96 queries: 0.319 ms vs 0.3315 ms at 1/128 and 0.337 ms at 1/32 — the
        full scan's candidate compaction is its compute-side cost, profiles/r3_knn_probe.txt.)"""
        n_ref = self.n_ref
        scan = K.knn_scan_bits if self.packed else K.knn_scan
        data = self.data
        if presample is None:
            presample = n_ref >= self.SAMPLE_MIN
        th = None
        if presample:
            div = int(os.environ.get("SNVRAG_SAMPLE_DIV", "64"))
            rpp = int(os.environ.get("SNVRAG_SAMPLE_RPP", "64"))
            m = max(16 * k, ((n_ref // div) + 15) // 16 * 16)
            sample = scan(data[:m], self.n_sites_pad, lut, nq, limbs, k, self.ref_offset,
                          n_parts=max(1, min(256, m // rpp)))
            th = K.knn_threshold(K.topk_merge(sample, k), k)
        parts = scan(data, self.n_sites_pad, lut, nq, limbs, k, self.ref_offset, th_init=th)
        return K.topk_merge(parts, k)

    def search(self, tok_q: torch.Tensor, W: torch.Tensor, site_mask: torch.Tensor, k: int, limbs: int = 2,
               Aq: Optional[torch.Tensor] = None, aq_period: int = 0, Ar: Optional[torch.Tensor] = None,
               return_keys: bool = False, Wp: Optional[torch.Tensor] = None):
        """idx int64 [nq, k] (-1 pads when the panel has < k haplotypes), dist f32 [nq, k] (squared L2).
        ``Wp`` / ``Ar``: the panel side's token table / AF embedding when they differ from the
        queries' (a cached, stale panel embedding: snvrag_knn_lut_panel)."""
        nq = tok_q.shape[0]
        lut, exps, consts = self.lut(tok_q, W, site_mask, limbs, Aq, aq_period, Ar, Wp=Wp)
        keys = self.scan_keys(lut, nq, limbs, k)
        idx, dist = K.knn_decode(keys, exps, consts)
        if return_keys:
            return idx, dist, keys, lut, exps
        return idx, dist
