"""Device-resident featurisation: batches built on the GPU (opt-in, ``--device_features``).

The host path builds every batch one ``__getitem__`` at a time (``InferDataset`` /
``EmbeddingRAGInferDataset`` / ``EmbeddingRAGDataset``), stacks the items
(``embedding_rag_collate_fn``) and copies ~13 MB of mostly int64 tensors to the device.  Every
input of that work is static — the cohort's genotypes, the frequency table, each window's site
list, normalised positions and mask, each sample's population — so a batch is a gather over them.
``DeviceFeatures`` uploads them once and ``batch(items)`` is one small upload (the row table)
plus one kernel launch (``snvrag_batch_features``, csrc/features.hip).  The kernel does no float
arithmetic, so every tensor is bit for bit what the host path produces.

Layouts (``host_tables``):
  gt_bits        u8  [2 S, ld_bits]   haplotype h of sample s = row 2 s + h over the rows of ``vcf``,
                                      1 bit per site (site r = bit r & 7 of byte r >> 3), ld_bits = ceil(rows / 8)
  win_off        i32 [W + 1]          window w owns entries [win_off[w], win_off[w + 1]) of:
  site_row       i32 [sum n_w]        row in ``vcf`` (-1: absent from the target, allele 0)
  freq_col       i32 [sum n_w]        column of the frequency table
  pos_norm       f32 [sum n_w]        position_normalize -> float32, per window
  win_mask       u8  [W, L]           the padded mask the window's items carry
  freq           f32 [4, P, n_cols]   as the dataset holds it
  pop_of_sample  i32 [S]

Memory (``DeviceFeatures.nbytes`` = ``table_nbytes``):
  2 S ceil(rows / 8)  +  12 sum_w n_w  +  4 (W + 1)  +  W L  +  16 P n_cols  +  4 S      bytes.

Not covered: genotype values other than 0/1 (missing = -1: ``ValueError``, those cohorts keep the
host path); a plain ``TrainDataset`` (its masks draw from the global numpy RNG per item: nothing to
reproduce); H5 files need h5py.  A dataset read from a VCF (``vcf_genotypes``, vcf_reader.py) hands its
device bit rows over as ``gt_bits``: nothing is packed or uploaded again.  Masks stay the host's numpy stream (``af_guided_mask``), so they
match the reference's seeds.
"""

from __future__ import annotations

from typing import Dict, Iterable, List, Sequence

import numpy as np
import torch

from .dataset import GLOBAL, InferDataset, TrainDataset
from .utils import MAX_SEQ_LEN, af_guided_mask, position_normalize, sequence_padding

FLOAT_KEYS = ("pos", "af", "af_p", "ref", "het", "hom")
LABEL_KEYS = ("hap_1_label", "hap_2_label", "gt_label")
VAL_SEED = 2024          # embedding_rag_dataset.py:486-555: seed = current_epoch for "train", else 2024


def _is_infer(ds) -> bool:
    return isinstance(ds, InferDataset)


def window_sites(ds, w: int):
    """(site_row, freq_col, pos_norm) of window ``w``: what ``__getitem__`` gathers with, per site."""
    if _is_infer(ds):
        start, end = ds.window_bounds(w)
        rows = ds._vcf_row[start:end]
        cols = ds._freq_col[start:end]
        pos = ds.ori_pos[start:end]
    else:
        sl = ds._window_slice(w)
        rows = np.arange(sl.start, sl.stop)
        valid = getattr(ds, "window_valid_indices", {}).get(w)
        if valid is not None:
            rows = rows[valid]
        cols = ds._freq_col[rows]
        pos = ds.pos[rows]
    with np.errstate(invalid="ignore", divide="ignore"):      # a one-site window: 0 / 0 = NaN, as the host path
        pn = position_normalize(pos) if len(pos) else np.zeros(0)
    return np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.asarray(pn, np.float64).astype(np.float32)


def mask_key(ds):
    """What the items' masks depend on: (seed, level, mask_version); None for the static infer masks."""
    if _is_infer(ds):
        return None
    seed = ds.current_epoch if ds.name == "train" else VAL_SEED
    return int(seed), int(ds._level), int(getattr(ds, "mask_version", 0))


def window_masks(ds, L: int = MAX_SEQ_LEN) -> np.ndarray:
    """u8 [W, L]: the padded mask ``__getitem__`` gives every item of each window, now."""
    W = ds.window_count
    out = np.zeros((W, L), np.uint8)
    for w in range(W):
        if _is_infer(ds):
            if hasattr(ds, "infer_masks"):
                if len(ds.infer_masks) != W:
                    raise ValueError("the infer dataset has no per-window masks (built without its panel index)")
                m = ds.infer_masks[w]
            else:
                start, end = ds.window_bounds(w)
                m = sequence_padding((ds._vcf_row[start:end] < 0).astype(np.int64), "int", L)
        else:
            n = ds.window_actual_lens[w]
            seed, level, _ = mask_key(ds)
            m = sequence_padding(af_guided_mask(ds.ref_af_windows[w][1:1 + n], level, seed, w), "int", L)
        out[w] = np.asarray(m)[:L] != 0
    return out


def pack_genotypes(vcf: np.ndarray) -> np.ndarray:
    """vcf [rows, S, 2] of 0/1 -> u8 [2 S, ceil(rows / 8)] bit rows (numpy.packbits, little-endian)."""
    vcf = np.asarray(vcf)
    if vcf.ndim != 3 or vcf.shape[2] != 2:
        raise ValueError(f"genotypes must be [sites, samples, 2], got {vcf.shape}")
    rows, S = vcf.shape[0], vcf.shape[1]
    bits = np.zeros((2 * S, max(1, (rows + 7) // 8)), np.uint8)
    step = max(1, (64 << 20) // max(1, 2 * rows))                # ~64 MiB of genotypes at a time
    for s0 in range(0, S, step):
        g = vcf[:, s0:s0 + step]
        if ((g != 0) & (g != 1)).any():
            raise ValueError(MISSING_CALLS)
        if rows:
            g = np.ascontiguousarray(g.transpose(1, 2, 0)).reshape(-1, rows).astype(np.uint8)
            bits[2 * s0:2 * s0 + g.shape[0], :(rows + 7) // 8] = np.packbits(g, axis=1, bitorder="little")
    return bits


MISSING_CALLS = ("device features need 0/1 genotypes; this cohort holds other values (missing = -1?) "
                 "and keeps the host path")


def vcf_gt_bits(ds):
    """The device bit rows of a dataset read from a VCF (``ds.vcf_genotypes.alt_bits``: already the
    ``gt_bits`` layout), or None.  Missing calls: the ``ValueError`` of ``pack_genotypes``."""
    vg = getattr(ds, "vcf_genotypes", None)
    if vg is None:
        return None
    if vg.any_missing:
        raise ValueError(MISSING_CALLS)
    n_rows, S = np.asarray(ds.vcf).shape[:2]
    if vg.n_sites != n_rows or vg.alt_bits.shape != (2 * S, max(1, (n_rows + 7) // 8)):
        return None                                            # the dataset no longer holds the file's rows
    return vg.alt_bits


def host_tables(ds, L: int = MAX_SEQ_LEN, gt_bits=None) -> Dict[str, np.ndarray]:
    """The static tables of ``ds`` on the host (module docstring), validated: every index the kernel
    gathers with is in range.  ``gt_bits``: bit rows that exist already (a device tensor), taken as they are."""
    if not _is_infer(ds):
        if not isinstance(ds, TrainDataset) or not hasattr(ds, "window_actual_lens"):
            raise ValueError("device features need an EmbeddingRAGDataset (seeded per-window masks) or an infer "
                             "dataset; a plain TrainDataset masks each item from the global numpy RNG")
        if len(ds.window_actual_lens) != ds.window_count:
            raise ValueError("the dataset was built without its panel (no per-window masks)")
    W = ds.window_count
    parts = [window_sites(ds, w) for w in range(W)]
    counts = np.array([len(p[0]) for p in parts], np.int64)
    if not _is_infer(ds) and (counts != np.asarray(ds.window_actual_lens)).any():
        raise ValueError("window site counts disagree with window_actual_lens")
    if W == 0 or counts.max() + 1 > L:
        raise ValueError(f"a window has {counts.max() if W else 0} sites: more than L - 1 = {L - 1}")
    freq = np.ascontiguousarray(ds.freq, np.float32)
    if freq.ndim != 3 or freq.shape[0] != 4 or freq.shape[1] <= GLOBAL:
        raise ValueError(f"frequency table must be [4, >= {GLOBAL + 1}, n_cols], got {freq.shape}")
    t = dict(gt_bits=pack_genotypes(ds.vcf) if gt_bits is None else gt_bits,
             win_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
             site_row=np.concatenate([p[0] for p in parts]), freq_col=np.concatenate([p[1] for p in parts]),
             pos_norm=np.concatenate([p[2] for p in parts]), win_mask=window_masks(ds, L), freq=freq)
    S = np.asarray(ds.vcf).shape[1]
    t["pop_of_sample"] = np.array([ds.pop_to_idx[p] for p in ds.panel.pop_list[:S]], np.int32)
    if len(t["pop_of_sample"]) != S:
        raise ValueError("fewer population labels than samples")
    n_rows = np.asarray(ds.vcf).shape[0]
    if len(t["site_row"]) and (t["site_row"].max() >= n_rows or t["site_row"].min() < -1):
        raise ValueError("a window site points outside the genotype array")
    if len(t["freq_col"]) and (t["freq_col"].min() < 0 or t["freq_col"].max() >= freq.shape[2]):
        raise ValueError("a window site points outside the frequency table")
    if S and (t["pop_of_sample"].min() < 0 or t["pop_of_sample"].max() >= freq.shape[1]):
        raise ValueError("a sample's population is outside the frequency table")
    return t


def table_nbytes(n_rows: int, n_samples: int, site_counts: Sequence[int], n_pop: int, n_cols: int,
                 L: int = MAX_SEQ_LEN) -> int:
    """The memory formula of the module docstring (and DESIGN.md)."""
    W = len(site_counts)
    return (2 * n_samples * max(1, (n_rows + 7) // 8) + 12 * int(sum(site_counts)) + 4 * (W + 1) + W * L +
            16 * n_pop * n_cols + 4 * n_samples)


class DeviceBatch(dict):
    """A batch dictionary that also carries its row table (int32 [3, B]: sample, window, flags) on the
    device and on the host, for ``kernels.infer_scatter``."""
    rows_dev: torch.Tensor = None
    rows_host: torch.Tensor = None


class DeviceFeatures:
    """The static tables of ``dataset`` on ``device`` and the batch builder over them.

    ``batch(items)`` returns the keys, shapes and dtypes of
    ``embedding_rag_collate_fn([dataset[i] for i in items])`` with every tensor already on the device
    and bit-identical, except:
      * ``window_idx`` stays on the host, as collate gives it (a list of 0-d CPU tensors for the infer
        dataset, a list of ints for the train dataset): retrieval iterates it with ``int()``;
      * ``sample_idx`` / ``start_idx`` / ``end_idx`` (infer) ride in the same small upload as the row table;
      * the ragged ``hap1_nomask`` / ``hap2_nomask`` lists are omitted: nothing downstream reads them.
    ``hap_1`` / ``hap_2`` are the two halves of one [2B, L] buffer (``batch["hap_1"]._base``).

    Masks follow the dataset: the train / validation mask of ``__getitem__``
    (``af_guided_mask(af, level, seed, w)``, seed = ``current_epoch`` for name "train", else 2024) is
    cached per (seed, level) and re-uploaded when ``current_epoch``, the level or ``mask_version``
    changes — checked at every ``batch`` call.
    """

    def __init__(self, dataset, device, L: int = MAX_SEQ_LEN):
        from .. import native as N
        self.dataset, self.device, self.L = dataset, torch.device(device), int(L)
        self.infer = _is_infer(dataset)
        t = host_tables(dataset, self.L, vcf_gt_bits(dataset))
        self._mask_key = mask_key(dataset)
        self._mask_cache = {self._mask_key[:2] if self._mask_key else None: t["win_mask"]}
        self.win_off = t["win_off"].astype(np.int64)
        self.n_samples = int(t["pop_of_sample"].shape[0])
        self.n_items = len(dataset)
        self.dev = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(self.device)
                    for k, v in t.items()}
        v = dataset.vocab
        self.token_ids = (v.sos_index, v.eos_index, v.pad_index, v.mask_index, v.stoi[0], v.stoi[1])
        T = N.FeatureTables()
        for k, d in self.dev.items():
            setattr(T, k, int(d.data_ptr()))
        T.ld_bits, T.n_cols = t["gt_bits"].shape[1], t["freq"].shape[2]
        T.n_samples, T.n_windows = self.n_samples, dataset.window_count
        T.max_window_sites = int(np.diff(t["win_off"]).max())
        T.n_pop, T.global_row = t["freq"].shape[1], GLOBAL
        self.tables = T

    @property
    def nbytes(self) -> int:
        return sum(d.numel() * d.element_size() for d in self.dev.values())

    def refresh_masks(self) -> None:
        """Re-upload the window masks if what they depend on changed (stream-ordered: batches already
        launched keep the masks they were built with)."""
        key = mask_key(self.dataset)
        if key == self._mask_key:
            return
        m = self._mask_cache.get(key[:2])
        if m is None:
            if len(self._mask_cache) >= 4:
                self._mask_cache.pop(next(iter(self._mask_cache)))
            m = self._mask_cache[key[:2]] = window_masks(self.dataset, self.L)
        self.dev["win_mask"].copy_(torch.from_numpy(m).pin_memory(), non_blocking=True)
        self._mask_key = key

    def batch(self, items: Iterable[int]) -> DeviceBatch:
        from .. import kernels as K
        items = np.asarray(list(items), np.int64).reshape(-1)
        B, W = len(items), self.dataset.window_count
        dup = items >= self.n_items
        if self.infer and dup.any():
            raise IndexError("item outside the infer dataset")
        base = np.where(dup, items - self.n_items, items)
        if B and (base.min() < 0 or base.max() >= self.n_items):
            raise IndexError("item outside the dataset")
        sample, win = base // W, base % W
        self.refresh_masks()
        # one pinned buffer, one copy: [sample_idx, start_idx, end_idx] i64 (infer), then the i32 row table
        n64 = 3 * B if self.infer else 0
        buf = torch.empty(n64 + (3 * B + 1) // 2, dtype=torch.int64, pin_memory=True)
        rows_host = buf[n64:].view(torch.int32)[:3 * B]
        rh = rows_host.numpy().reshape(3, B)
        rh[0], rh[1], rh[2] = sample, win, dup
        if self.infer:
            b64 = buf[:n64].numpy().reshape(3, B)
            b64[0] = sample
            b64[1] = win * self.dataset.window_len
            b64[2] = np.minimum(b64[1] + self.dataset.window_len, len(self.dataset.ori_pos))
        dbuf = buf.to(self.device, non_blocking=True)
        rows_dev = dbuf[n64:].view(torch.int32)[:3 * B]
        tokens, mask, floats, labels = K.batch_features(self.tables, rows_dev, rows_host, B, self.L, self.token_ids,
                                                        labels=not self.infer)
        out = DeviceBatch(hap_1=tokens[:B], hap_2=tokens[B:], mask=mask)
        out.rows_dev, out.rows_host = rows_dev, rows_host
        for i, k in enumerate(FLOAT_KEYS):
            out[k] = floats[i]
        if self.infer:
            out["window_idx"] = list(torch.from_numpy(win.copy()).unbind(0))
            for i, k in enumerate(("sample_idx", "start_idx", "end_idx")):
                out[k] = dbuf[i * B:(i + 1) * B].view(B, 1)
        else:
            out["window_idx"] = [int(w) for w in win]
            for i, k in enumerate(LABEL_KEYS):
                out[k] = labels[i]
        return out


class DeviceBatchLoader:
    """What the entry points and the trainer read from a ``DataLoader`` (iteration, ``__len__``,
    ``dataset``, ``sampler``, ``batch_size``) over ``DeviceFeatures.batch`` of consecutive sampler
    chunks.  One batch is kept in flight ahead on the current stream — its upload and launch are
    queued before the consumer gets the previous batch, so the host work of batch i + 1 overlaps the
    device work of batch i; no threads.  The dataset's epoch / level must not change inside one
    iteration (the trainer changes them between epochs)."""

    def __init__(self, dataset, sampler, batch_size: int, device, features: DeviceFeatures = None):
        self.dataset, self.sampler, self.batch_size = dataset, sampler, int(batch_size)
        self.features = features if features is not None else DeviceFeatures(dataset, device)

    def __len__(self) -> int:
        return (len(self.sampler) + self.batch_size - 1) // self.batch_size

    def _chunks(self):
        chunk: List[int] = []
        for item in self.sampler:
            chunk.append(int(item))
            if len(chunk) == self.batch_size:
                yield chunk
                chunk = []
        if chunk:
            yield chunk

    def __iter__(self):
        ahead = None
        for chunk in self._chunks():
            nxt = self.features.batch(chunk)
            if ahead is not None:
                yield ahead
            ahead = nxt
        if ahead is not None:
            yield ahead
