// What the bf16 attention kernels share (inference and training forward in attention.hip,
// training backward in attention_train.hip): tile geometry, the XCD block order, the
// register-staged tile helpers of the generic kernels, the dh = 32 tile images of the LDS-DMA
// ring kernels (t32; ring_wait is in common.h beside dma_x4), and the dropout mask.
#pragma once
#include "common.h"

namespace snvrag {

constexpr int AQ = 64;     // queries per workgroup
constexpr int AK = 64;     // keys per tile

template <int DH>
struct AttnCfg {
  static constexpr int KS = (DH + 31) / 32;        // 32-wide MFMA k-steps over head dim
  static constexpr int DP = KS * 32;               // padded head dim in the K tile
  static constexpr int KROWB = DP * 2;             // bytes per K-tile row
  static constexpr int CPR = DP / 8;               // 16-B chunks per K row
  static constexpr int RPC = 256 / KROWB;          // rows per 256-B bank cycle
  static constexpr int ET = DH / 16;               // 16-wide output d tiles
  static constexpr int VT_LD = AK + 8;             // V^T row stride (bf16), padded
  static constexpr int KBYTES = AK * KROWB;
  static constexpr int VBYTES = DP * VT_LD * 2;
  static constexpr int STAGE = KBYTES + VBYTES;
  static constexpr int NLD = (64 * CPR + 255) / 256;   // register-staged loads per thread per 64-row tile
};

template <int DH>
__device__ __forceinline__ int k_off(int key, int chunk) {
  using C = AttnCfg<DH>;
  return key * C::KROWB + ((chunk ^ ((key / C::RPC) % C::CPR)) << 4);
}

// XCD-aware block order (consecutive tiles of one (sequence, head) share an XCD's L2)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int qq = nwg / 8, rr = nwg % 8, xcd = orig % 8;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + orig / 8;
}

// ---- register-staged 64-row tiles of the generic (any head dim) kernels, 256 threads ----
// load a 64-row x DH bf16 tile (rows >= L are zero) into registers
template <int DH>
__device__ __forceinline__ void tile_load(u32x4 (&r)[AttnCfg<DH>::NLD], const bf16* __restrict__ P, long ld, int t0,
                                          int L, int tid) {
  using C = AttnCfg<DH>;
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int id = tid + 256 * i;
    const int row = id / C::CPR, c = id % C::CPR;
    const int rr = t0 + row, d0 = 8 * c;
    if (id < 64 * C::CPR && rr < L && d0 < DH) r[i] = *reinterpret_cast<const u32x4*>(P + (long)rr * ld + d0);
    else r[i] = u32x4{0u, 0u, 0u, 0u};
  }
}
// row-major swizzled store (A operand rows: MFMA reads row li, chunk 4 ks + lg)
template <int DH>
__device__ __forceinline__ void tile_store_rows(char* dst, const u32x4 (&r)[AttnCfg<DH>::NLD], int tid) {
  using C = AttnCfg<DH>;
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int id = tid + 256 * i;
    if (id < 64 * C::CPR) *reinterpret_cast<u32x4*>(dst + k_off<DH>(id / C::CPR, id % C::CPR)) = r[i];
  }
}
// transposed store [d][row] with row stride VT_LD (A operand of the P / dS products)
template <int DH>
__device__ __forceinline__ void tile_store_t(char* dst, const u32x4 (&r)[AttnCfg<DH>::NLD], int tid) {
  using C = AttnCfg<DH>;
  bf16* t = reinterpret_cast<bf16*>(dst);
#pragma unroll
  for (int i = 0; i < C::NLD; ++i) {
    const int id = tid + 256 * i;
    if (id < 64 * C::CPR) {
      const int row = id / C::CPR, c = id % C::CPR;
      const bf16x8 v = __builtin_bit_cast(bf16x8, r[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) t[(8 * c + j) * C::VT_LD + row] = v[j];
    }
  }
}
// A fragment of a transposed tile whose k = 64 rows follow the accumulator order of a
// 4 x (16-row) score block: half c covers rows 32c + 4 lg + {0..3} and 32c + 16 + 4 lg + {0..3}
template <int DH>
__device__ __forceinline__ bf16x8 t_frag(const char* tt, int e, int c, int li, int lg) {
  using C = AttnCfg<DH>;
  const bf16* row = reinterpret_cast<const bf16*>(tt) + (16 * e + li) * C::VT_LD + 32 * c + 4 * lg;
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(row);
  const bf16x4 hi = *reinterpret_cast<const bf16x4*>(row + 16);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// B fragment of this lane's row r over d: k = 32 ks + 8 lg + j
template <int DH>
__device__ __forceinline__ void row_frag(bf16x8 (&f)[AttnCfg<DH>::KS], const bf16* __restrict__ P, long ld, int r,
                                         int L, int lg) {
#pragma unroll
  for (int ks = 0; ks < AttnCfg<DH>::KS; ++ks) {
    const int d0 = 32 * ks + 8 * lg;
    f[ks] = (r < L && d0 < DH) ? *reinterpret_cast<const bf16x8*>(P + (long)r * ld + d0) : bf16x8{};
  }
}
// closing store of N 16-wide accumulator tiles: row 16 e + 4 lg + {0..3} of the lane's column, scaled
template <int N>
__device__ __forceinline__ void store_acc_bf16(bf16* op, const f32x4 (&acc)[N], float scale, int lg) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    bf16x4 w;
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = (bf16)(acc[e][r] * scale);
    *reinterpret_cast<bf16x4*>(op + 16 * e + 4 * lg) = w;
  }
}

// ---- the dh = 32 tile images of the LDS-DMA ring kernels (attn32_dma, attn_bwd_dq32 / dkv32) ----
// A tile is 64 rows x 32 bf16 = 64-B rows, filled by 4 waves x 1 KiB dma_x4 pieces: wave w moves rows
// 16 w .. 16 w + 15, lane l lands at byte 16 l of the piece (row 16 w + l / 4, 16-B position l % 4),
// so an image's swizzle is applied on the SOURCE side (img_src: the chunk that lands there).
namespace t32 {
constexpr int NS = 4;                                   // ring slots
constexpr int TILE = 64 * 64;
// the transposed-readable image: 32-B halves swapped on (row >> 2) & 1, conflict-free both for
// ds_read_b128 row reads (rowfrag) and for ds_read_b64_tr_b16 transposed reads (tfrag)
__device__ __forceinline__ int half_off(int row, int half) { return row * 64 + ((half ^ ((row >> 2) & 1)) << 5); }
__device__ __forceinline__ int img(int row, int chunk) { return half_off(row, chunk >> 1) + ((chunk & 1) << 4); }
__device__ __forceinline__ int img_src(int row, int p) { return (((p >> 1) ^ ((row >> 2) & 1)) << 1) | (p & 1); }
// the forward's K image: chunk XOR (-(key >> 2)) & 3 — conflict-free for the ds_read_b128 lane groups
__device__ __forceinline__ int k_off(int key, int chunk) { return key * 64 + ((chunk ^ ((-(key >> 2)) & 3)) << 4); }
__device__ __forceinline__ bf16x4 tr_read(const char* p) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(bf16x4, v);
}
// A fragment over 64 image rows (MFMA k = 8 lg + j: rows 32 c + 4 lg + {0..3}, 32 c + 16 + 4 lg + {0..3})
// at columns 16 e + li: the transposed tile, read transposed (lane 4 q + p -> row q, columns 4 p .. 4 p + 3)
__device__ __forceinline__ bf16x8 tfrag(const char* im, int e, int c, int li, int lg) {
  const int q = li >> 2, p = li & 3, r0 = 32 * c + 4 * lg + q;
  const bf16x4 lo = tr_read(im + half_off(r0, e) + 8 * p), hi = tr_read(im + half_off(r0 + 16, e) + 8 * p);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 rowfrag(const char* im, int row, int lg) {
  return *reinterpret_cast<const bf16x8*>(im + img(row, lg));
}
}  // namespace t32

// Attention-probability dropout (model/attention/attention.py:28-29) with a counter-based
// RNG, so the forward and both backward kernels regenerate the same keep mask.  One hash
// serves a key PAIR (2j, 2j + 1), 16 bits each:
//   h(q, j) = mix24(base + q * 0x9E3779B1 + j * 0x85EBCA77),
//   base    = fmix32(lo(seed) ^ fmix32(hi(seed) + sh * 0xC2B2AE3D)),   sh = seq * heads + head
//   mix24(h): h ^= h >> 16; h = lo32((h & 0xFFFFFF) * 0xEB352D); h ^= h >> 15;
//             h = lo32((h & 0xFFFFFF) * 0x6CA68B); h ^= h >> 16
// keep (q, k) iff half (k & 1) of h(q, k >> 1) >= thresh (thresh = round(p * 2^16), so the
// drop probability is p to within 2^-17); kept probabilities are scaled by 1 / (1 - p).
// mix24 is the lowbias32 mixer with 24-bit multiplies (v_mul_u32_u24, full VALU rate) instead
// of the quarter-rate 32-bit ones of fmix32: the mask is hashed per probability pair inside the
// VALU-issue-bound attention loops (head dim 32), where fmix32's two v_mul_lo_u32 dominated the
// dropout cost.  Callers keep the hash input additive (drop_row + pair offset * C2) so the
// per-element work is one add plus the mixer.  thresh == 0: no dropout.
// (tests/attn_helpers.py restates it; tests/test_host_cpu.py checks the mask statistics.)
struct AttnDrop {
  uint32_t thresh;
  float scale;
  uint64_t seed;
};
constexpr uint32_t DROP_C1 = 0x9E3779B1u;     // query multiplier
constexpr uint32_t DROP_C2 = 0x85EBCA77u;     // key-pair multiplier
__host__ __device__ inline uint32_t drop_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t drop_mix24(uint32_t h) {
  h ^= h >> 16;
  h = __umul24(h, 0xEB352Du);
  h ^= h >> 15;
  h = __umul24(h, 0x6CA68Bu);
  h ^= h >> 16;
  return h;
}
__host__ __device__ inline uint32_t drop_base(uint64_t seed, uint32_t sh) {
  return drop_fmix32((uint32_t)seed ^ drop_fmix32((uint32_t)(seed >> 32) + sh * 0xC2B2AE3Du));
}
__device__ __forceinline__ uint32_t drop_hash(uint32_t base, uint32_t q, uint32_t pair) {
  return drop_mix24(base + q * DROP_C1 + pair * DROP_C2);
}
// hash input of (q, pair0): add dpair * DROP_C2 for pair0 + dpair
__device__ __forceinline__ uint32_t drop_row(uint32_t base, uint32_t q, uint32_t pair0) {
  return base + q * DROP_C1 + pair0 * DROP_C2;
}
// multipliers of the two keys of a pair from its hash
__device__ __forceinline__ void drop_split(const AttnDrop& d, uint32_t h, float& m0, float& m1) {
  m0 = (h & 0xFFFFu) >= d.thresh ? d.scale : 0.f;
  m1 = (h >> 16) >= d.thresh ? d.scale : 0.f;
}
// probabilities of a key pair after dropout: w = the packed bf16 pair (key 2i low half, 2i + 1
// high half), h = the pair's hash.  A half is dropped iff its hash half < thresh, i.e. iff
// (hash half - thresh) is negative, whose bits 16..31 are then all ones: one byte permute
// gathers those bits of both differences into a drop mask and the kept halves pass unscaled
// (the 1 / (1 - p) scale is applied once to the output).  4 VALU ops per pair instead of two
// compares, two selects, two multiplies and a second conversion.
__device__ __forceinline__ uint32_t drop_pair_apply(uint32_t w, uint32_t h, uint32_t thresh) {
  const uint32_t xlo = (h & 0xFFFFu) - thresh, xhi = (h >> 16) - thresh;
  const uint32_t m = __builtin_amdgcn_perm(xhi, xlo, 0x07060302u);   // [xlo.b2, xlo.b3, xhi.b2, xhi.b3]
  return w & ~m;
}
// dropout multiplier of probability (q, k): 0 or 1 / (1 - p)
__device__ __forceinline__ float drop_mul(const AttnDrop& d, uint32_t base, uint32_t q, uint32_t k) {
  const uint32_t h = drop_hash(base, q, k >> 1);
  return ((k & 1u) ? h >> 16 : h & 0xFFFFu) >= d.thresh ? d.scale : 0.f;
}
// multipliers of (q, k) and (q, k + 1) for even k: one hash
__device__ __forceinline__ void drop_mul2(const AttnDrop& d, uint32_t base, uint32_t q, uint32_t k, float& m0,
                                          float& m1) {
  drop_split(d, drop_hash(base, q, k >> 1), m0, m1);
}
// dq kernels (one query per lane column, keys 16 kt + 4 lg + r down the accumulators): multipliers of
// entries (kt, r), (kt, r + 1), r even, from drow = drop_row(base, q, key pair (64 t + 4 lg) / 2),
// to which (kt, r) adds 8 kt + r / 2; all ones without dropout
__device__ __forceinline__ void drop_mul_dq(const AttnDrop& d, uint32_t drow, int kt, int r, float (&dm)[2]) {
  dm[0] = dm[1] = 1.f;
  if (d.thresh) drop_split(d, drop_mix24(drow + (uint32_t)(8 * kt + (r >> 1)) * DROP_C2), dm[0], dm[1]);
}
// dkv kernels (one key per lane column, queries 64 t + 16 qt + 4 lg + r down the accumulators): the
// keys of a hash pair sit in lanes li, li ^ 1 with the same 16 queries, so each lane hashes half of
// them (r in {0,1} even lanes, {2,3} odd lanes) and swaps with its neighbour (DPP quad_perm
// [1,0,3,2]); it then takes its key's 16-bit half.  mkv is left unset without dropout.
__device__ __forceinline__ void drop_mul_dkv(const AttnDrop& d, uint32_t base, int t, int key, int li, int lg,
                                             float (&mkv)[4][4]) {
  if (!d.thresh) return;
  const bool odd = li & 1;
  // hash input of (query 64 t + 4 lg (+ 2 on odd lanes), this key's pair); (qt, rr) adds (16 qt + rr) * C1
  const uint32_t drow = drop_row(base, (uint32_t)(t * 64 + 4 * lg + (odd ? 2 : 0)), (uint32_t)key >> 1);
#pragma unroll
  for (int qt = 0; qt < 4; ++qt)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const uint32_t hm = drop_mix24(drow + (uint32_t)(16 * qt + rr) * DROP_C1);
      const uint32_t ho = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hm, 0xB1, 0xF, 0xF, false);
      const uint32_t h_lo = odd ? ho : hm, h_hi = odd ? hm : ho;       // hashes of r = rr, 2 + rr
      mkv[qt][rr] = (odd ? h_lo >> 16 : h_lo & 0xFFFFu) >= d.thresh ? d.scale : 0.f;
      mkv[qt][2 + rr] = (odd ? h_hi >> 16 : h_hi & 0xFFFFu) >= d.thresh ? d.scale : 0.f;
    }
}
static inline AttnDrop make_attn_drop(float p, uint64_t seed) {
  AttnDrop d;
  const double t = (double)p * 65536.0 + 0.5;
  d.thresh = p > 0.f ? (t < 1.0 ? 1u : (uint32_t)t) : 0u;
  d.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  d.seed = seed;
  return d;
}

}  // namespace snvrag
