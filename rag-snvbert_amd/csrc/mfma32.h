// Primitives shared by the 32x32-MFMA stream kernels (tail.hip, tailw.hip, sgemm.hip, gemm256.hip):
// every MFMA (v_mfma_f32_32x32x16_bf16) computes a TRANSPOSED tile — 32 weight rows (A operand, a
// 1 KiB fragment) x 32 tokens (B operand) — so a lane (token n = lane % 32, half hh = lane / 32)
// ends up holding 16 consecutive output features of one token.  The weight rows are permuted at pack
// time (out_feat), the k order of the B fragments is in_feat; weights stream as 16 KiB slabs of 16
// fragments.  Everything here is forced inline, constexpr or a literal.
#pragma once
#include "common.h"

#include <utility>

namespace snvrag {

constexpr int FRAG_BYTES = 1024;             // one A fragment: 32 weight rows x 16 k (bf16)
constexpr int SLAB_BYTES = 16 * FRAG_BYTES;  // the unit of the LDS rings

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// feature (within its 32-feature tile; tile T: + 32 T) held by MFMA row m: lane half hh = (m/4)%2,
// accumulator element i = 4(m/8) + m%4, so lane (n, hh) holds features 32 T + 16 hh + i, i < 16
__host__ __device__ constexpr int out_feat(int m) { return 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3); }
__host__ __device__ constexpr int out_feat(int T, int m) { return 32 * T + out_feat(m); }
// input feature at k = 8 kh + j of k-step s (the activations' B fragments and the weights' columns)
__host__ __device__ constexpr int in_feat(int s, int kh, int j) { return 32 * (s >> 1) + 16 * kh + 8 * (s & 1) + j; }

// ---- stream layouts, each stated once: piece pc (16 B = 8 bf16 contiguous in the stream and in the
// source row) is lane l = pc % 64 = (m = l % 32, kh = l / 32) of fragment F = pc / 64 and holds
// W[row][col .. col + 7]
struct PieceSrc { long row, col; };
// stream GEMM (sgemm.hip), W [N, D]: F = T KS + s (output tile T, k-step s)
__host__ __device__ constexpr PieceSrc sgemm_piece_src(int D, long pc) {
  const int KS = D / 16, l = (int)(pc % 64);
  const long F = pc / 64;
  return {32 * (F / KS) + out_feat(l & 31), in_feat((int)(F % KS), l >> 5, 0)};
}
// wide-row GEMM (gemm256.hip), W [32 NT, K]: F = k16 NT + T (k16 step, feature tile T), plain k order
__host__ __device__ constexpr PieceSrc gemm256_piece_src(int NT, long pc) {
  const int l = (int)(pc % 64);
  const long F = pc / 64;
  return {out_feat((int)(F % NT), l & 31), 16 * (F / NT) + 8 * (l >> 5)};
}

// calls body(std::integral_constant<int, I>{}) for I = 0 .. N-1: a forced full unroll (every
// register-array index in the body is a compile-time constant)
template <typename Body, int... Is>
__device__ __forceinline__ void unroll(Body&& body, std::integer_sequence<int, Is...>) {
  (body(std::integral_constant<int, Is>{}), ...);
}

__device__ __forceinline__ f32x16 mfma32(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// The MFMA as inline asm, so that the register class of every accumulator is fixed (AGPR or VGPR;
// the builtin's single form for the whole kernel spills half of 384 accumulator registers).  The
// compiler then does not know these are MFMAs: nothing may read an accumulator within 18 wait
// states of its last MFMA unless drain() runs in between — including the compiler's own register
// moves — and it pads nothing inside the asm string: NOP puts an s_nop 1 ahead of the MFMA, for
// segments where a VALU write of an operand can land within 2 wait states of it
// (tests/test_asm_hazards.py scans for both).  Every call states both arguments.
template <bool AGPR, bool NOP>
__device__ __forceinline__ void mfma32_asm(f32x16& c, const u32x4& a, const u32x4& b) {
  if constexpr (AGPR && NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else if constexpr (AGPR)
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// zero C operand: the accumulator's first k-step
template <bool AGPR, bool NOP>
__device__ __forceinline__ void mfma32_asm0(f32x16& c, const u32x4& a, const u32x4& b) {
  if constexpr (AGPR && NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
  else if constexpr (AGPR)
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
  else if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(c) : "v"(a), "v"(b));
}
// 32x32 MFMA (16 passes): a result is readable 18 wait states after issue
__device__ __forceinline__ void drain() { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory"); }

// lane id produced afresh at each use (volatile: not CSE'd with earlier ones), so no lane-derived
// address stays live across a K loop or the FFN and gets spilled
__device__ __forceinline__ int lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// x + x of the lane 32 apart (the row reductions over the two lane halves)
__device__ __forceinline__ float xsum32(float x) {
  return x + __int_as_float(__builtin_amdgcn_ds_bpermute((lane_id() ^ 32) << 2, __float_as_int(x)));
}

// two floats -> packed bf16 pair (RNE) in ONE v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
// the two bf16 of a packed word as floats (low half first); element j of 8 packed in a u32x4
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ f32x2 bf_pair(uint32_t u) { return f32x2{bf_lo(u), bf_hi(u)}; }
__device__ __forceinline__ float bf_at(const u32x4& v, int j) { return (j & 1) ? bf_hi(v[j >> 1]) : bf_lo(v[j >> 1]); }

// LeakyReLU(0.1) in 2 VALU ops (fmaxf on a register hipcc cannot prove canonical costs a third,
// a v_max x, x canonicalisation)
__device__ __forceinline__ float lrelu(float x) {
  float r;
  asm("v_mul_f32 %0, 0x3dcccccd, %1\n v_max_f32 %0, %1, %0" : "=&v"(r) : "v"(x));
  return r;
}
// MAF weight of an allele frequency (fusion.py:155-160)
__device__ __forceinline__ float maf_w(float af) {
  const float maf = fminf(af, 1.0f - af);
  return fminf(log1pf(1.0f / (maf + 1e-6f)), 3.0f);
}

// 32-bit LDS byte address of a pointer into dynamic shared memory (an address-space cast; common.h's
// lds_addr is the wave-uniform form)
__device__ __forceinline__ uint32_t lds_byte_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
// 16 consecutive floats of an LDS table at byte address `addr` (this lane's features 16 hh .. +15
// of a 32-feature tile): reads and their wait in ONE asm statement, so the compiler can neither
// hoist them nor keep whole tables live in registers across a phase, and its own wait for an LDS
// read would cover the whole in-flight weight stream
__device__ __forceinline__ void ld16(uint32_t addr, float (&v)[16]) {
  u32x4 r[4];
  asm volatile(
      "ds_read_b128 %0, %4 offset:0\n ds_read_b128 %1, %4 offset:16\n ds_read_b128 %2, %4 offset:32\n"
      " ds_read_b128 %3, %4 offset:48\n s_waitcnt lgkmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
      : "v"(addr));
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = __uint_as_float(r[i >> 2][i & 3]);
}

// ---- first-round stagger.  Every workgroup runs the same weight stream for the same time, so
// without this all 256 CUs start each round together and the prologue's activation + residual
// loads (block tail: 192 KB per CU) and the epilogue's stores hit HBM as one chip-wide burst
// (measured: prologue 12 % of the wave, HBM-bound at ~4 TB/s, then idle HBM for the rest of the
// round).  The first round's workgroups start at 8 phase offsets of `step` cycles (per XCD: dispatch
// order blockIdx / 8), so later rounds stay spread and each CU's bursts overlap other CUs' MFMA
// phases.  The delay is paid once per CU; with >= 17 blocks per CU it ends inside the last partial
// round's slack.  Each kernel guards the call itself (first-round workgroups, step > 0).
__device__ __forceinline__ void stagger_wait(int step) {
  const long wait = (long)step * ((blockIdx.x >> 3) & 7);
  const long t0 = (long)__builtin_amdgcn_s_memtime();
  while ((long)__builtin_amdgcn_s_memtime() - t0 < wait) __builtin_amdgcn_s_sleep(16);
}
// the launch side: the step in cycles for a launch of nwg workgroups — none below min_nwg (the delay
// must be won back over several rounds); option value opt >= 0 overrides the measured default
static inline int stagger_step(long nwg, long min_nwg, int64_t opt, int dflt) {
  return nwg >= min_nwg ? (opt >= 0 ? (int)opt : dflt) : 0;
}

}  // namespace snvrag
