// Block tail, wide-row form (option tail_wide), D = 384, eval — the same function as tail_kernel
// (csrc/tail.hip) on the same packed weight stream and vector tables:
//
//   x1  = LN1(x + att W_o^T + b_o)                     multi_head_attention.py:51, sublayer.py:15-16
//   x   = LN2(x1 + lrelu(LN_f(lrelu(x1 W1^T + b1)) W2^T + b2))   feed_forward.py:18-21
//
// tail_kernel gives each wave 32 token rows and ALL features, so every weight fragment is read
// from LDS by all four waves and the 2.65 MB stream enters each CU by LDS-DMA, whose issue cost
// (~60 cycles per 1 KiB piece, serialised with the wave's MFMAs at one wave per SIMD) caps it at
// ~41 % of the MFMA peak.  Here the roles are transposed, like the wide-row GEMM (gemm256.hip):
// a workgroup owns 128 rows (4 token groups of 32) and wave w owns FEATURES — output tiles
// 3w .. 3w+2 of the out-projection and of FFN2, and hidden chunks 4c + w of FFN1 — so every W
// fragment is loaded ONCE per workgroup straight into the registers of the one wave that uses it
// (buffer_load_dwordx4, three k16 steps ahead) and feeds four MFMAs (one per token group); the
// activations are the LDS-resident operands instead:
//   X [24 k16 steps][4 groups] x 1 KiB B-fragment images (96 KiB): att by LDS-DMA in the prologue,
//     then x1 (written by LN1, read by every FFN1 k-step and as the LN2 residual);
//   H [4 chunks][4 k16 steps][4 groups] x 1 KiB (64 KiB): the bf16 hidden of one round of four
//     64-unit chunks (one per wave), the B fragments of FFN2 — the packed W2' k order makes a
//     lane's 8 consecutive FFN1 accumulators exactly its 16-B slot of an FFN2 B fragment.
// Per round c (6 rounds): FFN1 of chunk 4c + w (24 k16 steps x 2 tiles x 4 groups = 192 MFMAs),
// barrier, the chunk epilogue (b1, LeakyReLU, LN_f sums, bf16 into H), barrier, FFN2 over the
// round's 4 chunks (16 k16 steps x 3 tiles x 4 groups = 192 MFMAs).  Row statistics (LN1, LN_f,
// LN2) are per-wave partials combined through LDS.
// The W fragment loads are inline asm with hand-counted s_waitcnt vmcnt (tw_younger): the
// compiler sees no loads, so it neither drains them at loop edges nor reorders around them; the
// MFMAs are inline asm too (fixed AGPR / VGPR accumulators), so every accumulator read waits for
// drain() (the compiler's hazard recognizer does not know these are MFMAs).
#include "common.h"
#include "mfma32.h"

namespace snvrag {

#ifndef TW_PACKED_LN
#define TW_PACKED_LN 1                               // LayerNorm epilogues in packed f32 (v_pk_*) math
#endif

constexpr int TW_D = 384, TW_NT = 12, TW_KS = 24;
constexpr int TW_FPRE = TW_NT * TW_KS;               // W_o' fragments (288)
constexpr int TW_FPC = 96;                           // fragments per 64-unit chunk: W1 48, W2' 48
constexpr int TW_NFRAG = TW_FPRE + 24 * TW_FPC;      // whole stream (2592)
constexpr int TW_X = 0;                              // LDS: X images (96 KiB)
constexpr int TW_H = 96 * 1024;                      // LDS: H images (64 KiB)
constexpr int TW_LDS = 160 * 1024;
// W fragments: one stream per wave in consumption order, TW_AH fragments in flight ahead of the
// step being consumed, in a ring of TW_RING registers (fragment n in register n % 12)
constexpr int TW_AH = 9;
constexpr int TW_RING = 12;
// k16 steps: q in [0, 24) phase A (3 W_o' fragments each); [24, 48) FFN1 of half-round 0 (1 W1
// fragment); half-round h = 1 .. 11: 32 steps at 48 + 32 (h - 1): FFN1(h) x 24 (1), FFN2(h - 1) x 8
// (3 W2' fragments); [400, 408) FFN2(11)
constexpr int TW_QA = 24;
constexpr int TW_Q0 = 48;
constexpr int TW_HS = 32;
constexpr int TW_QF = TW_Q0 + 11 * TW_HS;
constexpr int TW_QEND = TW_QF + 8;
constexpr int TW_QREP = TW_Q0 + TW_HS;               // half-round 2: the loop's representative steps
constexpr int TW_NB1 = 4;                            // b1 loads of one half-round's tile

__host__ __device__ constexpr int tw_nf(int q) {
  return q < 0 ? 0 : q < TW_QA ? 3 : q < TW_Q0 ? 1 : q < TW_QF ? ((q - TW_Q0) % TW_HS < 24 ? 1 : 3) : q < TW_QEND ? 3 : 0;
}
__host__ __device__ constexpr int tw_f0(int q) {     // first fragment of step q
  if (q <= TW_QA) return 3 * q;
  if (q <= TW_Q0) return 72 + (q - TW_QA);
  if (q <= TW_QF) {
    const int k = (q - TW_Q0) / TW_HS, r = (q - TW_Q0) % TW_HS;
    return 96 + 48 * k + (r <= 24 ? r : 24 + 3 * (r - 24));
  }
  return q <= TW_QEND ? 624 + 3 * (q - TW_QF) : 648;
}
__host__ __device__ constexpr int tw_step_of(int m) {  // the step that consumes fragment m
  if (m < 72) return m / 3;
  if (m < 96) return TW_QA + (m - 72);
  if (m < 624) {
    const int k = (m - 96) / 48, r = (m - 96) % 48;
    return TW_Q0 + TW_HS * k + (r < 24 ? r : 24 + (r - 24) / 3);
  }
  return TW_QF + (m - 624) / 3;
}
constexpr int TW_NFRAGW = 648;                       // fragments per wave
// the b1 loads (after the step's W loads): half-round 0's at its FFN1 step 16, half-round h's
// (h >= 1) at the first FFN2 step of its iteration
__host__ __device__ constexpr int tw_extra(int q) {
  return (q == TW_QA + 16 || (q >= TW_Q0 && q < TW_QF && (q - TW_Q0) % TW_HS == 24)) ? TW_NB1 : 0;
}
// the step during which fragment n is issued (-1: the prologue); step q issues [f0(q) + AH, + nf(q))
__host__ __device__ constexpr int tw_issuer(int n) { return n < TW_AH ? -1 : tw_step_of(n - TW_AH); }
__host__ __device__ constexpr int tw_min(int a, int b) { return a < b ? a : b; }
// vector-memory ops issued after step q's last fragment up to the wait before step q's MFMAs
__host__ __device__ constexpr int tw_younger(int q) {
  const int nl = tw_f0(q) + tw_nf(q) - 1;
  int n = tw_min(tw_f0(q) + TW_AH, TW_NFRAGW) - 1 - nl;
  const int qi = tw_issuer(nl);
  for (int j = qi < 0 ? 0 : qi; j < q; ++j) n += tw_extra(j);
  return n;
}
// ops issued during steps qa+1 .. qb
__host__ __device__ constexpr int tw_ops_between(int qa, int qb) {
  int n = 0;
  for (int q = qa + 1; q <= qb; ++q) n += (tw_f0(q) + TW_AH < TW_NFRAGW ? tw_nf(q) : 0) + tw_extra(q);
  return n;
}
// b1 of half-round h - 1 waited for at FFN1 step 2 of half-round h (h = 1: loaded at step 40; h >= 2:
// at the previous iteration's first FFN2 step): the smaller count is safe for every h
constexpr int TW_B1_WAIT = tw_min(tw_ops_between(TW_QA + 16, TW_Q0 + 2), tw_ops_between(TW_Q0 + 24, TW_QREP + 2));
// b1 of half-round 11 (loaded at step 392), waited for after step 399
constexpr int TW_B1_WAIT_END = tw_ops_between(TW_Q0 + 10 * TW_HS + 24, TW_QF - 1);
// the loop body serves half-rounds 1 .. 11: its wait at step i of an iteration is the smallest
// count over them (h = 1 sees half-round 0's b1 loads in its first windows) — a smaller count only
// waits for more
__host__ __device__ constexpr int tw_younger_it(int i) {
  int m = 63;
  for (int h = 1; h <= 11; ++h) m = tw_min(m, tw_younger(TW_Q0 + (h - 1) * TW_HS + i));
  return m;
}
// step q's wait: in the loop (the representative half-round's steps) the iteration minimum
__host__ __device__ constexpr int tw_wait_of(int q) {
  return (q >= TW_QREP && q < TW_QREP + TW_HS) ? tw_younger_it(q - TW_QREP) : tw_younger(q);
}
__host__ __device__ constexpr bool tw_ring_periodic() {
  return tw_f0(TW_QEND) == TW_NFRAGW && tw_f0(TW_QA) % TW_RING == 0 && tw_f0(TW_Q0) % TW_RING == 0 &&
         tw_f0(TW_QREP) % TW_RING == 0 && (tw_f0(TW_QREP + TW_HS) - tw_f0(TW_QREP)) % TW_RING == 0 &&
         tw_f0(TW_QF) % TW_RING == 0;
}
static_assert(tw_ring_periodic(), "fragment ring registers periodic over the sections");
static_assert(TW_B1_WAIT_END <= 63 && tw_younger(0) <= 63, "vmcnt range");

// mfma32_asm's NOP (mfma32.h): outside the FFN loop (phase A, half-round 0, the last half-rounds)
// hipcc stashes W fragments in AGPRs and reads one back right before its MFMA (a VALU write of an
// operand: 2 wait states); the loop body has no such write (tests/test_asm_hazards.py scans for it)
// TW_NOPMASK: which MFMA segments outside the FFN loop carry the s_nop (bit 0 phase A, bit 1 FFN1(0),
// bit 2 the last FFN1 / FFN2 of the loop's tail, bit 3 FFN2(11), bit 4 the projection phase); the
// 32-row (G = 1) body always.
// r6: only FFN1(0) gets a VALU write of an MFMA operand within 2 wait states without it (a scan of
// each segment with its s_nop removed: tests/test_asm_hazards.py keeps checking the build)
#ifndef TW_NOPMASK
#define TW_NOPMASK 2
#endif
// the drain with the accumulators as operands: no read or register move of them (a compiler copy is
// not a memory access and crossed the plain drain) can be scheduled before it
__device__ __forceinline__ void tw_drain_o(f32x16 (&a)[3][4]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7"
               : "+a"(a[0][0]), "+a"(a[0][1]), "+a"(a[0][2]), "+a"(a[0][3]), "+a"(a[1][0]), "+a"(a[1][1]),
                 "+a"(a[1][2]), "+a"(a[1][3]), "+a"(a[2][0]), "+a"(a[2][1]), "+a"(a[2][2]), "+a"(a[2][3])
               :: "memory");
}
template <bool AGPR> __device__ __forceinline__ void tw_drain_h4(f32x16 (&h)[4]) {
  if constexpr (AGPR)
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+a"(h[0]), "+a"(h[1]), "+a"(h[2]), "+a"(h[3]) :: "memory");
  else
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]) :: "memory");
}
__device__ __forceinline__ f32x2 tw_lrelu2(f32x2 x) {
  const f32x2 m = x * 0.1f;                           // one v_pk_mul_f32
  float a, b;
  asm("v_max_f32 %0, %1, %2" : "=v"(a) : "v"(x.x), "v"(m.x));
  asm("v_max_f32 %0, %1, %2" : "=v"(b) : "v"(x.y), "v"(m.y));
  return f32x2{a, b};
}
// ld16 by plain LDS reads (LN phases: no LDS-DMA is in flight there, so the compiler's waits
// count only these reads and it may issue the next tile's reads under this tile's math)
__device__ __forceinline__ void tw_ld16p(const char* p, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + 16 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[4 * i + j] = q[j];
  }
}
// wait until at most Y younger vector-memory ops are in flight; the fragments' uses are ordered after it
#ifndef TW_ASM_WAITS
#define TW_ASM_WAITS 0                                 // 1: hand-counted waits on asm loads (diagnostics)
#endif
template <int Y> __device__ __forceinline__ void tw_wait1(u32x4& a) {
  static_assert(Y >= 0 && Y <= 63, "vmcnt range");
  if constexpr (TW_ASM_WAITS) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(Y) : "memory");
}
template <int Y> __device__ __forceinline__ void tw_wait3(u32x4& a, u32x4& b, u32x4& c) {
  static_assert(Y >= 0 && Y <= 63, "vmcnt range");
  if constexpr (TW_ASM_WAITS) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(Y) : "memory");
}
template <int OFF> __device__ __forceinline__ void tw_load_off(u32x4& r, int voff, const i32x4& rsrc, int so) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(so), "n"(OFF) : "memory");
}
__device__ __forceinline__ void tw_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct TwArgs {
  int M;
  const bf16* att;          // [M, D]
  const bf16* resid;        // [M, D] (x; out may alias it)
  bf16* out;                // [M, D]
  const char* ws;           // snvrag_tail_pack stream
  const float* vec;         // [b1 4D | b2' | c1 | g2 | be2]
  const float* b_o; const float* g1; const float* be1;
  float eps;
  int desync;
  unsigned long long* stamps;   // STAMP: [workgroup][wave][8] s_memtime stamps
  int n_full;                   // workgroups of 128 rows (the rest: 32 rows)
  // the projection phase (null: none): qkv_out[M, 3 D] = out W^T + pbias, the next layer's QKV
  const char* pw;               // snvrag_proj_pack stream, NC = 3
  const float* pbias;           // [3 D]
  bf16* qkv_out;                // [M, 3 D], M 3 D 2 bytes < 2^31
};

// ---- the wide-row projection's chunk loop: out[rows of the tile][NC D] = X W^T + bias, the tail's
// phase A per output chunk c of D features, shared by projw_kernel (G = 4) and the block tail's
// projection phase (G = 4 and the 32-row body's G = 1): per chunk 24 k16 steps x 3 tiles x G token
// groups into the phase-A accumulators, then + bias -> bf16 -> two 16-B stores per (tile, token
// group) through the bounds-checked resource `ors` (rows >= M are dropped).  The caller has the X
// images complete and visible (a barrier), the bias table (f32 [NC D]) at LDS byte address
// `bias_lds`, and the first TW_AH fragments of the wave's stream in flight in wf[0 .. TW_AH) (pw_loadW).
// W fragments (snvrag_proj_pack: chunk c, k16 step s, tile T at fragment c 288 + 12 s + T): fragment n
// of wave w's stream = chunk n / 72, k16 step (n % 72) / 3, tile 3w + n % 3 (past the last chunk: the
// last chunk again, never consumed), compiler-visible loads through the 12-register ring, TW_AH ahead
__device__ __forceinline__ void pw_loadW(u32x4& r, const __amdgpu_buffer_rsrc_t wrb, int lane16, int wave, int NC, int c,
                                         int n72) {
  const int cc = c < NC ? c : NC - 1;
  r = __builtin_amdgcn_raw_buffer_load_b128(wrb, lane16, (cc * TW_FPRE + (n72 / 3) * TW_NT + 3 * wave + n72 % 3) * FRAG_BYTES, 0);
}
template <int G, bool NOP>
__device__ __forceinline__ void pw_chunks(const char* smem, uint32_t bias_lds, int wave, int lane16,
                                          const __amdgpu_buffer_rsrc_t wrb, int NC, const __amdgpu_buffer_rsrc_t ors,
                                          u32x4 (&wf)[TW_RING], f32x16 (&acc)[3][4]) {
  constexpr int D = TW_D, KS = TW_KS, GI = G > 1 ? 1 : 0;
  auto rdB = [&](int blk) -> u32x4 { return *reinterpret_cast<const u32x4*>(smem + TW_X + blk * FRAG_BYTES + lane16); };
  u32x4 bq[2][4];
#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int g = 0; g < G; ++g) bq[0][g] = rdB(g);
    unroll([&](auto sc) {
      constexpr int s = decltype(sc)::value, n0 = 3 * s;
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if constexpr (s == 0) mfma32_asm0<true, NOP>(acc[t][g], wf[(n0 + t) % TW_RING], bq[s & 1][g]);
          else mfma32_asm<true, NOP>(acc[t][g], wf[(n0 + t) % TW_RING], bq[s & 1][g]);
        }
        if constexpr (s + 1 < KS) bq[(s + 1) & 1][g] = rdB((s + 1) * 4 + g);
        if (g == GI) {
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const int m = n0 + TW_AH + t;              // within [0, 72 + 9): this chunk or the next
            if (m < 72) pw_loadW(wf[(n0 + TW_AH + t) % TW_RING], wrb, lane16, wave, NC, c, m);
            else pw_loadW(wf[(n0 + TW_AH + t) % TW_RING], wrb, lane16, wave, NC, c + 1, m - 72);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, KS>{});
    tw_drain_o(acc);
    // + bias -> bf16 -> out[row][c D + 32 T + 16 hh .. + 15]
    const int l = lane_id();
    const uint32_t bb = bias_lds + 4 * (c * D + 16 * (l >> 5));
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int T = 3 * wave + t;
      float bv[16];
      ld16(bb + 4 * 32 * T, bv);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int ro = ((32 * g + (l & 31)) * NC * D + c * D + 32 * T + 16 * (l >> 5)) * 2;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          float y[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] = acc[t][g][8 * h2 + j] + bv[8 * h2 + j];
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{pack2(y[0], y[1]), pack2(y[2], y[3]), pack2(y[4], y[5]),
                                                       pack2(y[6], y[7])},
                                                 ors, ro + 16 * h2, 0, 0);
        }
      }
    }
  }
}
// the bounds-checked output resource of a tile whose first row is row0: rows [row0, M) of out[M, NC D]
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pw_out_rsrc(bf16* out, int M, long row0, int NC) {
  const long o_bytes = ((long)M - row0) * NC * TW_D * 2;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(out + row0 * NC * TW_D), (short)0,
                                           (int)(o_bytes < 0x7fffffffL ? o_bytes : 0x7fffffffL), 0x00020000);
}

// G token groups of 32 rows (G = 4: a 128-row tile; G = 1: the 32-row tiles that spread the last
// partial round of 128-row tiles over more CUs, tailw_kernel below).  GI: the group after whose
// MFMAs a step issues its W loads.  PROJ: the projection phase after LN2 (p.pw set): the tile's output
// rows, in registers as bf16 when LN2 stores them, also go into the X images (LN1's layout for x1) and
// are multiplied by the next layer's W_qkv (pw_chunks, NC = 3) — the rows never come back from HBM
template <bool STAMP, int G, bool PROJ>
__device__ __forceinline__ void tailw_body(const TwArgs& p, const long row0, const int wave) {
  constexpr int D = TW_D, NT = TW_NT, GI = G > 1 ? 1 : 0;
  constexpr uint32_t TW_PB = TW_H + 16 * 1024;        // LDS: the projection's bias table (3 D f32, 5 KiB of H half 0)
  // the residual rows are loaded during phase A, after step TW_RES_STEP's W loads, not in the
  // prologue: the prologue's HBM burst halves, -2 k cycles per wave net (r6)
  constexpr int TW_RES_STEP = 21;
  // s_nop ahead of the inline-asm MFMAs of a segment (TW_NOPMASK bit b, or the 32-row body)
  constexpr bool NOPA = G == 1 || (TW_NOPMASK & 1), NOP0 = G == 1 || (TW_NOPMASK & 2);
  constexpr bool NOPT = G == 1 || (TW_NOPMASK & 4), NOPF = G == 1 || (TW_NOPMASK & 8);
  constexpr bool NOPP = G == 1 || (TW_NOPMASK & 16);
  using TNA = std::integral_constant<bool, NOP0>;
  using TNT = std::integral_constant<bool, NOPT>;
  using TNF = std::integral_constant<bool, NOPF>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (wave: made once by the kernel; the thread index is re-made from it and a fresh lane id where
  // used, so that the launch's v0 does not stay live through the bodies the kernel holds)
  unsigned long long st[8] = {};
  auto stamp = [&](int i) {
    if constexpr (STAMP) st[i] = __builtin_amdgcn_s_memtime();
  };
  if (p.desync > 0 && blockIdx.x < 256) stagger_wait(p.desync);   // first-round stagger (mfma32.h)
  stamp(0);
  const uint32_t lds0 = lds_addr(smem);
  int lane16 = lane_id() * 16;                        // (lane-derived values are re-made from a fresh
  asm volatile("" : "+v"(lane16));                    //  v_mbcnt where used: kept live across the FFN they spill)

  // ---- prologue: att -> X by LDS-DMA (wave w: token group w, k16 steps in order; lane (n, kh) of
  // piece s reads att[32 w + n][in_feat(s, kh, 0 .. 7)]), the first W steps, the residual rows
  // (VGPRs, used by LN1), the LN1 tables -> H
  const i32x4 ars = dma_rsrc(p.att + row0 * D, ((long)p.M - row0) * D * 2);   // rows >= M read as 0
  const i32x4 wrs = dma_rsrc(p.ws, (long)TW_NFRAG * FRAG_BYTES);
  const i32x4 brs = dma_rsrc(p.vec, 4L * D * 4);                             // b1
  {
    const int l = lane_id();
    const int voff = (32 * wave + (l & 31)) * (D * 2) + 32 * (l >> 5);
    if (wave < G) {
#pragma unroll
      for (int s = 0; s < TW_KS; ++s)
        dma_x4(ars, lds0 + TW_X + (s * 4 + wave) * FRAG_BYTES, voff, 64 * (s >> 1) + 16 * (s & 1));
    }
  }
  u32x4 wf[TW_RING];                                 // W fragment ring
  // W fragment F of the stream into register r (soffset: scalar)
  // (compiler-visible loads: its waitcnt pass places the waits before every read of the register —
  // hand-counted asm loads were seen copied into AGPRs by the register allocator before they landed)
  const __amdgpu_buffer_rsrc_t wrb = __builtin_amdgcn_make_buffer_rsrc((void*)p.ws, (short)0, TW_NFRAG * FRAG_BYTES, 0x00020000);
  auto loadW = [&](u32x4& r, int F) { r = __builtin_amdgcn_raw_buffer_load_b128(wrb, lane16, F * FRAG_BYTES, 0); };
  // stream offsets: FFN1(h) step i = wave w's tile of chunk 4 (h >> 1) + w, half h & 1;
  // FFN2(h) step u, tile t = chunk 4 (h >> 1) + u / 2, k16 step 2 (h & 1) + u % 2, tile 3w + t
  auto f_ffn1 = [&](int h, int i) { return TW_FPRE + (4 * (h >> 1) + wave) * TW_FPC + 2 * i + (h & 1); };
  auto f_ffn2 = [&](int h, int u, int t) {
    return TW_FPRE + (4 * (h >> 1) + (u >> 1)) * TW_FPC + 48 + (2 * (h & 1) + (u & 1)) * NT + 3 * wave + t;
  };
  // fragment n of the prologue / phase A / half-round 0 (n < 120: W_o' k16 step n / 3 tile n % 3,
  // FFN1(0), FFN1(1))
  auto issue_a = [&](auto n_tag) {
    constexpr int n = decltype(n_tag)::value;
    if constexpr (n < 72) loadW(wf[n % TW_RING], (n / 3) * NT + 3 * wave + n % 3);
    else if constexpr (n < 96) loadW(wf[n % TW_RING], f_ffn1(0, n - 72));
    else loadW(wf[n % TW_RING], f_ffn1(1, n - 96));
  };
  unroll([&](auto nc) { issue_a(nc); }, std::make_integer_sequence<int, TW_AH>{});
  u32x4 rr[3][4][2];                                 // residual x: tile t, group g, half h2
  // (issued after phase A step TW_RES_STEP's W loads; the W waits after it then also wait for these
  // rows, in-order vmcnt)
  auto load_res = [&]() {
    const int l = lane_id();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      long r = row0 + 32 * g + (l & 31);
      r = r < p.M ? r : (long)p.M - 1;
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
          rr[t][g][h2] = *reinterpret_cast<const u32x4*>(p.resid + r * D + 32 * (3 * wave + t) + 16 * (l >> 5) + 8 * h2);
    }
  };
  float* tab = reinterpret_cast<float*>(smem + TW_H);                        // [b_o | g1 | be1]
  for (int i = 64 * wave + lane_id(); i < D; i += 256) {
    tab[i] = p.b_o[i];
    tab[D + i] = p.g1[i];
    tab[2 * D + i] = p.be1[i];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  tw_barrier();
  stamp(1);

  // ---- phase A: ao = att W_o'^T (wave w: tiles 3w .. 3w+2 x 4 token groups, AGPRs)
  f32x16 acc[3][4];
  u32x4 bq[3][4];                                     // B fragments, read two k16 steps ahead
  auto rdB = [&](uint32_t base, int blk) -> u32x4 {
    return *reinterpret_cast<const u32x4*>(smem + base + blk * FRAG_BYTES + lane16);
  };
  // (B fragments one step ahead in two buffers here: 12 MFMAs per step cover the LDS latency, and
  // a third buffer beside the residual rows pushed the W fragments into AGPR copies taken before
  // their loads had landed)
#pragma unroll
  for (int g = 0; g < G; ++g) bq[0][g] = rdB(TW_X, g);
  unroll([&](auto qc) {
    constexpr int q = decltype(qc)::value, n0 = 3 * q;
    tw_wait3<tw_younger(q)>(wf[n0 % TW_RING], wf[(n0 + 1) % TW_RING], wf[(n0 + 2) % TW_RING]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if constexpr (q == 0) mfma32_asm0<true, NOPA>(acc[t][g], wf[(n0 + t) % TW_RING], bq[q & 1][g]);
        else mfma32_asm<true, NOPA>(acc[t][g], wf[(n0 + t) % TW_RING], bq[q & 1][g]);
      }
      if constexpr (q + 1 < TW_KS) bq[(q + 1) & 1][g] = rdB(TW_X, (q + 1) * 4 + g);
      if (g == GI)
        unroll([&](auto tc) { issue_a(std::integral_constant<int, n0 + TW_AH + decltype(tc)::value>{}); },
                  std::make_integer_sequence<int, 3>{});
    }
    if constexpr (q == TW_RES_STEP) load_res();
    __builtin_amdgcn_sched_barrier(0);
  }, std::make_integer_sequence<int, TW_QA>{});
  tw_drain_o(acc);
  stamp(2);

  // ---- LN1 over the 4 waves' features: v = ao + b_o + x; per-wave (sum, sumsq) -> LDS
  float2* s1 = reinterpret_cast<float2*>(smem + TW_H + 8 * 1024);          // [wave][128 rows]
  {
    const uint32_t tb = lds0 + TW_H + 64 * (lane_id() >> 5);
#if TW_PACKED_LN
    // (packed f32 math: pairs of features per v_pk_* instruction)
    f32x2 s2v[4], q2v[4];
#pragma unroll
    for (int g = 0; g < G; ++g) s2v[g] = q2v[g] = f32x2{0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      float bo[16];
      tw_ld16p(smem + (tb - lds0) + 4 * 32 * (3 * wave + t), bo);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2 v = f32x2{acc[t][g][2 * e], acc[t][g][2 * e + 1]} + f32x2{bo[2 * e], bo[2 * e + 1]} +
                          bf_pair(rr[t][g][e >> 2][e & 3]);
          acc[t][g][2 * e] = v.x;
          acc[t][g][2 * e + 1] = v.y;
          s2v[g] += v;
          q2v[g] = v * v + q2v[g];
        }
    }
    float sum[4], sq[4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sum[g] = s2v[g].x + s2v[g].y;
      sq[g] = q2v[g].x + q2v[g].y;
    }
#else
    float sum[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      float bo[16];
      tw_ld16p(smem + (tb - lds0) + 4 * 32 * (3 * wave + t), bo);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[t][g][i] + bo[i] + bf_at(rr[t][g][i >> 3], i & 7);
          acc[t][g][i] = v;
          sum[g] += v;
          sq[g] = fmaf(v, v, sq[g]);
        }
    }
#endif
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int g = 0; g < G; ++g) {}   // v back in AGPRs
    const int l = lane_id();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sum[g] = xsum32(sum[g]);
      sq[g] = xsum32(sq[g]);
      s1[wave * 128 + 32 * g + (l & 31)] = make_float2(sum[g], sq[g]);
    }
  }
  tw_barrier();                                       // every wave past phase A: X is free for x1
  {
    const int l = lane_id();
    const uint32_t tb = lds0 + TW_H + 64 * (l >> 5);
    float mean[4], rstd[4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {
        const float2 v = s1[w2 * 128 + 32 * g + (l & 31)];
        a += v.x;
        b += v.y;
      }
      mean[g] = a * (1.0f / D);
      rstd[g] = 1.0f / sqrtf(fmaxf(b * (1.0f / D) - mean[g] * mean[g], 0.f) + p.eps);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      float gg[16], bb[16];
      tw_ld16p(smem + (tb - lds0) + 4 * (D + 32 * (3 * wave + t)), gg);
      tw_ld16p(smem + (tb - lds0) + 4 * (2 * D + 32 * (3 * wave + t)), bb);
      const int T = 3 * wave + t;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float y[16];
#if TW_PACKED_LN
        const float nmr = -mean[g] * rstd[g];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2 z = (f32x2{acc[t][g][2 * e], acc[t][g][2 * e + 1]} * rstd[g] + nmr) * f32x2{gg[2 * e], gg[2 * e + 1]} +
                          f32x2{bb[2 * e], bb[2 * e + 1]};
          y[2 * e] = z.x;
          y[2 * e + 1] = z.y;
        }
#else
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] = (acc[t][g][i] - mean[g]) * rstd[g] * gg[i] + bb[i];
#endif
        // x1 features 32T + 16hh + 8h2 + j = k16 step 2T + h2, lane slot (n, kh = hh)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
          *reinterpret_cast<u32x4*>(smem + TW_X + ((2 * T + h2) * 4 + g) * FRAG_BYTES + lane16) =
              u32x4{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                    pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
      }
    }
  }
  tw_barrier();                                       // x1 complete in X
  stamp(3);

  // ---- FFN in 12 half-rounds.  Half-round h: wave w's FFN1 tile (32 hidden units: chunk
  // 4 (h >> 1) + w, half h & 1) over all 128 rows into hv / ha (even / odd h: VGPRs / AGPRs), while
  // the chunk epilogue of half-round h - 1 (b1, LeakyReLU, LN_f sums, bf16) is interleaved between
  // its MFMAs and writes that hidden into H half (h - 1) & 1; one barrier; then FFN2 of half-round
  // h - 1 (the 4 waves' tiles = 8 k16 steps) from that H half.  H is double-buffered, so the next
  // half-round's epilogue writes the other half while this FFN2 reads.
  // B fragments: FFN2 step u uses bq[u % 3], FFN1 step i bq[(i + 2) % 3] (so that FFN2's
  // last two steps prefetch the next FFN1's first two), each read two steps ahead.
  f32x16 hv[4], ha[4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[t][g] = f32x16{};
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g) asm volatile("" : "+a"(acc[t][g]));
  typedef float f2 __attribute__((ext_vector_type(2)));
  float sa1[4], sa2[4];                               // LN_f partial sums of this lane's hidden units
#pragma unroll
  for (int g = 0; g < G; ++g) sa1[g] = sa2[g] = 0.f;
  u32x4 b1v[4];                                       // b1 of the tile whose epilogue runs next
  const __amdgpu_buffer_rsrc_t b1b = __builtin_amdgcn_make_buffer_rsrc((void*)p.vec, (short)0, 4 * D * 4, 0x00020000);
  auto b1_load = [&](int h) {                         // b1[64 c' + 32 (h & 1) + 8 r + 4 hh .. + 3]
    const int so = 4 * (64 * (4 * (h >> 1) + wave) + 32 * (h & 1));
    const int vo = 16 * (lane_id() >> 5);
#pragma unroll
    for (int r = 0; r < 4; ++r) b1v[r] = __builtin_amdgcn_raw_buffer_load_b128(b1b, vo + 32 * r, so, 0);
  };
  // epilogue unit k (0 .. 7: group k / 2, k16 step j = k % 2 of the tile) of the half-round with
  // parity Q: 8 hidden units of this lane's token -> its 16-B slot of an FFN2 B fragment in H half Q.
  // A unit runs as TW_EP pieces spread over the MFMA gaps of three FFN1 steps (piece p after MFMA
  // g of step 3k + p / G): values v at piece v (TW_EP - 2) / 8 (b1, LeakyReLU, the LN_f sums: five
  // scalar VALU each), the four bf16 packs at piece TW_EP - 2, the LDS write at TW_EP - 1 — at most
  // ~5 VALU per 32x32x16 gap, which the MFMA hides; one ~40-instruction block per unit (packed f32)
  // stalled the matrix pipe for ~130 cycles after every third step.
  constexpr int TW_EP = 3 * G;
  float ex[8];                                        // the unit's values between its pieces
  uint32_t epk[4];
  auto epi_piece = [&](auto k_tag, auto q_tag, auto p_tag) {
    constexpr int k = decltype(k_tag)::value, Q = decltype(q_tag)::value, pc = decltype(p_tag)::value;
    constexpr int g = k >> 1, j = k & 1;
    if constexpr (g < G) {
      const f32x16& a = Q ? ha[g] : hv[g];
      unroll([&](auto vc) {
        constexpr int v = decltype(vc)::value;
        if constexpr (v * (TW_EP - 2) / 8 == pc) {
          // (LeakyReLU as plain code: the inline-asm form made hipcc pad an s_nop after every one)
          const float u = a[8 * j + v] + __uint_as_float(b1v[(8 * j + v) >> 2][(8 * j + v) & 3]);
          const float x = fmaxf(u, 0.1f * u);
          ex[v] = x;
          sa1[g] += x;
          sa2[g] = fmaf(x, x, sa2[g]);
        }
      }, std::make_integer_sequence<int, 8>{});
      if constexpr (pc == TW_EP - 2) {
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) epk[e2] = pack2(ex[2 * e2], ex[2 * e2 + 1]);
      }
      if constexpr (pc == TW_EP - 1)
        *reinterpret_cast<u32x4*>(smem + TW_H + Q * 32768 + ((wave * 2 + j) * 4 + g) * FRAG_BYTES + lane16) =
            u32x4{epk[0], epk[1], epk[2], epk[3]};
    }
  };
  // fragment r of an iteration (r relative to its first fragment; h = the iteration's half-round):
  // [0, 24) FFN1(h), [24, 48) FFN2(h - 1), then the next iteration's FFN1(h + 1) (LAST: FFN2(11))
  auto issue_it = [&](auto r_tag, int h, auto last_tag) {
    constexpr int r = decltype(r_tag)::value, n = r;  // iteration starts are multiples of the ring
    if constexpr (r < 24) loadW(wf[n % TW_RING], f_ffn1(h, r));
    else if constexpr (r < 48) loadW(wf[n % TW_RING], f_ffn2(h - 1, (r - 24) / 3, (r - 24) % 3));
    else if constexpr (decltype(last_tag)::value) loadW(wf[n % TW_RING], f_ffn2(h, (r - 48) / 3, (r - 48) % 3));
    else loadW(wf[n % TW_RING], f_ffn1(h + 1, r - 48));
  };
  // FFN1(h), parity P; Q0 = its first global step (the representative half-round for h >= 1);
  // EPI: with the epilogue of half-round h - 1 (unit k over steps 3k .. 3k + 2, one piece per MFMA gap)
  auto seg1 = [&](int h, auto p_tag, auto q0_tag, auto epi_tag, auto nop_tag) {
    constexpr int P = decltype(p_tag)::value, Q0 = decltype(q0_tag)::value;
    constexpr bool EPI = decltype(epi_tag)::value, NOP = decltype(nop_tag)::value;
    constexpr int F0 = tw_f0(Q0);
    unroll([&](auto ic) {
      constexpr int i = decltype(ic)::value, q = Q0 + i, n = F0 + i;
      tw_wait1<tw_wait_of(q)>(wf[n % TW_RING]);
      unroll([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (P == 0) {
          if constexpr (i == 0) mfma32_asm0<false, NOP>(hv[g], wf[n % TW_RING], bq[(i + 2) % 3][g]);
          else mfma32_asm<false, NOP>(hv[g], wf[n % TW_RING], bq[(i + 2) % 3][g]);
        } else {
          if constexpr (i == 0) mfma32_asm0<true, NOP>(ha[g], wf[n % TW_RING], bq[(i + 2) % 3][g]);
          else mfma32_asm<true, NOP>(ha[g], wf[n % TW_RING], bq[(i + 2) % 3][g]);
        }
        if constexpr (i + 2 < 24) bq[(i + 4) % 3][g] = rdB(TW_X, (i + 2) * 4 + g);
        if constexpr (g == GI) {
          if constexpr (Q0 == TW_QA) issue_a(std::integral_constant<int, n + TW_AH>{});
          else issue_it(std::integral_constant<int, i + TW_AH>{}, h, std::false_type{});
        }
        if constexpr (EPI) {                          // piece (i % 3) G + g of unit i / 3, in this gap
          epi_piece(std::integral_constant<int, i / 3>{}, std::integral_constant<int, 1 - P>{},
                    std::integral_constant<int, (i % 3) * G + g>{});
          __builtin_amdgcn_sched_barrier(0);
        }
      }, std::make_integer_sequence<int, G>{});
      if constexpr (Q0 == TW_QA && i == 16) b1_load(0);
      __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, 24>{});
    if constexpr (P == 0) tw_drain_h4<false>(hv);
    else tw_drain_h4<true>(ha);
  };
  // FFN2(h) from H half h & 1 (P = h & 1); in the loop (Q0 = representative) its iteration is h + 1;
  // LAST: the iteration of h = 10, whose lookahead loads FFN2(11); FINAL: FFN2(11) itself
  // (b1 of half-round h + 1 is loaded at step 0, for its epilogue in FFN1(h + 2))
  auto seg2 = [&](int h, auto p_tag, auto q0_tag, auto last_tag, auto final_tag, auto nop_tag) {
    constexpr int P = decltype(p_tag)::value, Q0 = decltype(q0_tag)::value;
    constexpr bool LAST = decltype(last_tag)::value, FINAL = decltype(final_tag)::value;
    constexpr bool NOP = decltype(nop_tag)::value;
    constexpr uint32_t HB = TW_H + P * 32768;
    constexpr int F0 = tw_f0(Q0);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      bq[0][g] = rdB(HB, g);
      bq[1][g] = rdB(HB, 4 + g);
    }
    unroll([&](auto uc) {
      constexpr int u = decltype(uc)::value, q = Q0 + u, n0 = F0 + 3 * u;
      tw_wait3<tw_wait_of(q)>(wf[n0 % TW_RING], wf[(n0 + 1) % TW_RING], wf[(n0 + 2) % TW_RING]);
      unroll([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        unroll([&](auto tc) {
          constexpr int t = decltype(tc)::value;
          mfma32_asm<true, NOP>(acc[t][g], wf[(n0 + t) % TW_RING], bq[u % 3][g]);
        }, std::make_integer_sequence<int, 3>{});
        if constexpr (u + 2 < 8) bq[(u + 2) % 3][g] = rdB(HB, (u + 2) * 4 + g);
        else if constexpr (!FINAL && !LAST) bq[(u + 2) % 3][g] = rdB(TW_X, (u - 6) * 4 + g);   // next FFN1 steps 0, 1
        if constexpr (g == GI) {
          if constexpr (FINAL) {
            if constexpr (n0 + TW_AH < TW_NFRAGW)
              unroll([&](auto tc) {
                constexpr int m = n0 + TW_AH + decltype(tc)::value;
                if constexpr (m < TW_NFRAGW) loadW(wf[m % TW_RING], f_ffn2(h, (m - F0) / 3, (m - F0) % 3));
              }, std::make_integer_sequence<int, 3>{});
          } else {
            unroll([&](auto tc) {
              issue_it(std::integral_constant<int, 24 + 3 * u + TW_AH + decltype(tc)::value>{}, h + 1, last_tag);
            }, std::make_integer_sequence<int, 3>{});
          }
        }
      }, std::make_integer_sequence<int, G>{});
      if constexpr (!FINAL && u == 0) b1_load(h + 1);
      __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, 8>{});
    tw_drain_o(acc);
  };
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bq[2][g] = rdB(TW_X, g);
    bq[0][g] = rdB(TW_X, 4 + g);
  }
  seg1(0, std::integral_constant<int, 0>{}, std::integral_constant<int, TW_QA>{}, std::false_type{}, TNA{});
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bq[2][g] = rdB(TW_X, g);
    bq[0][g] = rdB(TW_X, 4 + g);
  }
  using T0 = std::false_type;
  using T1 = std::true_type;
  using IQR = std::integral_constant<int, TW_QREP>;
  using IQ2 = std::integral_constant<int, TW_QREP + 24>;
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  // a barrier of the FFN (the stamped kernel: cycles parked in the FFN's barriers into stamp slot 6)
  auto ffn_barrier = [&]() {
    if constexpr (STAMP) {
      const unsigned long long t0 = __builtin_amdgcn_s_memtime();
      tw_barrier();
      st[6] += __builtin_amdgcn_s_memtime() - t0;
    } else {
      tw_barrier();
    }
  };
  // FFN1(h) with the epilogue of half-round h - 1 in its MFMA gaps (b1(h - 1) loaded at FFN2(h - 2)
  // step 0), barrier, FFN2(h - 1)
#pragma unroll 1
  for (int h = 1; h < 11; h += 2) {
    seg1(h, P1{}, IQR{}, T1{}, T0{});
    ffn_barrier();                                    // H half (h - 1) & 1 complete
    seg2(h - 1, P0{}, IQ2{}, T0{}, T0{}, T0{});
    seg1(h + 1, P0{}, IQR{}, T1{}, T0{});
    ffn_barrier();
    seg2(h, P1{}, IQ2{}, T0{}, T0{}, T0{});
  }
  seg1(11, P1{}, IQR{}, T1{}, TNT{});
  ffn_barrier();
  seg2(10, P0{}, IQ2{}, T1{}, T0{}, TNT{});
  // the epilogue of half-round 11, then its FFN2
  unroll([&](auto kc) {                            // (unit by unit: a unit's pieces share ex / epk)
    unroll([&](auto pc) { epi_piece(kc, P1{}, pc); }, std::make_integer_sequence<int, TW_EP>{});
  }, std::make_integer_sequence<int, 8>{});
  ffn_barrier();
  // H half 0 is free from here (its last reader, FFN2(10), is behind this barrier): the LN epilogue's
  // tables [b2' | c1 | g2 | be2] (6 KiB) arrive there by LDS-DMA during FFN2(11) (retired by the
  // vmcnt(0) after it, visible after the epilogue's first barrier)
  {
    const i32x4 vrs = dma_rsrc(p.vec + 4 * D, 4L * D * 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pc = wave + 4 * j;
      if (pc < 6) dma_x4(vrs, lds0 + TW_H + pc * FRAG_BYTES, lane16, pc * FRAG_BYTES);
    }
    // the projection's bias table (3 D f32 = 4.5 pieces; the last piece's upper half reads past the
    // resource: zeros) into H half 0 behind the tables and the row statistics, the same way
    if constexpr (PROJ) {
      const i32x4 prs = dma_rsrc(p.pbias, 3L * D * 4);
      dma_x4(prs, lds0 + TW_PB + wave * FRAG_BYTES, lane16, wave * FRAG_BYTES);
      if (wave == 0) dma_x4(prs, lds0 + TW_PB + 4 * FRAG_BYTES, lane16, 4 * FRAG_BYTES);
    }
  }
  seg2(11, std::integral_constant<int, 1>{}, std::integral_constant<int, TW_QF>{}, std::false_type{},
       std::true_type{}, TNF{});
  float st1[4], st2[4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    st1[g] = sa1[g];
    st2[g] = sa2[g];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the overrun loads have landed
  stamp(4);
  const __amdgpu_buffer_rsrc_t pwb =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.pw, (short)0, PROJ ? 3 * TW_FPRE * FRAG_BYTES : 0, 0x00020000);

  // ---- epilogue: out = LN2(x1 + lrelu(rstd_f (acc - mean_f c1) + b2'))
  float2* s2 = reinterpret_cast<float2*>(smem + TW_H + 8 * 1024);
  float2* s3 = reinterpret_cast<float2*>(smem + TW_H + 12 * 1024);
  // (H half 0 holds the tables, DMA'd during FFN2(11), and the statistics; FFN2(11) reads half 1)
  {
    const int l = lane_id();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      st1[g] = xsum32(st1[g]);
      st2[g] = xsum32(st2[g]);
      s2[wave * 128 + 32 * g + (l & 31)] = make_float2(st1[g], st2[g]);
    }
  }
  tw_barrier();
  float hm[4], hr[4];
  {
    const int l = lane_id();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {
        const float2 v = s2[w2 * 128 + 32 * g + (l & 31)];
        a += v.x;
        b += v.y;
      }
      hm[g] = a * (1.0f / (4 * D));
      hr[g] = 1.0f / sqrtf(fmaxf(b * (1.0f / (4 * D)) - hm[g] * hm[g], 0.f) + p.eps);
    }
  }
  const uint32_t eb = lds0 + TW_H + 64 * (lane_id() >> 5);
  {
#if TW_PACKED_LN
    // u = hr (acc - hm c1) + b2' = acc hr + (b2' - hm hr c1), in pairs (v_pk_fma_f32)
    f32x2 s2v[4], q2v[4];
#pragma unroll
    for (int g = 0; g < G; ++g) s2v[g] = q2v[g] = f32x2{0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int T = 3 * wave + t;
      float b2[16], c1[16];
      tw_ld16p(smem + (eb - lds0) + 4 * (32 * T), b2);
      tw_ld16p(smem + (eb - lds0) + 4 * (D + 32 * T), c1);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const u32x4 xa = rdB(TW_X, (2 * T) * 4 + g), xb = rdB(TW_X, (2 * T + 1) * 4 + g);
        const float nhh = -hm[g] * hr[g];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2 k = f32x2{c1[2 * e], c1[2 * e + 1]} * nhh + f32x2{b2[2 * e], b2[2 * e + 1]};
          const f32x2 u = tw_lrelu2(f32x2{acc[t][g][2 * e], acc[t][g][2 * e + 1]} * hr[g] + k);
          const f32x2 v = u + bf_pair((e < 4 ? xa : xb)[e & 3]);
          acc[t][g][2 * e] = v.x;
          acc[t][g][2 * e + 1] = v.y;
          s2v[g] += v;
          q2v[g] = v * v + q2v[g];
        }
      }
    }
    float sum[4], sq[4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sum[g] = s2v[g].x + s2v[g].y;
      sq[g] = q2v[g].x + q2v[g].y;
    }
#else
    float sum[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int T = 3 * wave + t;
      float b2[16], c1[16];
      tw_ld16p(smem + (eb - lds0) + 4 * (32 * T), b2);
      tw_ld16p(smem + (eb - lds0) + 4 * (D + 32 * T), c1);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const u32x4 xa = rdB(TW_X, (2 * T) * 4 + g), xb = rdB(TW_X, (2 * T + 1) * 4 + g);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float u = hr[g] * fmaf(-hm[g], c1[i], acc[t][g][i]) + b2[i];
          u = lrelu(u);
          const float v = u + bf_at(i < 8 ? xa : xb, i & 7);
          acc[t][g][i] = v;
          sum[g] += v;
          sq[g] = fmaf(v, v, sq[g]);
        }
      }
    }
#endif
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int g = 0; g < G; ++g) {}
    const int l = lane_id();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sum[g] = xsum32(sum[g]);
      sq[g] = xsum32(sq[g]);
      s3[wave * 128 + 32 * g + (l & 31)] = make_float2(sum[g], sq[g]);
    }
  }
  tw_barrier();
  // the projection stream's first fragments, issued here so that their latency sits under LN2's
  // normalise-and-store pass (ahead of the LN_f pass they cost that pass 36 registers: spills)
  if constexpr (PROJ) {
#pragma unroll
    for (int n = 0; n < TW_AH; ++n) pw_loadW(wf[n], pwb, lane16, wave, 3, 0, n);
  }
  {
    const int l = lane_id();
    float mean[4], rstd[4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {
        const float2 v = s3[w2 * 128 + 32 * g + (l & 31)];
        a += v.x;
        b += v.y;
      }
      mean[g] = a * (1.0f / D);
      rstd[g] = 1.0f / sqrtf(fmaxf(b * (1.0f / D) - mean[g] * mean[g], 0.f) + p.eps);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int T = 3 * wave + t;
      float g2[16], be2[16];
      tw_ld16p(smem + (eb - lds0) + 4 * (2 * D + 32 * T), g2);
      tw_ld16p(smem + (eb - lds0) + 4 * (3 * D + 32 * T), be2);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const long r = row0 + 32 * g + (l & 31);
        const float nmr = -mean[g] * rstd[g];
        float y[16];
#pragma unroll
#if TW_PACKED_LN
        for (int e = 0; e < 8; ++e) {
          const f32x2 z = (f32x2{acc[t][g][2 * e], acc[t][g][2 * e + 1]} * rstd[g] + nmr) * f32x2{g2[2 * e], g2[2 * e + 1]} +
                          f32x2{be2[2 * e], be2[2 * e + 1]};
          y[2 * e] = z.x;
          y[2 * e + 1] = z.y;
        }
#else
        for (int i = 0; i < 16; ++i) y[i] = fmaf(fmaf(acc[t][g][i], rstd[g], nmr), g2[i], be2[i]);
#endif
        if constexpr (PROJ) {
          // the same bf16 values also into the X images, x1's layout (LN1 above): this lane's cells
          // are exactly those it read as the LN2 residual (xa / xb) before the barrier above, so no
          // wave still reads what another overwrites; rows >= M as zeros, as projw_kernel reads them
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            u32x4 v{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                    pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
            if (r < p.M) *reinterpret_cast<u32x4*>(p.out + r * D + 32 * T + 16 * (l >> 5) + 8 * h2) = v;
            else v = u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(smem + TW_X + ((2 * T + h2) * 4 + g) * FRAG_BYTES + 16 * l) = v;
          }
        } else if (r < p.M) {
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2)
            *reinterpret_cast<u32x4*>(p.out + r * D + 32 * T + 16 * (l >> 5) + 8 * h2) =
                u32x4{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                      pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
        }
      }
    }
  }
  stamp(5);
  if constexpr (PROJ) {
    // ---- projection: qkv_out rows of this tile = (the X images) W_qkv^T + b_qkv, three chunks of D
    // features (the bias table: DMA'd into H during FFN2(11), visible since the epilogue's barriers)
    tw_barrier();                                     // the tile's rows complete in X
    pw_chunks<G, NOPP>(smem, lds0 + TW_PB, wave, lane16, pwb, 3, pw_out_rsrc(p.qkv_out, p.M, row0, 3), wf, acc);
    stamp(7);
  }
  if constexpr (STAMP) {
    if (lane_id() == 0 && p.stamps) {
#pragma unroll
      for (int i = 0; i < 8; ++i) p.stamps[((long)blockIdx.x * 4 + wave) * 8 + i] = st[i];
    }
  }
}

// workgroups [0, n_full): 128-row tiles; the rest: 32-row tiles after row 128 n_full (the launch's
// last partial round of 128-row tiles spread over 4x the CUs, dispatched last)
template <bool STAMP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void tailw_kernel(TwArgs p) {
  // with a projection stream: the bodies with the projection phase — a tile's rows never need a
  // second kernel, the 32-row tiles included
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p.pw) {
    if ((int)blockIdx.x < p.n_full) tailw_body<STAMP, 4, true>(p, (long)blockIdx.x * 128, wave);
    else tailw_body<STAMP, 1, true>(p, (long)p.n_full * 128 + (long)(blockIdx.x - p.n_full) * 32, wave);
    return;
  }
  if ((int)blockIdx.x < p.n_full) tailw_body<STAMP, 4, false>(p, (long)blockIdx.x * 128, wave);
  else tailw_body<STAMP, 1, false>(p, (long)p.n_full * 128 + (long)(blockIdx.x - p.n_full) * 32, wave);
}

int tailw_launch(int M, const void* att, const void* resid, void* out, const void* ws, const float* vec,
                 const float* b_o, const float* g1, const float* be1, float eps, int desync, int var,
                 const void* pw, const float* pbias, void* qkv_out, hipStream_t s) {
  // the last partial round of 128-row tiles (rem of 256 CUs) as 4 rem workgroups of 32 rows, when
  // they fit one round of 32-row tiles (option tail_split = the largest rem split; 0: off)
  const long T = cdiv(M, 128), rem = T % 256;
  const long split = options().tail_split;
  const long n_full = (T > 256 && rem > 0 && rem <= split) ? T - rem : T;
  const long nwg = n_full < T ? n_full + cdiv((long)M - n_full * 128, 32) : T;
  TwArgs a{M, (const bf16*)att, (const bf16*)resid, (bf16*)out, (const char*)ws, vec, b_o, g1, be1, eps, desync,
           diag_stamps(), (int)n_full, (const char*)pw, pbias, (bf16*)qkv_out};
  // var (option tail_wide - 1): bit 0 = phase stamps, with a snvrag_tail_stamps buffer; the other
  // bits select nothing
  auto kern = (var & 1) && a.stamps ? tailw_kernel<true> : tailw_kernel<false>;
  return SNV_LAUNCH_LDS(kern, dim3((unsigned)nwg), dim3(256), TW_LDS, s, a);
}

// ---------------------------------------------------------------------------------------------
// Wide-row projection (option proj_wide; the encoder's QKV: out[M, NC D] = x W^T + b, D = 384,
// multi_head_attention.py:44-51): the tail's phase A per output chunk of D features.  A
// workgroup owns 128 rows (x by LDS-DMA into X once), wave w owns tiles 3w .. 3w+2 of each chunk;
// per chunk 24 k16 steps x 12 MFMAs into 192 AGPR accumulators, then + bias -> bf16 -> two 16-B
// stores per (tile, token group).  W fragments (snvrag_proj_pack: chunk c, k16 step s, tile T at
// fragment c 288 + 12 s + T) through the 12-register ring 9 ahead, compiler-visible loads: the chunk
// loop is pw_chunks above, which the block tail's projection phase runs too.
struct PwArgs {
  int M, NC;
  const bf16* x;            // [M, D]
  const char* ws;           // snvrag_proj_pack stream
  const float* bias;        // [NC D]
  bf16* out;                // [M, NC D]
  int desync;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void projw_kernel(PwArgs p) {
  constexpr int D = TW_D, NT = TW_NT, KS = TW_KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long row0 = (long)blockIdx.x * 128;
  if (p.desync > 0 && blockIdx.x < 256) stagger_wait(p.desync);   // first-round stagger (mfma32.h)
  const uint32_t lds0 = lds_addr(smem);
  int lane16 = lane_id() * 16;
  asm volatile("" : "+v"(lane16));
  const i32x4 xrs = dma_rsrc(p.x + row0 * D, ((long)p.M - row0) * D * 2);     // rows >= M read as 0
  {
    const int l = lane_id();
    const int voff = (32 * wave + (l & 31)) * (D * 2) + 32 * (l >> 5);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      dma_x4(xrs, lds0 + TW_X + (s * 4 + wave) * FRAG_BYTES, voff, 64 * (s >> 1) + 16 * (s & 1));
  }
  const __amdgpu_buffer_rsrc_t wrb =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.ws, (short)0, p.NC * TW_FPRE * FRAG_BYTES, 0x00020000);
  u32x4 wf[TW_RING];
#pragma unroll
  for (int n = 0; n < TW_AH; ++n) pw_loadW(wf[n], wrb, lane16, wave, p.NC, 0, n);
  float* bs = reinterpret_cast<float*>(smem + TW_H);
  for (int i = threadIdx.x; i < p.NC * D; i += 256) bs[i] = p.bias[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the x image (LDS-DMA) landed
  tw_barrier();
  f32x16 acc[3][4];
  pw_chunks<4, false>(smem, lds0 + TW_H, wave, lane16, wrb, p.NC, pw_out_rsrc(p.out, p.M, row0, p.NC), wf, acc);
}

int projw_launch(int M, int NC, const void* x, const void* ws, const float* bias, void* out, int desync, hipStream_t s) {
  PwArgs a{M, NC, (const bf16*)x, (const char*)ws, bias, (bf16*)out, desync};
  return SNV_LAUNCH_LDS(projw_kernel, dim3((unsigned)cdiv(M, 128)), dim3(256), TW_LDS, s, a);
}

}  // namespace snvrag
