// Typed-site overlay (opt-in, --vcf_sites all): the observed genotypes of the target take the place of the
// model's output in the site-major result arrays h1 / h2 f32 [n, S] and gt f32 [n, S, 4] at the sites the target
// was genotyped at (src/typed_sites.py typed_overlay_host is the specification).
//
// The target's genotypes are bit rows (alt / miss u8 [2 S_target, ld_bits], haplotype h of sample c in row
// 2 c + h, record r at bit r & 7 of byte r >> 3: what vcf_unpack_gt_kernel reads).  For the site row i with
// r = site_row[i] in [0, n_target) and the column s with c = col[s] in [0, S_target):
//   a1, m1 = bit r of alt / miss row 2 c;  a2, m2 = bit r of row 2 c + 1;
//   m1 | m2: the cell keeps every byte it had and missing[i] counts it;
//   else h1 = a1, h2 = a2 (0.0f / 1.0f) and gt = one-hot at 2 a1 + a2 (0|0, 0|1, 1|0, 1|1: post_gt's order).
// Every other cell is untouched; missing[i] is written for every row (0 for a row that is not typed).  No float
// arithmetic: the result is exact.
//
// Layout: a transpose.  The bit rows run along records, the outputs along samples, and the outputs are 24 bytes
// per cell against 4 bits read, so the stores decide the time.  A workgroup of four waves owns a tile of 64 site
// rows x 64 columns and goes through the LDS:
//   gather  lane = site row of the tile, a wave takes 16 of the 64 columns.  The lane's byte of each of the four
//           bit rows is at r >> 3: site_row usually increases with small gaps, so the 64 lanes of a load read a
//           few adjacent bytes of one or two lines (not 64 lines, as a lane per column would); the 64 loads of
//           a lane are independent.  The 4-bit code (8: valid, 4: a call missing, 2: a1, 1: a2) of every cell
//           goes to tile[row][column], row pitch 68 bytes = 17 dwords: the byte stores of a wave fall on
//           distinct banks.
//   store   lane = column, a wave takes every fourth site row; the codes of a row are 64 consecutive bytes.
//           h1 / h2 leave as 256 contiguous bytes per wave, gt as one 16-byte store per lane (1 KiB per wave).
//           The row's missing calls are a ballot's population count, added to missing[i] by lane 0 with an
//           integer atomic (the column tiles of a row are different workgroups; an integer sum has no order).
// A tile without a typed row ends after it has read its 64 site_row entries.
#include "common.h"

namespace snvrag {

constexpr int TY_ROWS = 64, TY_COLS = 64, TY_LD = 68, TY_THREADS = 256;

__global__ __launch_bounds__(TY_THREADS) void typed_overlay_kernel(
    const uint8_t* __restrict__ alt, const uint8_t* __restrict__ miss, long ld_bits, long n_target, long S_target,
    const int32_t* __restrict__ site_row, const int32_t* __restrict__ col, long n, long S, int ctiles,
    float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ gt, int32_t* __restrict__ missing) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[TY_ROWS * TY_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rtile = blockIdx.x / ctiles;
  const long row0 = rtile * TY_ROWS, col0 = (long)(blockIdx.x - rtile * ctiles) * TY_COLS;

  // gather: lane = site row
  long r = -1;
  if (row0 + lane < n) {
    const long v = site_row[row0 + lane];
    if (v >= 0 && v < n_target) r = v;
  }
  if (__ballot(r >= 0) == 0) return;            // workgroup-uniform: every wave reads the same 64 entries
  const long byte = r < 0 ? 0 : r >> 3;
  const int bit = (int)(r & 7);
  constexpr int PER_WAVE = TY_COLS / 4;
  uint32_t code[PER_WAVE];
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const long s = col0 + wave * PER_WAVE + j;
    long c = -1;
    if (s < S) {
      const long v = col[s];                    // wave-uniform
      if (v >= 0 && v < S_target) c = v;
    }
    code[j] = 0;
    if (c >= 0 && r >= 0) {
      const long o = 2 * c * ld_bits + byte;
      const uint32_t a1 = alt[o], a2 = alt[o + ld_bits], m1 = miss[o], m2 = miss[o + ld_bits];
      code[j] = 8u | ((((m1 | m2) >> bit) & 1u) << 2) | (((a1 >> bit) & 1u) << 1) | ((a2 >> bit) & 1u);
    }
  }
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) tile[lane * TY_LD + wave * PER_WAVE + j] = (uint8_t)code[j];
  __syncthreads();

  // store: lane = column
  const long s = col0 + lane;
  for (int i = wave; i < TY_ROWS; i += 4) {
    const long site = row0 + i;
    if (site >= n) break;
    const uint32_t c = s < S ? tile[i * TY_LD + lane] : 0u;
    const uint64_t any = __ballot(c != 0);
    if (any == 0) continue;                     // the row is not typed, or none of these columns is mapped
    const bool write = (c & 12u) == 8u;
    if (write) {
      const long cell = site * S + s;
      h1[cell] = (c & 2u) ? 1.0f : 0.0f;
      h2[cell] = (c & 1u) ? 1.0f : 0.0f;
      const uint32_t k = c & 3u;
      reinterpret_cast<f32x4*>(gt)[cell] =
          f32x4{k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f, k == 3 ? 1.0f : 0.0f};
    }
    const int nmiss = __popcll(__ballot((c & 12u) == 12u));
    if (nmiss && lane == 0) atomicAdd(missing + site, nmiss);
  }
}

// the checks of snvrag_typed_overlay (reported under the entry's name)
static int typed_args(const char* where, const uint8_t* alt_bits, const uint8_t* miss_bits, int64_t ld_bits,
                      int64_t n_target, int64_t S_target, const int32_t* site_row, const int32_t* col, int64_t n,
                      int64_t S, const float* h1, const float* h2, const float* gt, const int32_t* missing) {
  SNV_CHECK_AS(where, non_null(alt_bits, miss_bits, site_row, col, h1, h2, gt, missing), "null pointer");
  SNV_CHECK_AS(where, S >= 1 && S < (1LL << 29) && S_target >= 1 && S_target < (1LL << 29),
               "S and S_target must be in [1, 2^29)");
  SNV_CHECK_AS(where, n >= 0 && n_target >= 0, "n and n_target must not be negative");
  SNV_CHECK_AS(where, ld_bits >= 0 && ld_bits < (1LL << 31) && 8 * ld_bits >= n_target,
               "ld_bits must be below 2^31 and hold n_target records");
  SNV_CHECK_AS(where, n < (1LL << 40) && n * S < (1LL << 40), "n * S must be below 2^40");
  SNV_CHECK_AS(where, aligned(16, gt), "gt must be 16-byte aligned");
  SNV_CHECK_AS(where, aligned(4, h1, h2, site_row, col, missing),
               "h1 / h2 / site_row / col / missing must be 4-byte aligned");
  return 0;
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_typed_overlay(const uint8_t* alt_bits, const uint8_t* miss_bits, int64_t ld_bits,
                                    int64_t n_target, int64_t S_target, const int32_t* site_row, const int32_t* col,
                                    int64_t n, int64_t S, float* h1, float* h2, float* gt, int32_t* missing,
                                    void* stream) {
  if (int rc = typed_args("snvrag_typed_overlay", alt_bits, miss_bits, ld_bits, n_target, S_target, site_row, col, n,
                          S, h1, h2, gt, missing))
    return rc;
  if (n == 0) return 0;
  const int64_t ctiles = (S + TY_COLS - 1) / TY_COLS, rtiles = (n + TY_ROWS - 1) / TY_ROWS;
  SNV_CHECK_ARG(ctiles * rtiles < (1LL << 31), "tiles must be below 2^31");
  hipStream_t s = as_stream(stream);
  SNV_HIP(hipMemsetAsync(missing, 0, 4 * (size_t)n, s));
  hipLaunchKernelGGL(typed_overlay_kernel, dim3((unsigned)(ctiles * rtiles)), dim3(TY_THREADS), 0, s, alt_bits,
                     miss_bits, (long)ld_bits, (long)n_target, (long)S_target, site_row, col, (long)n, (long)S,
                     (int)ctiles, h1, h2, gt, missing);
  SNV_LAUNCH_CHECK();
  return 0;
}
