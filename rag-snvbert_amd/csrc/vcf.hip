// Device VCF writer: the text of imputed records formatted on the GPU (opt-in, --vcf_writer device;
// reference layout: src/dataset/utils.py:378-479 generate_vcf_efficient_optimized; the bytes are those
// of write_vcf / vcf_cells, src/infer_embedding_rag.py:97-128 of this package).
//
// A record is a host-built prefix (CHROM .. FORMAT and a tab) followed by one cell per sample,
//   G:h1,h2:gp0,gp1,gp2:ds        G = "0|0" "0|1" "1|0" "1|1"[first argmax of gt],
//   gp0 = gt[0], gp1 = gt[1] + gt[2], gp2 = gt[3], ds = gp1 + 2 gp2 (f32, as numpy computes them),
// every number '%.3f'.  For a value in [0, 9.9995) that is d.ddd: a cell is exactly 39 bytes plus its
// separator (tab; newline after the last sample), so the line body is 40 S bytes at a known offset.
//
// '%.3f' is exact: Python formats the binary value of the f32 with round-half-even (0.0625 -> 0.062,
// 0.1875 -> 0.188).  milli() does it in integers — significand m (24 bits) times 1000 < 2^34, shifted
// right by s = 150 - e with the remainder compared against half — and src/vcf_device.py milli_f32
// restates it in numpy, checked against Python's own formatting without a GPU.  A NaN, an infinity,
// a set sign bit (-0.0 too) or a value that rounds to >= 10.000 does not fit the fixed width: the
// kernel counts it in bad_count (and writes 0.000 in its place); the caller then discards the text
// and lets the host writer produce the file.
//
// Layout: one workgroup of 256 lanes formats a tile of 256 consecutive cells of one line (10 240 B).
// Lane t loads its h1 / h2 dwords (coalesced) and its gt row as one 16-B load, and puts its 40 bytes
// into the LDS at a + 40 t, where a = the tile's destination modulo 16: LDS byte x then belongs to
// output byte (destination - a) + x, a 16-byte aligned address, and the interior of the tile leaves
// as aligned 16-B LDS reads and global stores; only the <= 15 bytes before the first and after the
// last aligned piece go out as byte stores (prefix lengths make line starts arbitrarily aligned).
// The first tile of a line also copies the prefix (global to global, bytes).  72 B per cell move:
// 32 in, 40 out.
#include "common.h"

namespace snvrag {

constexpr int VCF_TILE = 256;                   // cells per workgroup = threads
constexpr int VCF_CELL = 40;                    // bytes per cell, separator included

// round-half-even(v * 1000) of a non-negative finite f32 given by its bits, or -1 when the value
// does not print as d.ddd (sign, NaN, infinity, >= 9.9995)
__device__ __forceinline__ int milli(uint32_t u) {
  const uint32_t e = (u >> 23) & 0xffu;
  if ((u >> 31) || e >= 131u) return -1;        // negative, -0.0, NaN, inf, >= 16
  const int s = 150 - (int)e;                   // value = m 2^-s;  here s in [20, 150]
  if (e == 0u || s >= 35) return 0;             // subnormal, or below 2^-11 < 0.0005
  const uint64_t P = (uint64_t)((u & 0x7fffffu) | 0x800000u) * 1000u;
  uint32_t q = (uint32_t)(P >> s);
  const uint64_t r = P & ((1ull << s) - 1), half = 1ull << (s - 1);
  q += (r > half || (r == half && (q & 1u))) ? 1u : 0u;
  return q > 9999u ? -1 : (int)q;
}

// "d.ddd" of q in [0, 9999] at p[0..4]
__device__ __forceinline__ void put_milli(uint8_t* p, int q, int& bad) {
  if (q < 0) {
    ++bad;
    q = 0;
  }
  const uint32_t v = (uint32_t)q, d0 = v / 1000u, r0 = v - d0 * 1000u, d1 = r0 / 100u, r1 = r0 - d1 * 100u,
                 d2 = r1 / 10u, d3 = r1 - d2 * 10u;
  p[0] = (uint8_t)('0' + d0);
  p[1] = '.';
  p[2] = (uint8_t)('0' + d1);
  p[3] = (uint8_t)('0' + d2);
  p[4] = (uint8_t)('0' + d3);
}

__global__ __launch_bounds__(VCF_TILE) void vcf_format_kernel(
    long n, int S, int tiles, const float* __restrict__ h1, const float* __restrict__ h2,
    const float* __restrict__ gt, const int32_t* __restrict__ rows, const int64_t* __restrict__ line_off,
    const int32_t* __restrict__ prefix_off, const uint8_t* __restrict__ prefix_blob, int prefix_bytes,
    uint8_t* __restrict__ out, int out_bytes, int32_t* __restrict__ bad_count) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[VCF_TILE * VCF_CELL + 16];
  const int tid = threadIdx.x;
  const int line = blockIdx.x / tiles, tile = blockIdx.x - line * tiles;
  const long row = rows[line];
  const int64_t lo = line_off[line], hi = line_off[line + 1];
  const int p0 = prefix_off[line], plen = prefix_off[line + 1] - p0;
  // the caller's contract, checked again where a breach would become a stray load or store: the
  // line lies inside the buffer, its length is prefix + 40 S, the row and the prefix exist
  if (row < 0 || row >= n || lo < 0 || hi > out_bytes || p0 < 0 || plen < 0 || (long)p0 + plen > prefix_bytes ||
      hi - lo != (int64_t)plen + (int64_t)VCF_CELL * S) {
    if (tile == 0 && tid == 0) atomicAdd(bad_count, 1);
    return;
  }
  if (tile == 0)
    for (int i = tid; i < plen; i += VCF_TILE) out[lo + i] = prefix_blob[p0 + i];

  const int c0 = tile * VCF_TILE, nc = min(VCF_TILE, S - c0);
  const int g0 = (int)lo + plen + c0 * VCF_CELL;         // first output byte of the tile (< 2^31)
  const int a = g0 & 15, nbytes = nc * VCF_CELL;
  int bad = 0;
  if (tid < nc) {
    const long cell = row * (long)S + c0 + tid;
    const float v1 = h1[cell], v2 = h2[cell];
    const f32x4 g = *reinterpret_cast<const f32x4*>(gt + 4 * cell);
    int am = 0;                                           // first maximum, as np.argmax
    float best = g[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (g[k] > best) {
        best = g[k];
        am = k;
      }
    const float gp1 = __fadd_rn(g[1], g[2]);
    const float ds = __fmaf_rn(2.0f, g[3], gp1);          // 2 gp2 is exact: the same bits as gp1 + 2 * gp2
    uint8_t* p = buf + a + tid * VCF_CELL;
    p[0] = (uint8_t)('0' + (am >> 1));
    p[1] = '|';
    p[2] = (uint8_t)('0' + (am & 1));
    p[3] = ':';
    put_milli(p + 4, milli(__float_as_uint(v1)), bad);
    p[9] = ',';
    put_milli(p + 10, milli(__float_as_uint(v2)), bad);
    p[15] = ':';
    put_milli(p + 16, milli(__float_as_uint(g[0])), bad);
    p[21] = ',';
    put_milli(p + 22, milli(__float_as_uint(gp1)), bad);
    p[27] = ',';
    put_milli(p + 28, milli(__float_as_uint(g[3])), bad);
    p[33] = ':';
    put_milli(p + 34, milli(__float_as_uint(ds)), bad);
    p[39] = (c0 + tid == S - 1) ? '\n' : '\t';
  }
  if (bad) atomicAdd(bad_count, bad);
  __syncthreads();

  // LDS byte x <-> out[gb + x], gb a multiple of 16; the tile owns x in [a, a + nbytes)
  const int gb = g0 - a, x0 = min((a + 15) & ~15, a + nbytes), x1 = max((a + nbytes) & ~15, x0);
  for (int x = x0 + 16 * tid; x < x1; x += 16 * VCF_TILE)
    *reinterpret_cast<u32x4*>(out + gb + x) = *reinterpret_cast<const u32x4*>(buf + x);
  if (tid < x0 - a) out[g0 + tid] = buf[a + tid];
  if (tid < a + nbytes - x1) out[gb + x1 + tid] = buf[x1 + tid];
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_vcf_format(int64_t n, int64_t S, const float* h1, const float* h2, const float* gt,
                                 int64_t n_lines, const int32_t* rows, const int64_t* line_off,
                                 const int32_t* prefix_off, const uint8_t* prefix_blob, int64_t prefix_bytes,
                                 uint8_t* out, int64_t out_bytes, int32_t* bad_count, void* stream) {
  SNV_CHECK_PTRS(h1, h2, gt, rows, line_off, prefix_off, prefix_blob, out, bad_count);
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 31) / VCF_CELL, "S must be in [1, 2^31 / 40)");
  SNV_CHECK_ARG(n >= 1 && n < (1LL << 31), "n must be in [1, 2^31)");
  SNV_CHECK_ARG(n_lines >= 0, "n_lines must not be negative");
  SNV_CHECK_ARG(out_bytes >= 0 && out_bytes < (1LL << 31), "chunk bytes must be below 2^31");
  SNV_CHECK_ARG(prefix_bytes >= 0 && prefix_bytes < (1LL << 31), "prefix bytes must be below 2^31");
  SNV_CHECK_ALIGN(16, "out and gt must be 16-byte aligned", out, gt);
  SNV_CHECK_ALIGN(4, "h1 and h2 must be 4-byte aligned", h1, h2);
  // every line holds at least 40 S bytes of the chunk: more lines than that cannot be monotone offsets
  SNV_CHECK_ARG(n_lines <= out_bytes / (VCF_CELL * S), "n_lines lines of 40 S bytes exceed the chunk");
  if (n_lines == 0) return 0;
  const int64_t tiles = cdiv(S, VCF_TILE);
  SNV_CHECK_ARG(n_lines * tiles < (1LL << 31), "n_lines * tiles must be below 2^31");
  hipLaunchKernelGGL(vcf_format_kernel, dim3((unsigned)(n_lines * tiles)), dim3(VCF_TILE), 0, as_stream(stream),
                     (long)n, (int)S, (int)tiles, h1, h2, gt, rows, line_off, prefix_off, prefix_blob,
                     (int)prefix_bytes, out, (int)out_bytes, bad_count);
  SNV_LAUNCH_CHECK();
  return 0;
}
