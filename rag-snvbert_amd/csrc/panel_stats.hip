// Genotype counts of a reference panel per site and per population, from the haplotype-major bit rows the
// device VCF reader leaves on the GPU (VcfGenotypes.alt_bits / miss_bits).  The reference gets the same
// numbers from four per-population CSVs in prepare_data_v4_0411.py:116-231; the specification here is
// src/dataset/panel_stats.py panel_counts_host.
//
// Layout.  A lane owns one dword column of the bit rows (32 sites), a wave 64 adjacent columns (256
// contiguous bytes of every row it reads), a workgroup of PS_WAVES waves one tile of PS_COLS columns =
// PS_SITES sites.  The workgroup walks the populations in turn; inside a population its waves split the
// samples into contiguous shares.  Per sample a lane loads four dwords (ALT and missing, two haplotypes) and
// forms five one-bit classes per site:
//     both  both alleles called            het   both called, one ALT        hom   both called, two ALT
//     half  exactly one allele called      alth  that one allele is ALT
// Each class is summed in a bit-sliced counter of 8 planes: eight samples go through a carry-save tree into
// the planes 1 / 2 / 4 and one carry into the planes 8 .. 128, so a counter holds 255 and is flushed after
// at most PS_CHUNK = 248 samples.  A flush turns the planes into per-site integers four sites at a time
// (4 plane bits -> 4 bytes by one multiply) and adds them to the tile's [5][PS_SITES] integers in the LDS
// (swizzled by the lane, conflict-free).  After a barrier the workgroup writes the population's five count
// rows with coalesced stores
//     n_ref = both - het - hom   n_het = het   n_hom = hom   n_alt = het + 2 hom + alth   n_called = 2 both + half
// keeps the sum over the populations in registers, clears the LDS for the next population, and at the end
// writes the zero rows P .. 4 and the whole-panel row 5.  Every bit-row byte is read once, every count is
// written once by a plain store, and the integers do not depend on the order of the LDS adds.
//
// Rows may start at any byte (odd ld_bits): a dword column is one 4-byte load at the row's own alignment;
// the columns of a row's last, partial dword are read byte by byte, so no load leaves
// [row, row + ceil(n_sites / 8)).  Bits at and past n_sites are treated as missing calls.
#include "common.h"

namespace snvrag {

constexpr int PS_WAVES = 8, PS_THREADS = 64 * PS_WAVES;
constexpr int PS_COLS = 64, PS_SITES = 32 * PS_COLS;        // dword columns and sites per workgroup
constexpr int PS_GROUP = 8, PS_CHUNK = 31 * PS_GROUP;       // samples per carry-save tree, per flush (<= 255)
constexpr int PS_CLASSES = 5, PS_PLANES = 8;
constexpr int PS_ROWS = 6, PS_GLOBAL = 5;                   // count rows: 5 populations and the whole panel

struct PsPlanes { uint32_t p[PS_PLANES]; };

// (h, l) = carry and sum of a + b + c, bit by bit
__device__ __forceinline__ void ps_csa(uint32_t& h, uint32_t& l, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t u = a ^ b;
  h = (a & b) | (u & c);
  l = u ^ c;
}

// adds the eight one-bit-per-site values x to the counter
__device__ __forceinline__ void ps_add8(PsPlanes& P, const uint32_t (&x)[PS_GROUP]) {
  uint32_t t2a, t2b, t4a, t4b, c;
  ps_csa(t2a, P.p[0], P.p[0], x[0], x[1]);
  ps_csa(t2b, P.p[0], P.p[0], x[2], x[3]);
  ps_csa(t4a, P.p[1], P.p[1], t2a, t2b);
  ps_csa(t2a, P.p[0], P.p[0], x[4], x[5]);
  ps_csa(t2b, P.p[0], P.p[0], x[6], x[7]);
  ps_csa(t4b, P.p[1], P.p[1], t2a, t2b);
  ps_csa(c, P.p[2], P.p[2], t4a, t4b);
#pragma unroll
  for (int k = 3; k < PS_PLANES; ++k) {
    const uint32_t n = P.p[k] & c;
    P.p[k] ^= c;
    c = n;
  }
}

// the dword of column col of one bit row.  EDGE: the tile holds the row's last dword, which may be partial
// (tail bytes, read one by one) or absent
template <bool EDGE>
__device__ __forceinline__ uint32_t ps_load(const uint8_t* __restrict__ row, int col, int n_full, int tail) {
  const uint8_t* p = row + 4L * col;
  uint32_t v = 0;
  if (!EDGE || col < n_full) {
    __builtin_memcpy(&v, p, 4);
  } else if (col == n_full) {
    for (int b = 0; b < tail; ++b) v |= (uint32_t)p[b] << (8 * b);
  }
  return v;
}

// the planes of one class as integers, added to the lane's 32 sites of that class in the LDS
__device__ __forceinline__ void ps_flush(PsPlanes& P, int* __restrict__ cls, int lane) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t acc = 0;                                         // four sites, one byte each (<= 255)
#pragma unroll
    for (int k = 0; k < PS_PLANES; ++k)
      acc += ((((P.p[k] >> (4 * g)) & 15u) * 0x204081u) & 0x01010101u) << k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = (int)((acc >> (8 * j)) & 255u);
      atomicAdd(&cls[lane * 32 + ((4 * g + j + lane) & 31)], v);
    }
  }
#pragma unroll
  for (int k = 0; k < PS_PLANES; ++k) P.p[k] = 0;
}

template <bool EDGE>
__device__ __forceinline__ void ps_population(const uint8_t* __restrict__ alt, const uint8_t* __restrict__ miss,
                                              long ld_bits, int S, const int32_t* __restrict__ order, int lo,
                                              int hi, int col, int n_full, int tail, uint32_t valid,
                                              int* __restrict__ acc, int lane) {
  PsPlanes cnt[PS_CLASSES];
#pragma unroll
  for (int q = 0; q < PS_CLASSES; ++q)
#pragma unroll
    for (int k = 0; k < PS_PLANES; ++k) cnt[q].p[k] = 0;
  for (int c0 = lo; c0 < hi; c0 += PS_CHUNK) {
    const int c1 = min(hi, c0 + PS_CHUNK);
    for (int g0 = c0; g0 < c1; g0 += PS_GROUP) {
      uint32_t a0[PS_GROUP], a1[PS_GROUP], m0[PS_GROUP], m1[PS_GROUP];
#pragma unroll
      for (int i = 0; i < PS_GROUP; ++i) {
        a0[i] = a1[i] = 0;
        m0[i] = m1[i] = ~0u;                                  // no sample: both alleles missing, counts nothing
        if (g0 + i < c1) {
          const int s = order[g0 + i];
          if ((unsigned)s < (unsigned)S) {                    // a sample number outside the panel loads nothing
            const long r = 2L * s * ld_bits;
            a0[i] = ps_load<EDGE>(alt + r, col, n_full, tail);
            a1[i] = ps_load<EDGE>(alt + r + ld_bits, col, n_full, tail);
            m0[i] = ps_load<EDGE>(miss + r, col, n_full, tail);
            m1[i] = ps_load<EDGE>(miss + r + ld_bits, col, n_full, tail);
          }
        }
      }
      uint32_t x[PS_CLASSES][PS_GROUP];
#pragma unroll
      for (int i = 0; i < PS_GROUP; ++i) {
        const uint32_t k0 = EDGE ? ~m0[i] & valid : ~m0[i], k1 = EDGE ? ~m1[i] & valid : ~m1[i];   // called
        const uint32_t b0 = a0[i] & k0, b1 = a1[i] & k1;
        const uint32_t both = k0 & k1, half = k0 ^ k1;
        x[0][i] = both;
        x[1][i] = both & (b0 ^ b1);
        x[2][i] = b0 & b1;
        x[3][i] = half;
        x[4][i] = half & (b0 | b1);
      }
#pragma unroll
      for (int q = 0; q < PS_CLASSES; ++q) ps_add8(cnt[q], x[q]);
    }
#pragma unroll
    for (int q = 0; q < PS_CLASSES; ++q) ps_flush(cnt[q], acc + q * PS_SITES, lane);
  }
}

// the five count columns of one site from the tile's class sums; clears them
__device__ __forceinline__ void ps_take(int* __restrict__ acc, int site, int (&out)[5]) {
  const int l = site >> 5, at = l * 32 + ((site + l) & 31);
  int v[PS_CLASSES];
#pragma unroll
  for (int q = 0; q < PS_CLASSES; ++q) {
    v[q] = acc[q * PS_SITES + at];
    acc[q * PS_SITES + at] = 0;
  }
  out[0] = v[0] - v[1] - v[2];
  out[1] = v[1];
  out[2] = v[2];
  out[3] = v[1] + 2 * v[2] + v[4];
  out[4] = 2 * v[0] + v[3];
}

template <bool EDGE>
__device__ __forceinline__ void ps_tile(const uint8_t* __restrict__ alt, const uint8_t* __restrict__ miss,
                                        long ld_bits, int S, long n_sites, const int32_t* __restrict__ order,
                                        const int32_t* __restrict__ pop_start, int P, int32_t* __restrict__ counts,
                                        int* __restrict__ acc) {
  constexpr int PER = PS_SITES / PS_THREADS;                  // sites per lane of the write-out
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long site0 = (long)blockIdx.x * PS_SITES;
  const int col = (int)(blockIdx.x * PS_COLS + lane);
  const long nb = (n_sites + 7) >> 3;
  const int n_full = (int)(nb >> 2), tail = (int)(nb & 3);
  const long left = n_sites - 32L * col;                      // sites of this lane's column
  const uint32_t valid = left >= 32 ? ~0u : left <= 0 ? 0u : (1u << left) - 1u;
  int total[PER][5];
#pragma unroll
  for (int i = 0; i < PER; ++i)
#pragma unroll
    for (int c = 0; c < 5; ++c) total[i][c] = 0;
  for (int i = threadIdx.x; i < PS_CLASSES * PS_SITES; i += PS_THREADS) acc[i] = 0;
  __syncthreads();
  for (int p = 0; p < PS_GLOBAL; ++p) {
    if (p < P) {
      const int lo = max(pop_start[p], 0), hi = min(pop_start[p + 1], S);
      const int share = (max(hi - lo, 0) + PS_WAVES - 1) / PS_WAVES;
      const int w_lo = lo + wave * share, w_hi = min(hi, w_lo + share);
      ps_population<EDGE>(alt, miss, ld_bits, S, order, w_lo, w_hi, col, n_full, tail, valid, acc, lane);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int site = threadIdx.x + i * PS_THREADS;
      int out[5] = {0, 0, 0, 0, 0};
      if (p < P) ps_take(acc, site, out);
      if (!EDGE || site0 + site < n_sites) {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          counts[(long)(p * 5 + c) * n_sites + site0 + site] = out[c];
          total[i][c] += out[c];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int site = threadIdx.x + i * PS_THREADS;
    if (!EDGE || site0 + site < n_sites) {
#pragma unroll
      for (int c = 0; c < 5; ++c) counts[(long)(PS_GLOBAL * 5 + c) * n_sites + site0 + site] = total[i][c];
    }
  }
}

__global__ __launch_bounds__(PS_THREADS) void panel_counts_kernel(
    const uint8_t* __restrict__ alt, const uint8_t* __restrict__ miss, long ld_bits, int S, long n_sites,
    const int32_t* __restrict__ order, const int32_t* __restrict__ pop_start, int P, int32_t* __restrict__ counts) {
  __shared__ int acc[PS_CLASSES * PS_SITES];
  // whole dwords only in this tile: PS_COLS columns, all below the row's last full dword
  const bool inner = ((long)blockIdx.x + 1) * PS_COLS <= (((n_sites + 7) >> 3) >> 2) &&
                     ((long)blockIdx.x + 1) * PS_SITES <= n_sites;
  if (inner)
    ps_tile<false>(alt, miss, ld_bits, S, n_sites, order, pop_start, P, counts, acc);
  else
    ps_tile<true>(alt, miss, ld_bits, S, n_sites, order, pop_start, P, counts, acc);
}

// the checks of snvrag_panel_counts (reported under this name)
static int panel_counts_args(const uint8_t* alt_bits, const uint8_t* miss_bits, int64_t ld_bits, int64_t S,
                             int64_t n_sites, const int32_t* order, const int32_t* pop_start, int64_t P,
                             int32_t* counts) {
  SNV_CHECK_PTRS(alt_bits, miss_bits, order, pop_start, counts);
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 29), "S must be in [1, 2^29)");
  SNV_CHECK_ARG(P >= 1 && P <= PS_GLOBAL, "P must be in [1, 5]: row 5 is the whole panel");
  SNV_CHECK_ARG(n_sites >= 0 && n_sites < (1LL << 31), "n_sites must be in [0, 2^31)");
  SNV_CHECK_ARG(ld_bits >= (n_sites + 7) / 8, "ld_bits must hold n_sites sites");
  SNV_CHECK_ALIGN(4, "order, pop_start and counts must be 4-byte aligned", order, pop_start, counts);
  return 0;
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_panel_counts(const uint8_t* alt_bits, const uint8_t* miss_bits, int64_t ld_bits, int64_t S,
                                   int64_t n_sites, const int32_t* order, const int32_t* pop_start, int64_t P,
                                   int32_t* counts, void* stream) {
  if (int rc = panel_counts_args(alt_bits, miss_bits, ld_bits, S, n_sites, order, pop_start, P, counts)) return rc;
  if (n_sites == 0) return 0;
  const int64_t tiles = (n_sites + PS_SITES - 1) / PS_SITES;
  hipLaunchKernelGGL(panel_counts_kernel, dim3((unsigned)tiles), dim3(PS_THREADS), 0, as_stream(stream), alt_bits,
                     miss_bits, (long)ld_bits, (int)S, (long)n_sites, order, pop_start, (int)P, counts);
  SNV_LAUNCH_CHECK();
  return 0;
}
