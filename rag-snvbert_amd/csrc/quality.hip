// Per-site statistics of the site-major result arrays (opt-in, --vcf_info / --truth_vcf): the sums behind the
// INFO fields AF / R2 / DR2 and, against a truth genotype array, the 3 x 3 genotype table and the dosage sums
// (src/quality.py site_stats_host is the specification; estimates / accuracy turn the sums into the figures).
//
// Per sample of a site, in f32 exactly as the writer (vcf.hip) computes them:
//   gp1 = gt[1] + gt[2],  ds = fma(2, gt[3], gp1),  c = ALT count of the first maximum of gt (0, 1, 1, 2)
// then in f64:  e = ds,  f = gp1 + 4 gt[3]  (= E[dosage^2]; 4 gt[3] is exact, so f is rounded once with or
// without contraction).  Every product below is of two f32 values and therefore exact in f64: only the order
// of the additions can differ from another implementation.
//   est  [n][5]  sum h1 + h2 (two terms), sum h1^2 + h2^2 (two terms), sum e, sum e^2, sum f     (all S samples)
//   acc  [n][3]  sum e, sum e^2, sum e t         table [n][9]  table[3 t + c] += 1
// over the samples with a truth column, both truth alleles called, t = the true ALT count.
//
// Layout: one 64-lane wave per site, four sites per workgroup of 256 lanes (no LDS, no barrier).  Lane l takes
// samples l, l + 64, ...; a round covers 256 samples: the four h1 / h2 dword loads (coalesced across the wave;
// a row starts at 4 S r bytes, aligned for wider loads only when S % 4 == 0), the four 16-B gt loads and the
// four truth_col loads of a lane are issued before the first is used, the 2-byte truth pairs are gathered
// through the columns behind them.  A lane adds its samples in increasing order into 8 f64 and 9 i32 registers;
// one xor butterfly (32 .. 1) sums the lanes and lane 0 stores.  The order of every sum depends on S alone, a
// + b == b + a bit for bit makes the butterfly's result the same in every lane, and there is no float atomic:
// two launches give identical bits.
//
// An index outside [-1, n_truth) / [-1, S_truth) never reaches an address: it is treated as -1 and counted in
// bad_count (a vector atomic add) — a bad row once by its site's wave, a bad column once by the wave of site 0.
#include "common.h"

namespace snvrag {

constexpr int QS_WAVES = 4;                     // sites per workgroup
constexpr int QS_UNROLL = 4;                    // samples of a lane in flight

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool TRUTH>
__global__ __launch_bounds__(64 * QS_WAVES) void site_stats_kernel(
    long n, int S, const float* __restrict__ h1, const float* __restrict__ h2, const float* __restrict__ gt,
    const int8_t* __restrict__ truth, long n_truth, long S_truth, const int32_t* __restrict__ truth_row,
    const int32_t* __restrict__ truth_col, double* __restrict__ est, double* __restrict__ acc,
    int32_t* __restrict__ table, int32_t* __restrict__ bad_count) {
  const int lane = threadIdx.x & 63;
  const long site = (long)blockIdx.x * QS_WAVES + (threadIdx.x >> 6);
  if (site >= n) return;                        // wave-uniform
  const float* r1 = h1 + site * (long)S;
  const float* r2 = h2 + site * (long)S;
  const f32x4* rg = reinterpret_cast<const f32x4*>(gt) + site * (long)S;

  long trow = -1;                               // the site's truth row, -1: none
  int bad = 0;
  if constexpr (TRUTH) {
    const long r = truth_row[site];
    if (r >= 0 && r < n_truth) trow = r;
    else if (r != -1 && lane == 0) ++bad;
  }
  const int8_t* tr = truth + (trow < 0 ? 0 : trow) * S_truth * 2;

  double a0 = 0., a1 = 0., a2 = 0., a3 = 0., a4 = 0., b0 = 0., b1 = 0., b2 = 0.;
  int tab[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

  for (long base = 0; base < S; base += 64 * QS_UNROLL) {
    float v1[QS_UNROLL], v2[QS_UNROLL];
    f32x4 g[QS_UNROLL];
    int col[QS_UNROLL], ta[QS_UNROLL];
    bool in[QS_UNROLL];
#pragma unroll
    for (int u = 0; u < QS_UNROLL; ++u) {
      const long s = base + 64 * u + lane;
      in[u] = s < S;
      v1[u] = v2[u] = 0.f;
      g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      col[u] = -1;
      if (in[u]) {
        v1[u] = r1[s];
        v2[u] = r2[s];
        g[u] = rg[s];
        if constexpr (TRUTH) col[u] = truth_col[s];
      }
    }
    if constexpr (TRUTH) {
#pragma unroll
      for (int u = 0; u < QS_UNROLL; ++u) {
        ta[u] = -1;                             // both alleles in 16 bits, -1: not evaluated
        if (in[u]) {
          const long c = col[u];
          if (c >= 0 && c < S_truth) {
            if (trow >= 0) ta[u] = *reinterpret_cast<const uint16_t*>(tr + 2 * c);
          } else if (c != -1 && site == 0) {
            ++bad;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < QS_UNROLL; ++u) {
      if (!in[u]) continue;
      const float gp1 = __fadd_rn(g[u][1], g[u][2]);
      const float ds = __fmaf_rn(2.0f, g[u][3], gp1);       // the writer's DS
      const double e = (double)ds, d1 = (double)v1[u], d2 = (double)v2[u];
      a0 += d1;
      a0 += d2;
      a1 += d1 * d1;
      a1 += d2 * d2;
      a2 += e;
      a3 += e * e;
      a4 += (double)gp1 + 4.0 * (double)g[u][3];
      if constexpr (TRUTH) {
        const int t0 = (int)(int8_t)(ta[u] & 0xff), t1 = (int)(int8_t)((ta[u] >> 8) & 0xff);
        if (ta[u] >= 0 && t0 >= 0 && t1 >= 0) {
          int am = 0;                           // first maximum, as the writer's G
          float best = g[u][0];
#pragma unroll
          for (int k = 1; k < 4; ++k)
            if (g[u][k] > best) {
              best = g[u][k];
              am = k;
            }
          const int t = (t0 > 0) + (t1 > 0), cell = 3 * t + (am >> 1) + (am & 1);
          b0 += e;
          b1 += e * e;
          b2 += e * (double)t;
#pragma unroll
          for (int k = 0; k < 9; ++k) tab[k] += (cell == k) ? 1 : 0;
        }
      }
    }
  }

  a0 = wave_sum_f64(a0);
  a1 = wave_sum_f64(a1);
  a2 = wave_sum_f64(a2);
  a3 = wave_sum_f64(a3);
  a4 = wave_sum_f64(a4);
  if constexpr (TRUTH) {
    b0 = wave_sum_f64(b0);
    b1 = wave_sum_f64(b1);
    b2 = wave_sum_f64(b2);
#pragma unroll
    for (int k = 0; k < 9; ++k) tab[k] = wave_sum_i32(tab[k]);
    if (bad) atomicAdd(bad_count, bad);
  }
  if (lane == 0) {
    double* e = est + 5 * site;
    e[0] = a0;
    e[1] = a1;
    e[2] = a2;
    e[3] = a3;
    e[4] = a4;
    if constexpr (TRUTH) {
      double* a = acc + 3 * site;
      a[0] = b0;
      a[1] = b1;
      a[2] = b2;
#pragma unroll
      for (int k = 0; k < 9; ++k) table[9 * site + k] = tab[k];
    }
  }
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_site_stats(int64_t n, int64_t S, const float* h1, const float* h2, const float* gt,
                                 const int8_t* truth, int64_t n_truth, int64_t S_truth, const int32_t* truth_row,
                                 const int32_t* truth_col, double* est, double* acc, int32_t* table,
                                 int32_t* bad_count, void* stream) {
  SNV_CHECK_PTRS(h1, h2, gt, est);
  SNV_CHECK_ARG(n >= 1 && n < (1LL << 31), "n must be in [1, 2^31)");
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 31), "S must be in [1, 2^31)");
  SNV_CHECK_ALIGN(16, "gt must be 16-byte aligned", gt);
  SNV_CHECK_ARG(aligned(4, h1, h2) && aligned(8, est), "h1 / h2 must be 4-byte and est 8-byte aligned");
  const unsigned grid = (unsigned)cdiv(n, QS_WAVES);
  if (!truth) {
    hipLaunchKernelGGL(site_stats_kernel<false>, dim3(grid), dim3(64 * QS_WAVES), 0, as_stream(stream), (long)n, (int)S,
                       h1, h2, gt, nullptr, 0L, 0L, nullptr, nullptr, est, nullptr, nullptr, nullptr);
    SNV_LAUNCH_CHECK();
    return 0;
  }
  SNV_CHECK_ARG(truth_row && truth_col && acc && table && bad_count,
                "truth needs truth_row, truth_col, acc, table and bad_count");
  SNV_CHECK_ARG(n_truth >= 1 && S_truth >= 1 && n_truth < (1LL << 31) && S_truth < (1LL << 31),
                "n_truth and S_truth must be in [1, 2^31)");
  SNV_CHECK_ARG(aligned(2, truth) && aligned(8, acc) && aligned(4, table, truth_row, truth_col, bad_count),
                "misaligned truth, acc, table, truth_row, truth_col or bad_count");
  hipLaunchKernelGGL(site_stats_kernel<true>, dim3(grid), dim3(64 * QS_WAVES), 0, as_stream(stream), (long)n, (int)S, h1,
                     h2, gt, truth, (long)n_truth, (long)S_truth, truth_row, truth_col, est, acc, table, bad_count);
  SNV_LAUNCH_CHECK();
  return 0;
}
