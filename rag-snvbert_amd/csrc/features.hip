// Device-resident featurisation: one launch builds every tensor a batch of (sample, window)
// items hands to retrieval and to the model (reference: dataset.py TrainDataset.__getitem__ /
// InferDataset.__getitem__, vocab.py to_seq, utils.py sequence_padding; v18 overrides
// embedding_rag_dataset.py:486-555, embedding_rag_infer_dataset.py:226-248).
//
// Everything a batch is made of is static and lives in HBM (snvrag_feature_tables_t): the cohort's
// genotypes at 1 bit per (haplotype, site), the frequency table, and per window its site list
// (row in the genotype array, frequency column, normalised position) and padded mask.  A batch is
// a gather over them; the kernel does no float arithmetic, so every output is bit for bit what the
// host path computes.
//
// Write-bound: 72 B per token position with labels (48 B without) against <= 13 B read.  One wave
// per 128 positions of one batch row, two positions per lane: the i64 outputs go out as one 16-B
// store per lane and array, the f32 outputs as one 8-B store (a [B][1030] f32 row has a 4120-B
// pitch: odd rows are 8-byte aligned only).  Each lane reads its own two table entries and
// genotype bytes once into registers; no LDS, no scratch.  B = 24 launches 216 workgroups at
// L = 1030, B = 256 launches 2304.
#include "common.h"

namespace snvrag {

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int FT_THREADS = 64;
constexpr int FT_POS = 2;                       // token positions per lane
constexpr int FT_MAX_L = 1030;

struct FeatTok {
  int sos, eos, pad, mask, tok0, tok1;
};

template <typename T, typename V>
__device__ __forceinline__ void put2(T* __restrict__ p, T a, T b, bool vec, bool two) {
  if (vec) {
    V v;
    v[0] = a;
    v[1] = b;
    *reinterpret_cast<V*>(p) = v;
  } else {
    p[0] = a;
    if (two) p[1] = b;
  }
}

template <bool LABELS>
__global__ __launch_bounds__(FT_THREADS) void batch_features_kernel(snvrag_feature_tables_t T,
                                                                    const int32_t* __restrict__ rows, int B, int L,
                                                                    FeatTok tk, int64_t* __restrict__ tokens,
                                                                    int64_t* __restrict__ mask_out,
                                                                    float* __restrict__ floats,
                                                                    int64_t* __restrict__ labels) {
  const int b = blockIdx.y;
  const int t0 = (blockIdx.x * FT_THREADS + threadIdx.x) * FT_POS;
  if (t0 >= L) return;
  const int s = rows[b], w = rows[B + b], flags = rows[2 * B + b];
  if (s < 0 || s >= T.n_samples || w < 0 || w >= T.n_windows) return;   // refused on the host already
  const int off = T.win_off[w];
  const int n = min(T.win_off[w + 1] - off, L - 1);
  const long pop = T.pop_of_sample[s];
  const uint8_t* __restrict__ g1 = T.gt_bits + (long)(2 * s) * T.ld_bits;
  const uint8_t* __restrict__ g2 = g1 + T.ld_bits;
  const long fstride = (long)T.n_pop * T.n_cols;          // one frequency kind: [P][n_cols]
  const float* __restrict__ f_glob = T.freq + 3 * fstride + (long)T.global_row * T.n_cols;
  const float* __restrict__ f_pop = T.freq + pop * T.n_cols;

  int64_t tok1[FT_POS], tok2[FT_POS], mk[FT_POS], a1[FT_POS], a2[FT_POS];
  float fv[6][FT_POS];
#pragma unroll
  for (int e = 0; e < FT_POS; ++e) {
    const int t = t0 + e;
    int64_t base1 = tk.pad, base2 = tk.pad;
    a1[e] = a2[e] = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) fv[f][e] = 0.f;
    mk[e] = 0;
    if (t < L) {
      if (t == 0) {
        base1 = base2 = tk.sos;
      } else if (t <= n) {
        const int j = off + t - 1;
        const int r = T.site_row[j];
        if (r >= 0) {
          a1[e] = (g1[r >> 3] >> (r & 7)) & 1;
          a2[e] = (g2[r >> 3] >> (r & 7)) & 1;
        }
        base1 = a1[e] ? tk.tok1 : tk.tok0;
        base2 = a2[e] ? tk.tok1 : tk.tok0;
        const long c = T.freq_col[j];
        fv[0][e] = T.pos_norm[j];
        fv[1][e] = f_glob[c];
        fv[2][e] = f_pop[3 * fstride + c];
        fv[3][e] = f_pop[c];
        fv[4][e] = f_pop[fstride + c];
        fv[5][e] = f_pop[2 * fstride + c];
      } else if (t == n + 1) {
        base1 = base2 = tk.eos;
      }
      const int m = T.win_mask[(long)w * L + t];
      if (m) base1 = base2 = tk.mask;
      mk[e] = (flags & 1) ? 0 : m;
    }
    tok1[e] = base1;
    tok2[e] = base2;
  }

  // L even: every row starts on an even element, so the pair is 16-B (i64) / 8-B (f32) aligned
  const bool vec = (L & 1) == 0, two = t0 + 1 < L;
  const long BL = (long)B * L, o = (long)b * L + t0;
  put2<int64_t, i64x2>(tokens + o, tok1[0], tok1[1], vec, two);
  put2<int64_t, i64x2>(tokens + BL + o, tok2[0], tok2[1], vec, two);
  put2<int64_t, i64x2>(mask_out + o, mk[0], mk[1], vec, two);
#pragma unroll
  for (int f = 0; f < 6; ++f) put2<float, f32x2>(floats + f * BL + o, fv[f][0], fv[f][1], vec, two);
  if constexpr (LABELS) {
    put2<int64_t, i64x2>(labels + o, a1[0], a1[1], vec, two);
    put2<int64_t, i64x2>(labels + BL + o, a2[0], a2[1], vec, two);
    put2<int64_t, i64x2>(labels + 2 * BL + o, (a1[0] << 1) + a2[0], (a1[1] << 1) + a2[1], vec, two);
  }
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_batch_features(const snvrag_feature_tables_t* tables, const int32_t* rows_dev,
                                     const int32_t* rows_host, int64_t B, int32_t L, int sos, int eos, int pad,
                                     int mask, int tok0, int tok1, int64_t* tokens, int64_t* mask_out,
                                     float* floats, int64_t* labels, void* stream) {
  SNV_CHECK_PTRS(tables, rows_dev, rows_host, tokens, mask_out, floats);
  const snvrag_feature_tables_t& T = *tables;
  SNV_CHECK_ARG(T.gt_bits && T.win_off && T.site_row && T.freq_col && T.pos_norm && T.win_mask && T.freq &&
                T.pop_of_sample, "null table pointer");
  SNV_CHECK_ARG(L >= 2 && L <= FT_MAX_L, "L must be in [2, 1030]");
  SNV_CHECK_ARG(T.max_window_sites >= 0 && T.max_window_sites + 1 <= L,
                "a window has more than L - 1 sites (n + 1 > L)");
  SNV_CHECK_ARG(B >= 0 && B * (int64_t)L < (1LL << 31), "B * L must be below 2^31");
  SNV_CHECK_ARG(T.n_samples >= 1 && T.n_windows >= 1 && T.n_pop >= 1 && T.n_cols >= 1 && T.ld_bits >= 1,
                "empty tables");
  SNV_CHECK_ARG(T.global_row >= 0 && T.global_row < T.n_pop, "global_row outside the frequency table");
  SNV_CHECK_ARG(aligned(16, tokens, mask_out, labels) && aligned(8, floats),
                "outputs must be 16-byte (i64) / 8-byte (f32) aligned");
  for (int64_t b = 0; b < B; ++b) {
    SNV_CHECK_ARG(rows_host[b] >= 0 && rows_host[b] < T.n_samples, "sample index out of range");
    SNV_CHECK_ARG(rows_host[B + b] >= 0 && rows_host[B + b] < T.n_windows, "window index out of range");
  }
  if (B == 0) return 0;
  const FeatTok tk{sos, eos, pad, mask, tok0, tok1};
  const dim3 grid(cdiv(L, FT_THREADS * FT_POS), (unsigned)B), block(FT_THREADS);
  SNV_CHECK_ARG(B <= 65535, "B must be at most 65535 (grid.y)");
  if (labels)
    hipLaunchKernelGGL(batch_features_kernel<true>, grid, block, 0, as_stream(stream), T, rows_dev, (int)B, (int)L,
                       tk, tokens, mask_out, floats, labels);
  else
    hipLaunchKernelGGL(batch_features_kernel<false>, grid, block, 0, as_stream(stream), T, rows_dev, (int)B, (int)L,
                       tk, tokens, mask_out, floats, labels);
  SNV_LAUNCH_CHECK();
  return 0;
}
