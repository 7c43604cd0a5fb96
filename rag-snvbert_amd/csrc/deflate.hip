// Device deflate of BGZF members (src/vcf_device.py write_vcf_device(bgzf=True), src/dataset/bgzf.py
// deflate_device; the bgzip pass over the reference writer's output).  The compressor is csrc/deflate_core.h,
// the same text a host program runs under AddressSanitizer, and the bytes are a function of the input alone.
//
//   form       one workgroup of 256 lanes per member.  The core's wide steps (hashing, match lengths, the
//              histogram, the leaf ranking, the segment bit totals, the bit packing, the CRC, the write-out)
//              run on all lanes; its serial steps (the greedy token chain, the Huffman merge, the header) on
//              lane 0 between workgroup barriers.  Every branch around a barrier is uniform: the core tests
//              only values that all lanes read from the LDS behind a barrier.
//   LDS        DeflState, 77 KiB: hash heads 16 KiB (u32, so the winner of a batch is an LDS max), match
//              records 32 KiB (DEFL_T = 8 192 positions), staging 17 KiB, tables and Huffman scratch 12 KiB;
//              two workgroups per CU out of 160 KiB.  The input is read from global memory (read-only).
//   atomics    LDS integer max / add / or / xor only: commutative, so no result depends on lane order.
//   bounds     input bytes lie in text[off, off + n); a member's writes lie in its slot below n + 31 <= 65 536
//              and, in the end, exactly in [0, member_len): the coded form is abandoned for the stored one
//              before a byte past n + 5 payload bytes is written.
//   pack       total: one workgroup sums member_len (fixed order, no atomics) and refuses a sum above
//              out_bytes or a length outside [0, 65 536] with -1.  copy: one workgroup per member sums the
//              lengths in front of it the same way and copies 16 bytes per lane per step to 16-byte aligned
//              destinations.
#include "common.h"
#include "deflate_core.h"

namespace snvrag {

constexpr int DF_THREADS = 256;
constexpr long DF_SLOT = DEFL_MAX_MEMBER;

struct DeflLanes {
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nlanes() const { return DF_THREADS; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ void amax(uint32_t* p, uint32_t v) { atomicMax(p, v); }
  __device__ __forceinline__ void aadd(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
  __device__ __forceinline__ void aor(uint32_t* p, uint32_t v) { atomicOr(p, v); }
  __device__ __forceinline__ void axor(uint32_t* p, uint32_t v) { atomicXor(p, v); }
};

__global__ __launch_bounds__(DF_THREADS) void bgzf_deflate_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                                  int block_size, uint8_t* __restrict__ members,
                                                                  int32_t* __restrict__ member_len) {
  __shared__ DeflState S;
  const long b = blockIdx.x, off = b * block_size;
  const int n = (int)(nbytes - off < block_size ? nbytes - off : block_size);     // >= 1: the grid is ceil(nbytes / block_size)
  DeflLanes ctx;
  const int len = defl_member(ctx, S, text + off, n, members + DF_SLOT * b);
  if (threadIdx.x == 0) member_len[b] = len;
}

// sum of v over the workgroup, the same in every lane; red: DF_THREADS / 64 entries.  Fixed order: no atomics.
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();                                    // the readers of the previous call are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
#pragma unroll
  for (int i = 0; i < DF_THREADS / 64; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(DF_THREADS) void bgzf_pack_total_kernel(const int32_t* __restrict__ member_len,
                                                                     long n_blocks, long out_bytes,
                                                                     int64_t* __restrict__ total) {
  __shared__ long long red[DF_THREADS / 64];
  long long sum = 0, bad = 0;
  for (long i = threadIdx.x; i < n_blocks; i += DF_THREADS) {
    const int32_t l = member_len[i];
    bad += (l < 0 || l > DEFL_MAX_MEMBER);
    sum += l;
  }
  sum = block_sum(sum, red);
  bad = block_sum(bad, red);
  if (threadIdx.x == 0) *total = (bad != 0 || sum > out_bytes) ? -1 : sum;
}

__global__ __launch_bounds__(DF_THREADS) void bgzf_pack_copy_kernel(const uint8_t* __restrict__ members,
                                                                    const int32_t* __restrict__ member_len,
                                                                    uint8_t* __restrict__ out,
                                                                    const int64_t* __restrict__ total) {
  __shared__ long long red[DF_THREADS / 64];
  if (*total < 0) return;                             // uniform: nothing is written
  const long b = blockIdx.x;
  long long off = 0;
  for (long i = threadIdx.x; i < b; i += DF_THREADS) off += member_len[i];
  off = block_sum(off, red);
  const int n = member_len[b], tid = threadIdx.x;
  const uint8_t* src = members + DF_SLOT * b;
  uint8_t* dst = out + off;
  const int head = min(n, (int)((16 - ((uintptr_t)dst & 15)) & 15)), pieces = (n - head) >> 4, tail0 = head + (pieces << 4);
  if (tid < head) dst[tid] = src[tid];
  for (int k = tid; k < pieces; k += DF_THREADS) {
    u32x4 v;                                          // the slot is 16-byte aligned; src + head is where head is 0
    __builtin_memcpy(&v, src + head + 16 * k, 16);
    *reinterpret_cast<u32x4*>(dst + head + 16 * k) = v;
  }
  if (tail0 + tid < n) dst[tail0 + tid] = src[tail0 + tid];
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_bgzf_deflate(const uint8_t* text, int64_t nbytes, int64_t block_size, uint8_t* members,
                                   int32_t* member_len, void* stream) {
  SNV_CHECK_ARG(nbytes >= 0 && nbytes < (1LL << 31), "nbytes must be in [0, 2^31)");
  SNV_CHECK_ARG(block_size >= 1 && block_size <= DEFL_MAX_IN, "block_size must be in [1, 0xff00]");
  SNV_CHECK_PTRS(text, members, member_len);
  SNV_CHECK_ARG(aligned(16, members) && aligned(4, member_len), "members must be 16-byte, member_len 4-byte aligned");
  if (nbytes == 0) return 0;
  const int64_t n_blocks = (nbytes + block_size - 1) / block_size;
  hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)n_blocks), dim3(DF_THREADS), 0, as_stream(stream), text,
                     (long)nbytes, (int)block_size, members, member_len);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_bgzf_pack(const uint8_t* members, const int32_t* member_len, int64_t n_blocks, uint8_t* out,
                                int64_t out_bytes, int64_t* total, void* stream) {
  SNV_CHECK_ARG(n_blocks >= 0 && n_blocks < (1LL << 31), "n_blocks must be in [0, 2^31)");
  SNV_CHECK_ARG(out_bytes >= 0, "out_bytes must not be negative");
  SNV_CHECK_PTRS(members, member_len, out, total);
  SNV_CHECK_ARG(aligned(16, members) && aligned(4, member_len) && aligned(8, total),
                "members must be 16-byte, member_len 4-byte, total 8-byte aligned");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(bgzf_pack_total_kernel, dim3(1), dim3(DF_THREADS), 0, s, member_len, (long)n_blocks,
                     (long)out_bytes, total);
  SNV_LAUNCH_CHECK();
  if (n_blocks == 0) return 0;
  hipLaunchKernelGGL(bgzf_pack_copy_kernel, dim3((unsigned)n_blocks), dim3(DF_THREADS), 0, s, members, member_len, out,
                     total);
  SNV_LAUNCH_CHECK();
  return 0;
}
