// Device inflate of BGZF blocks (src/dataset/vcf_reader.py read_vcf(inflate="device"); the gzip layer under
// the reference's allel.read_vcf).  The specification of every status is src/dataset/bgzf.py
// inflate_block_host; the decoder itself is csrc/inflate_core.h, the same text a host program runs under
// AddressSanitizer.
//
//   form       one wave (a workgroup of 64 lanes) per BGZF block; blocks are independent, so a chunk of
//              some thousand blocks fills the machine.  The symbol decode is serial: all 64 lanes walk it with
//              the same values.  The lanes split the work that has width: the stored-block copy, the
//              match copy (up to 258 bytes, five steps), the CRC (64 segments, combined with x^(8n) mod P) and
//              the write-out (16 bytes per lane per step).
//   LDS        the block's whole output (64 KiB + 16) stays in the LDS until it is complete, so a match reads
//              what this wave's earlier LDS stores wrote: LDS operations of one wave execute in order, and
//              a wavefront-scope fence with a wave barrier keeps the compiler from moving them.  Nothing is
//              read back from global memory.
//              The output sits at LDS offset (text + out_off) & 15, so LDS and global 16-byte pieces line up
//              whatever out_off is.  Tables 1 404 B (canonical walk: count[16] + symbols per code), CRC table
//              1 KiB: 68 004 B per workgroup, two workgroups per CU out of 160 KiB.
//   bounds     every compressed byte is read inside [in_off, in_off + in_len) (the core reads zero bits past
//              it and answers status 6); every LDS store lies below isize <= 65536; a match source lies at or
//              behind the block's first byte; the write-out covers exactly text[out_off, out_off + isize) and
//              happens only for a block that inflated (status 0 or 9).  A block whose ranges leave comp or
//              text is answered with a status and touches nothing (the launcher refuses such a table first).
//   last '\n'  one workgroup walks the text backwards 4 KiB per step and stops at the first step that holds
//              a newline: a max-reduction over lanes and waves, no atomics.
#include "common.h"
#include "inflate_core.h"

namespace snvrag {

constexpr int IF_LANES = 64;

static_assert(INFL_OK == SNVRAG_INFL_OK && INFL_BAD_TYPE == SNVRAG_INFL_BAD_TYPE &&
              INFL_BAD_STORED == SNVRAG_INFL_BAD_STORED && INFL_BAD_LENGTHS == SNVRAG_INFL_BAD_LENGTHS &&
              INFL_BAD_SYMBOL == SNVRAG_INFL_BAD_SYMBOL && INFL_BAD_DISTANCE == SNVRAG_INFL_BAD_DISTANCE &&
              INFL_INPUT_END == SNVRAG_INFL_INPUT_END && INFL_OUTPUT_FULL == SNVRAG_INFL_OUTPUT_FULL &&
              INFL_OUTPUT_SHORT == SNVRAG_INFL_OUTPUT_SHORT && INFL_BAD_CRC == SNVRAG_INFL_BAD_CRC &&
              INFL_MAX_ISIZE == 65536, "the decoder's status codes are the public ones of snvrag.h");

// Lanes of the one wave hand bytes to each other through the LDS: the hardware executes a wave's LDS operations
// in order; the wavefront-scope fence orders them for the compiler, the wave barrier pins the schedule.
__device__ __forceinline__ void lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LdsSink {
  uint8_t* out;      // LDS, the block's byte 0
  int lane;
  __device__ __forceinline__ void put(int64_t pos, uint8_t v) {
    if (lane == 0) out[pos] = v;
  }
  __device__ __forceinline__ void stored(int64_t pos, const uint8_t* src, int n) {
    for (int i = lane; i < n; i += IF_LANES) out[pos + i] = src[i];
  }
  // sources lie in [pos - dist, pos): written by earlier LDS stores of this wave (lds_handoff on both sides)
  __device__ __forceinline__ void match(int64_t pos, int dist, int len) {
    lds_handoff();
    const uint8_t* src = out + (pos - dist);
    if (dist >= len) {
      for (int i = lane; i < len; i += IF_LANES) out[pos + i] = src[i];
    } else {
      for (int i = lane; i < len; i += IF_LANES) out[pos + i] = src[i % dist];
    }
    lds_handoff();
  }
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// table: i64 [n_blocks][4] = in_off, out_off, in_len | isize << 32, crc
__global__ __launch_bounds__(IF_LANES) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, long comp_bytes,
                                                                const int64_t* __restrict__ table,
                                                                uint8_t* __restrict__ text, long text_bytes,
                                                                int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[INFL_MAX_ISIZE + 16];
  __shared__ InflTables s_tab;
  __shared__ uint32_t s_crc[256];
  const int lane = threadIdx.x;
  const long blk = blockIdx.x;
  const int64_t in_off = table[4 * blk], out_off = table[4 * blk + 1], w2 = table[4 * blk + 2];
  const int64_t in_len = (int32_t)(uint32_t)w2, isize = (int32_t)(uint32_t)((uint64_t)w2 >> 32);
  const uint32_t want_crc = (uint32_t)table[4 * blk + 3];
  int st = INFL_OK;
  if (in_off < 0 || in_len < 0 || in_off > comp_bytes || in_len > comp_bytes - in_off) st = INFL_INPUT_END;
  else if (isize < 0 || isize > INFL_MAX_ISIZE || out_off < 0 || out_off > text_bytes || isize > text_bytes - out_off)
    st = INFL_OUTPUT_FULL;
  if (st != INFL_OK) {
    if (lane == 0) status[blk] = st;
    return;
  }
  for (int i = lane; i < 256; i += IF_LANES) s_crc[i] = infl_crc_table_entry((uint32_t)i);
  uint8_t* dst = text + out_off;
  const int sh = (int)((uintptr_t)dst & 15);
  LdsSink sink{s_out + sh, lane};
  int64_t produced;
  st = infl_block(comp + in_off, in_len, isize, s_tab, sink, &produced);
  lds_handoff();                        // the CRC table and the block's bytes, stored by other lanes, are read below
  if (st == INFL_OK) {
    const int n = (int)isize, seg = (n + IF_LANES - 1) / IF_LANES;
    const int lo = min(n, lane * seg), hi = min(n, lo + seg);
    const uint32_t r = infl_crc_raw(lane == 0 ? 0xffffffffu : 0u, sink.out + lo, hi - lo, s_crc);
    const uint32_t crc = wave_xor(infl_crc_mul(r, infl_crc_x8n(n - hi))) ^ 0xffffffffu;
    if (crc != want_crc) st = INFL_BAD_CRC;
    // write-out: bytes up to the first 16-byte boundary of text, whole pieces, the rest
    const int head = min(n, (16 - sh) & 15), pieces = (n - head) >> 4, tail0 = head + (pieces << 4);
    if (lane < head) dst[lane] = sink.out[lane];
    for (int k = lane; k < pieces; k += IF_LANES)
      *reinterpret_cast<u32x4*>(dst + head + 16 * k) = *reinterpret_cast<const u32x4*>(sink.out + head + 16 * k);
    if (tail0 + lane < n) dst[tail0 + lane] = sink.out[tail0 + lane];
  }
  if (lane == 0) status[blk] = st;
}

// bit j = byte j of the dword is '\n'
__device__ __forceinline__ uint32_t nl_mask4(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
  return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

constexpr int LN_THREADS = 256;
constexpr long LN_SPAN = (long)LN_THREADS * 16;

__global__ __launch_bounds__(LN_THREADS) void text_last_newline_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                                       int64_t* __restrict__ out) {
  __shared__ long long wmax[LN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (long s = nbytes > 0 ? (nbytes - 1) / LN_SPAN : -1; s >= 0; --s) {
    const long o = s * LN_SPAN + (long)tid * 16;
    long long best = -1;
    if (o + 16 <= nbytes) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(text + o);           // text is 16-byte aligned
      const uint32_t m = nl_mask4(v[0]) | (nl_mask4(v[1]) << 4) | (nl_mask4(v[2]) << 8) | (nl_mask4(v[3]) << 12);
      if (m) best = o + 31 - __clz((int)m);
    } else {
      for (long q = o; q < nbytes; ++q)
        if (text[q] == '\n') best = q;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const long long t = __shfl_xor(best, d, 64);
      best = t > best ? t : best;
    }
    __syncthreads();                                  // the readers of the previous step are done with wmax
    if (lane == 0) wmax[w] = best;
    __syncthreads();
    long long m = wmax[0];
#pragma unroll
    for (int i = 1; i < LN_THREADS / 64; ++i) m = wmax[i] > m ? wmax[i] : m;
    if (m >= 0) {                                     // uniform over the workgroup
      if (tid == 0) *out = m;
      return;
    }
  }
  if (tid == 0) *out = -1;
}

}  // namespace snvrag

using namespace snvrag;

extern "C" int snvrag_bgzf_inflate(const uint8_t* comp, int64_t comp_bytes, const int64_t* table_host,
                                   int64_t* table_dev, int64_t n_blocks, uint8_t* text, int64_t text_bytes,
                                   int32_t* status, void* stream) {
  SNV_CHECK_ARG(n_blocks >= 0 && n_blocks < (1LL << 31), "n_blocks must be in [0, 2^31)");
  SNV_CHECK_ARG(comp_bytes >= 0 && text_bytes >= 0, "comp_bytes and text_bytes must not be negative");
  if (n_blocks == 0) return 0;
  SNV_CHECK_PTRS(comp, table_host, table_dev, text, status);
  SNV_CHECK_ALIGN(8, "table_dev must be 8-byte aligned", table_dev);
  for (int64_t b = 0; b < n_blocks; ++b) {
    const int64_t in_off = table_host[4 * b], out_off = table_host[4 * b + 1], w2 = table_host[4 * b + 2];
    const int64_t in_len = (int32_t)(uint32_t)w2, isize = (int32_t)(uint32_t)((uint64_t)w2 >> 32);
    SNV_CHECK_ARG(in_len >= 0 && in_off >= 0 && in_off <= comp_bytes && in_len <= comp_bytes - in_off,
                  "block " + std::to_string(b) + ": the compressed range lies outside comp");
    SNV_CHECK_ARG(isize >= 0 && isize <= INFL_MAX_ISIZE, "block " + std::to_string(b) + ": isize must be in [0, 65536]");
    SNV_CHECK_ARG(out_off >= 0 && out_off <= text_bytes && isize <= text_bytes - out_off,
                  "block " + std::to_string(b) + ": the output range lies outside text");
  }
  hipStream_t s = as_stream(stream);
  SNV_HIP(hipMemcpyAsync(table_dev, table_host, (size_t)n_blocks * 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n_blocks), dim3(IF_LANES), 0, s, comp, (long)comp_bytes,
                     table_dev, text, (long)text_bytes, status);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_text_last_newline(const uint8_t* text, int64_t nbytes, int64_t* out, void* stream) {
  SNV_CHECK_PTRS(text, out);
  SNV_CHECK_ARG(nbytes >= 0 && nbytes < (1LL << 40), "nbytes must be in [0, 2^40)");
  SNV_CHECK_ARG(aligned(16, text) && aligned(8, out), "text must be 16-byte, out 8-byte aligned");
  hipLaunchKernelGGL(text_last_newline_kernel, dim3(1), dim3(LN_THREADS), 0, as_stream(stream), text, (long)nbytes, out);
  SNV_LAUNCH_CHECK();
  return 0;
}
