// Device VCF reader: the genotypes of a VCF body parsed on the GPU into haplotype-major bit rows
// (reference: allel.read_vcf(fields=['variants/POS', 'calldata/GT']) as src/dataset/embedding_rag_dataset.py
// :463-484 and embedding_rag_infer_dataset.py:56-69 call it; the specification of every flag and code
// below is src/dataset/vcf_reader.py parse_vcf_host).
//
// A text chunk starts at a line start, holds nbytes bytes and is padded by the caller with '\n' up to a
// multiple of 16 bytes; text is 16-byte aligned.  No kernel reads at or past the padded end: the 16-byte
// pieces of the line index lie inside it, every other load is guarded by nbytes and reads '\n' beyond it.
//
//   line index   16 bytes per lane per step; compare with '\n' -> 16-bit mask; a line starts where the
//                byte before is '\n' (or the chunk start) and the line is not empty ("\n" or "\r\n"), so
//                zero-length lines vanish.  Count per workgroup, exclusive scan of the counts by one
//                workgroup, second pass writes the offsets at base + rank: sorted by construction.
//   parse        per record: POS, flags; per cell: one code byte (bit 0 / 1 ALT on haplotype 1 / 2,
//                bit 2 / 3 missing, bit 4 the separator was '/').  Every workgroup first walks the line's
//                prefix 64 bytes per step (ballot of the tab compares, running popcount) to the ninth tab.
//                Fixed-width path: the rest of the line is exactly 4 S - 1 bytes of [0-9.][|/][0-9.] cells,
//                cell s at cell0 + 4 s; a workgroup checks and decodes a tile of 1024 cells, four per lane.
//                A tile that fails marks the line, and the general path redoes the whole line: one wave
//                walks it 64 bytes per step, numbers the cells by the running popcount of the tab ballot,
//                and the lane behind a tab decodes that cell's first ':'-delimited subfield.
//                The general kernel also folds the OR of each fixed line's codes into flags bits 8..12.
//   pack rows    tile = 64 records x 64 samples staged through the LDS (row stride 68 B: conflict-free
//                byte reads); lane = record, so a ballot of one code bit is the 64 site bits of one
//                (sample, haplotype): lane 4 j + b keeps the ballot of sample j, bit b, and all 64 lanes
//                store 8 bytes each in one instruction.
//   gather bits  a window's PanelIndex rows for an arbitrary site list, straight from the bit rows.
//   unpack gt    int8 [n, S, 2] (0 / 1, -1 missing) of the bit rows, for VcfGenotypes.gt().
//   site columns CHROM, ID, REF, ALT (opt-in, read_vcf(columns=True); specification site_columns_host): one wave
//                per line walks to the fifth tab and writes four (start, length) spans; after an exclusive scan
//                of the lengths (the caller's) a lane per string copies up to 16 bytes into the packed blob,
//                and the longer strings of a wave are copied by the whole wave, 64 bytes per step.
#include "common.h"

namespace snvrag {

constexpr int LI_THREADS = 256, LI_STEPS = 4;
constexpr long LI_SPAN = (long)LI_THREADS * 16 * LI_STEPS;      // text bytes per workgroup of the line index
constexpr int FX_THREADS = 256, FX_CELLS = 4, FX_TILE = FX_THREADS * FX_CELLS;   // fixed path: cells per workgroup
constexpr int PK_THREADS = 256, PK_REC = 64, PK_SMP = 64, PK_LD = 68;
constexpr uint32_t FLAG_FORMAT = 1u, FLAG_COUNT = 2u, FLAG_PLOIDY = 4u, FLAG_POS = 8u, FLAG_BYTE = 16u,
                   FLAG_OFFSET = 1u << 31;

__device__ __forceinline__ uint8_t text_at(const uint8_t* __restrict__ text, long nbytes, long q) {
  return q < nbytes ? text[q] : (uint8_t)'\n';
}

// exclusive scan of v over the workgroup (256 lanes) and its total; wsum: 4 ints of LDS
__device__ __forceinline__ int block_exscan(int v, int& total, int* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                               // the readers of the previous call are done with wsum
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int pre = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < LI_THREADS / 64; ++i) {
    const int s = wsum[i];
    pre += i < w ? s : 0;
    total += s;
  }
  return pre + inc - v;
}

// bit j = byte j of the dword equals C (exact per byte: no borrow between bytes)
template <uint32_t C> __device__ __forceinline__ uint32_t eq_mask4(uint32_t w) {
  const uint32_t x = w ^ (C * 0x01010101u);
  const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);     // 0x80 in each zero byte
  return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// line starts among the 16 bytes at offset o (a multiple of 16 inside the padded chunk), as a 16-bit mask:
// the byte in front is '\n' (or the chunk starts) and the line is neither "\n" nor "\r\n"
__device__ __forceinline__ uint32_t line_starts16(const uint8_t* __restrict__ text, long nbytes, long o) {
  if (o >= nbytes) return 0u;
  const u32x4 v = *reinterpret_cast<const u32x4*>(text + o);
  const uint32_t nl = eq_mask4<'\n'>(v[0]) | (eq_mask4<'\n'>(v[1]) << 4) | (eq_mask4<'\n'>(v[2]) << 8) |
                      (eq_mask4<'\n'>(v[3]) << 12);
  const uint32_t cr = eq_mask4<'\r'>(v[0]) | (eq_mask4<'\r'>(v[1]) << 4) | (eq_mask4<'\r'>(v[2]) << 8) |
                      (eq_mask4<'\r'>(v[3]) << 12);
  const uint32_t prev = o == 0 ? 1u : (text[o - 1] == '\n' ? 1u : 0u);
  const uint32_t next = text_at(text, nbytes, o + 16) == '\n' ? 1u : 0u;
  const uint32_t blank = nl | (cr & ((nl >> 1) | (next << 15)));      // "\n", or the "\r" of a "\r\n"
  uint32_t st = ((nl << 1) | prev) & ~blank & 0xffffu;
  if (o + 16 > nbytes) st &= (1u << (int)(nbytes - o)) - 1u;       // whatever the padding holds
  return st;
}

__global__ __launch_bounds__(LI_THREADS) void vcf_line_count_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                                     int32_t* __restrict__ counts) {
  __shared__ int wsum[LI_THREADS / 64];
  const long b0 = (long)blockIdx.x * LI_SPAN;
  int c = 0;
#pragma unroll
  for (int st = 0; st < LI_STEPS; ++st)
    c += __popc(line_starts16(text, nbytes, b0 + ((long)st * LI_THREADS + threadIdx.x) * 16));
  int total;
  block_exscan(c, total, wsum);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(LI_THREADS) void vcf_line_scan_kernel(const int32_t* __restrict__ counts, int nb,
                                                                    int64_t* __restrict__ base, long nbytes,
                                                                    long max_lines, int64_t* __restrict__ line_off,
                                                                    int64_t* __restrict__ n_lines_out) {
  __shared__ int wsum[LI_THREADS / 64];
  int64_t carry = 0;
  for (int i0 = 0; i0 < nb; i0 += LI_THREADS) {
    const int i = i0 + threadIdx.x;
    const int v = i < nb ? counts[i] : 0;
    int total;
    const int ex = block_exscan(v, total, wsum);
    if (i < nb) base[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *n_lines_out = carry;
    line_off[carry < max_lines ? carry : max_lines] = nbytes;
  }
}

__global__ __launch_bounds__(LI_THREADS) void vcf_line_write_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                                     const int64_t* __restrict__ base, long max_lines,
                                                                     int64_t* __restrict__ line_off) {
  __shared__ int wsum[LI_THREADS / 64];
  const long b0 = (long)blockIdx.x * LI_SPAN;
  int64_t rank0 = base[blockIdx.x];
  for (int st = 0; st < LI_STEPS; ++st) {
    const long o = b0 + ((long)st * LI_THREADS + threadIdx.x) * 16;
    uint32_t m = line_starts16(text, nbytes, o);
    int total;
    int64_t r = rank0 + block_exscan(__popc(m), total, wsum);
    while (m) {
      const int j = __ffs(m) - 1;
      m &= m - 1;
      if (r < max_lines) line_off[r] = o + j;
      ++r;
    }
    rank0 += total;
  }
}

// ---------------------------------------------------------------------------------------------- parse --
struct Prefix {
  long t1, t2, t8, t9, nl;      // positions of tabs 1, 2, 8, 9 and of the newline (-1: not met)
  int ntabs;                    // tabs met before the walk stopped (at the ninth tab's step or the newline)
};

__device__ __forceinline__ int nth_bit(uint64_t m, int n) {
  for (int i = 0; i < n; ++i) m &= m - 1;
  return __ffsll((unsigned long long)m) - 1;
}

// One whole wave walks the line at lo to its ninth tab (or its end), 64 bytes per step.  Wave-uniform.
__device__ __forceinline__ Prefix walk_prefix(const uint8_t* __restrict__ text, long nbytes, long lo) {
  const int lane = threadIdx.x & 63;
  Prefix P{-1, -1, -1, -1, -1, 0};
  for (long p = lo;; p += 64) {
    const uint8_t c = text_at(text, nbytes, p + lane);
    uint64_t tm = __ballot(c == '\t');
    const uint64_t nm = __ballot(c == '\n');
    if (nm) tm &= (nm & (0 - nm)) - 1;                       // tabs in front of the newline only
    const int k = __popcll(tm), n0 = P.ntabs;
    if (n0 < 1 && n0 + k >= 1) P.t1 = p + nth_bit(tm, 0 - n0);
    if (n0 < 2 && n0 + k >= 2) P.t2 = p + nth_bit(tm, 1 - n0);
    if (n0 < 8 && n0 + k >= 8) P.t8 = p + nth_bit(tm, 7 - n0);
    if (n0 < 9 && n0 + k >= 9) P.t9 = p + nth_bit(tm, 8 - n0);
    P.ntabs = n0 + k;
    if (P.ntabs >= 9) break;
    if (nm) {
      P.nl = p + (__ffsll((unsigned long long)nm) - 1);
      break;
    }
  }
  return P;
}

// POS and the record-level flags (FORMAT, POS) of a walked line.  Wave-uniform; every load lies in front
// of the ninth tab or of the line's newline.
__device__ __forceinline__ uint32_t line_fields(const uint8_t* __restrict__ text, long nbytes, long lo,
                                                const Prefix& P, int32_t& pos) {
  long end = -1;                                              // the line end without a trailing '\r'
  if (P.nl >= 0) end = (P.nl > lo && text_at(text, nbytes, P.nl - 1) == '\r') ? P.nl - 1 : P.nl;
  uint32_t fl = 0;
  pos = 0;
  bool pos_ok = P.t1 >= 0;
  if (pos_ok) {
    const long a = P.t1 + 1, b = P.t2 >= 0 ? P.t2 : end;
    pos_ok = b - a >= 1 && b - a <= 10;
    uint64_t v = 0;
    if (pos_ok)
      for (long q = a; q < b; ++q) {
        const uint8_t c = text_at(text, nbytes, q);
        pos_ok = pos_ok && c >= '0' && c <= '9';
        v = v * 10 + (uint64_t)(c - '0');
      }
    pos_ok = pos_ok && v < (1ull << 31);
    if (pos_ok) pos = (int32_t)v;
  }
  if (!pos_ok) fl |= FLAG_POS;
  bool fmt_ok = P.t8 >= 0;
  if (fmt_ok) {
    const long a = P.t8 + 1, b = P.t9 >= 0 ? P.t9 : end;
    fmt_ok = b - a >= 2 && text_at(text, nbytes, a) == 'G' && text_at(text, nbytes, a + 1) == 'T' &&
             (b - a == 2 || text_at(text, nbytes, a + 2) == ':');
  }
  if (!fmt_ok) fl |= FLAG_FORMAT;
  return fl;
}

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - (uint32_t)'0' <= 9u; }

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// The code of the cell whose first byte is at q: its first ':'-delimited subfield, allele (sep allele)*
// with allele = digits or '.', ended by ':', a tab, the newline or the "\r\n" of the line end.
__device__ __forceinline__ uint32_t decode_cell(const uint8_t* __restrict__ text, long nbytes, long q, uint32_t& fl) {
  int n = 0, state = 0;                // alleles begun; 0 an allele must begin, 1 inside digits, 2 behind '.'
  uint32_t code = 0;
  bool bad = false;
  for (;; ++q) {
    const uint8_t c = text_at(text, nbytes, q);
    if (c == '\n' || c == ':' || c == '\t') break;
    if (c == '\r' && text_at(text, nbytes, q + 1) == '\n') break;
    if (is_digit(c)) {
      if (state == 0) {
        ++n;
        state = 1;
      } else if (state == 2) {
        bad = true;
      }
      if (c != '0' && n <= 2) code |= 1u << (n - 1);
    } else if (c == '.') {
      if (state == 0) {
        ++n;
        state = 2;
        if (n <= 2) code |= 4u << (n - 1);
      } else {
        bad = true;
      }
    } else if (c == '|' || c == '/') {
      if (state == 0) bad = true;
      state = 0;
      if (n == 1 && c == '/') code |= 16u;
    } else {
      bad = true;
    }
  }
  if (state == 0) bad = true;          // an empty subfield, or one that ends in a separator
  if (n == 1) code |= 8u;              // haploid: the second allele is absent
  if (n > 2) fl |= FLAG_PLOIDY;
  if (bad) fl |= FLAG_BYTE;
  return code;
}

__global__ __launch_bounds__(FX_THREADS) void vcf_parse_fixed_kernel(
    const uint8_t* __restrict__ text, long nbytes, const int64_t* __restrict__ line_off, int S, int tiles,
    uint8_t* __restrict__ redo, uint8_t* __restrict__ tile_or, int32_t* __restrict__ pos,
    uint32_t* __restrict__ flags, uint8_t* __restrict__ codes, long ld_codes) {
  __shared__ long s_cell0;
  __shared__ uint32_t s_or[FX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long line = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - line * tiles);
  const long lo = line_off[line];
  if (lo < 0 || lo >= nbytes) {                               // the general path reports it
    if (tid == 0) redo[line] = 1;
    return;
  }
  if (wave == 0) {
    const Prefix P = walk_prefix(text, nbytes, lo);
    if (lane == 0) s_cell0 = P.ntabs >= 9 ? P.t9 + 1 : -1;
    if (tile == 0 && P.ntabs >= 9) {
      int32_t p;
      const uint32_t fl = line_fields(text, nbytes, lo, P, p);
      if (lane == 0) {
        pos[line] = p;
        flags[line] = fl;
      }
    }
  }
  __syncthreads();
  const long cell0 = s_cell0, end = cell0 + 4L * S;            // the line's terminator sits at end - 1
  bool fixed = cell0 >= 0 && end <= nbytes;
  if (fixed) {
    const uint8_t z = text[end - 1];
    fixed = z == '\n' || (z == '\r' && end < nbytes && text[end] == '\n');
  }
  if (!fixed) {
    if (tid == 0) redo[line] = 1;
    return;
  }
  bool ok = true;
  uint32_t orc = 0;
  const int s0 = tile * FX_TILE + tid * FX_CELLS;
  if (s0 < S) {
    const int nc = min(FX_CELLS, S - s0);
    const uint8_t* p = text + cell0 + 4L * s0;                 // cells s0 .. s0 + nc - 1: bytes below end
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < FX_CELLS; ++i)
      if (i < nc) {
        uint32_t w;
        __builtin_memcpy(&w, p + 4 * i, 4);
        const uint32_t b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
        const bool d0 = is_digit(b0), p0 = b0 == '.', d2 = is_digit(b2), p2 = b2 == '.';
        ok = ok && (d0 || p0) && (b1 == '|' || b1 == '/') && (d2 || p2) && (s0 + i == S - 1 || b3 == '\t');
        const uint32_t code = ((d0 && b0 != '0') ? 1u : 0u) | ((d2 && b2 != '0') ? 2u : 0u) | (p0 ? 4u : 0u) |
                              (p2 ? 8u : 0u) | (b1 == '/' ? 16u : 0u);
        out |= code << (8 * i);
        orc |= code;
      }
    uint8_t* dst = codes + line * ld_codes + s0;
    if (nc == FX_CELLS) {
      *reinterpret_cast<uint32_t*>(dst) = out;                 // ld_codes, s0 multiples of 4
    } else {
      for (int i = 0; i < nc; ++i) dst[i] = (uint8_t)(out >> (8 * i));
    }
  }
  orc = wave_or(orc);
  if (lane == 0) s_or[wave] = orc;
  const int all_ok = __syncthreads_and(ok ? 1 : 0);
  if (tid == 0) {
    tile_or[line * tiles + tile] = (uint8_t)(s_or[0] | s_or[1] | s_or[2] | s_or[3]);
    if (!all_ok) redo[line] = 1;
  }
}

// one wave per line, four lines per workgroup
__global__ __launch_bounds__(256) void vcf_parse_general_kernel(
    const uint8_t* __restrict__ text, long nbytes, const int64_t* __restrict__ line_off, long n_lines, int S,
    int tiles, const uint8_t* __restrict__ redo, const uint8_t* __restrict__ tile_or, int32_t* __restrict__ pos,
    uint32_t* __restrict__ flags, uint8_t* __restrict__ codes, long ld_codes) {
  const int lane = threadIdx.x & 63;
  const long line = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= n_lines) return;
  if (!redo[line]) {                                          // parsed by the fixed path: fold its tiles' code bits
    uint32_t o = 0;
    for (int t = lane; t < tiles; t += 64) o |= tile_or[line * tiles + t];
    o = wave_or(o);
    if (lane == 0) flags[line] |= o << 8;
    return;
  }
  const long lo = line_off[line];
  if (lo < 0 || lo >= nbytes) {
    if (lane == 0) {
      pos[line] = 0;
      flags[line] = FLAG_OFFSET;
    }
    return;
  }
  const Prefix P = walk_prefix(text, nbytes, lo);
  int32_t pv;
  uint32_t fl = line_fields(text, nbytes, lo, P, pv), orc = 0;
  int count = 0;
  if (P.ntabs >= 9) {
    uint64_t carry = 1;                                       // the byte in front of cell0 is the ninth tab
    for (long p = P.t9 + 1;; p += 64) {
      const long q = p + lane;
      const uint8_t c = text_at(text, nbytes, q);
      const uint64_t tm = __ballot(c == '\t'), nm = __ballot(c == '\n');
      const uint64_t valid = nm ? (((nm & (0 - nm)) << 1) - 1) : ~0ull;   // up to and including the newline
      const uint64_t st = ((tm << 1) | carry) & valid;
      carry = tm >> 63;
      if ((st >> lane) & 1ull) {
        const int s = count + __popcll(st & ((1ull << lane) - 1));
        const uint32_t code = decode_cell(text, nbytes, q, fl);
        if (s < S) codes[line * ld_codes + s] = (uint8_t)code;
        orc |= code;
      }
      count += __popcll(st);
      if (nm) break;
    }
  }
  fl = wave_or(fl);
  orc = wave_or(orc);
  if (count != S) fl |= FLAG_COUNT;
  if (lane == 0) {
    pos[line] = pv;
    flags[line] = fl | (orc << 8);
  }
}

// ------------------------------------------------------------------------------------------ pack rows --
__global__ __launch_bounds__(PK_THREADS) void vcf_pack_rows_kernel(
    const uint8_t* __restrict__ codes, long ld_codes, long n_lines, int S, int stiles, uint8_t* __restrict__ alt,
    uint8_t* __restrict__ miss, long ld_bits, long byte0) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[PK_REC * PK_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long rtile = blockIdx.x / stiles;
  const int stile = (int)(blockIdx.x - rtile * stiles);
  const long rec0 = rtile * PK_REC;
  const int nrec = (int)min((long)PK_REC, n_lines - rec0), s_base = stile * PK_SMP;
  for (int i = tid; i < PK_REC * (PK_SMP / 4); i += PK_THREADS) {
    const int r = i >> 4, c = (i & 15) * 4, s = s_base + c;
    uint32_t w = 0;
    if (r < nrec) {
      const uint8_t* src = codes + (rec0 + r) * ld_codes + s;
      if (s + 3 < S) {
        w = *reinterpret_cast<const uint32_t*>(src);           // ld_codes, s multiples of 4
      } else {
        for (int b = 0; b < 4; ++b)
          if (s + b < S) w |= (uint32_t)src[b] << (8 * b);
      }
    }
    *reinterpret_cast<uint32_t*>(tile + r * PK_LD + c) = w;
  }
  __syncthreads();
  uint64_t mine = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t c = tile[lane * PK_LD + wave * 16 + j];    // lane = record
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint64_t m = __ballot((c >> b) & 1u);
      if (lane == 4 * j + b) mine = m;
    }
  }
  const int s = s_base + wave * 16 + (lane >> 2), b = lane & 3;
  if (s < S) {
    uint8_t* dst = ((b & 2) ? miss : alt) + (2L * s + (b & 1)) * ld_bits + byte0 + rtile * 8;
    if (nrec == PK_REC) {
      *reinterpret_cast<uint64_t*>(dst) = mine;                // ld_bits, byte0 multiples of 8
    } else {
      for (int i = 0; i < (nrec + 7) / 8; ++i) dst[i] = (uint8_t)(mine >> (8 * i));   // records >= nrec: 0 bits
    }
  }
}

// ---------------------------------------------------------------------------------------- gather bits --
__global__ __launch_bounds__(256) void panel_gather_bits_kernel(
    const uint8_t* __restrict__ bits, long N, long ld_bits, long n_src, const int32_t* __restrict__ site_idx,
    int n, long out_ld, int packed, uint8_t* __restrict__ out) {
  const long total = N * out_ld;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long r = g / out_ld;
    const int j = (int)(g - r * out_ld);
    const uint8_t* row = bits + r * ld_bits;
    uint32_t v = 0;
    if (packed) {
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int k = 8 * j + b;
        const long si = k < n ? (long)site_idx[k] : -1;
        if (si >= 0 && si < n_src) v |= ((row[si >> 3] >> (si & 7)) & 1u) << b;
      }
    } else {
      const long si = j < n ? (long)site_idx[j] : -1;
      if (si >= 0 && si < n_src) v = (row[si >> 3] >> (si & 7)) & 1u;
    }
    out[g] = (uint8_t)v;
  }
}

// ------------------------------------------------------------------------------------------ unpack gt --
__global__ __launch_bounds__(256) void vcf_unpack_gt_kernel(const uint8_t* __restrict__ alt,
                                                            const uint8_t* __restrict__ miss, long ld_bits, int S,
                                                            long n_sites, int sblocks, int8_t* __restrict__ gt) {
  const long rb = blockIdx.x / sblocks;
  const int s = (int)(blockIdx.x - rb * sblocks) * 256 + threadIdx.x;
  if (s >= S) return;
  const long r0 = rb * 8;
  const uint32_t a1 = alt[(2L * s) * ld_bits + rb], a2 = alt[(2L * s + 1) * ld_bits + rb];
  const uint32_t m1 = miss[(2L * s) * ld_bits + rb], m2 = miss[(2L * s + 1) * ld_bits + rb];
  const int nr = (int)min(8L, n_sites - r0);
  for (int i = 0; i < nr; ++i) {
    const uint32_t v1 = ((m1 >> i) & 1u) ? 0xffu : ((a1 >> i) & 1u), v2 = ((m2 >> i) & 1u) ? 0xffu : ((a2 >> i) & 1u);
    *reinterpret_cast<uint16_t*>(gt + ((r0 + i) * S + s) * 2) = (uint16_t)(v1 | (v2 << 8));
  }
}

// ------------------------------------------------------------------------------------- site columns --
// CHROM, ID, REF and ALT (columns 1, 3, 4, 5) of every line as (start, length) in the chunk's text: spans
// i32 [n_lines][8].  One wave per line, four lines per workgroup; the walk is walk_prefix stopped at the
// fifth tab.  A column runs from behind the tab in front of it to the next tab, or to the line's end without
// its '\r'; a column the line does not reach is (line end, 0).  A line offset outside the chunk gives zeros.
__global__ __launch_bounds__(256) void vcf_cols_span_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                            const int64_t* __restrict__ line_off, long n_lines,
                                                            int32_t* __restrict__ spans) {
  const int lane = threadIdx.x & 63;
  const long line = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= n_lines) return;
  const long lo = line_off[line];
  if (lo < 0 || lo >= nbytes) {
    if (lane < 8) spans[line * 8 + lane] = 0;
    return;
  }
  long t[5] = {-1, -1, -1, -1, -1}, nl = -1;                   // tabs 1 .. 5 and the newline (-1: not met)
  int ntabs = 0;
  for (long p = lo;; p += 64) {
    const uint8_t c = text_at(text, nbytes, p + lane);
    uint64_t tm = __ballot(c == '\t');
    const uint64_t nm = __ballot(c == '\n');
    if (nm) tm &= (nm & (0 - nm)) - 1;                         // tabs in front of the newline only
    const int k = __popcll(tm), n0 = ntabs;
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if (n0 <= i && n0 + k > i) t[i] = p + nth_bit(tm, i - n0);
    ntabs = n0 + k;
    if (ntabs >= 5) break;
    if (nm) {
      nl = p + (__ffsll((unsigned long long)nm) - 1);
      break;
    }
  }
  long end = -1;                                               // met only when the fifth tab was not
  if (nl >= 0) end = (nl > lo && text_at(text, nbytes, nl - 1) == '\r') ? nl - 1 : nl;
  // column j of 1, 3, 4, 5: from behind tab a (the line start for CHROM) to tab b
  const long a0[4] = {lo, t[1] + 1, t[2] + 1, t[3] + 1}, b0[4] = {t[0], t[2], t[3], t[4]};
  const bool reach[4] = {true, t[1] >= 0, t[2] >= 0, t[3] >= 0};
  int32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long a = reach[j] ? a0[j] : end, b = reach[j] && b0[j] >= 0 ? b0[j] : end;
    if (lane == 2 * j) v = (int32_t)a;
    if (lane == 2 * j + 1) v = (int32_t)(b - a);
  }
  if (lane < 8) spans[line * 8 + lane] = v;
}

constexpr int CG_SHORT = 16;     // bytes a lane copies itself; a longer string is copied by its whole wave

// Item i = c * n + r is column c (0 .. 3) of record r: its spans[r][2 c .. 2 c + 1] bytes of text go to
// blob[off[i], off[i + 1]).  A lane owns an item.  An item whose span leaves the text, whose length is not
// off[i + 1] - off[i], or whose range leaves the blob copies nothing: no store leaves a record's own range.
__global__ __launch_bounds__(256) void vcf_cols_gather_kernel(const uint8_t* __restrict__ text, long nbytes,
                                                              const int32_t* __restrict__ spans, long n,
                                                              const int64_t* __restrict__ off,
                                                              uint8_t* __restrict__ blob, long blob_bytes) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  long src = 0, dst = 0;
  int len = 0;
  if (i < 4 * n) {
    const long c = i / n, r = i - c * n;
    const long s = spans[r * 8 + 2 * c], l = spans[r * 8 + 2 * c + 1], d0 = off[i], d1 = off[i + 1];
    if (s >= 0 && l > 0 && s + l <= nbytes && d0 >= 0 && d1 - d0 == l && d1 <= blob_bytes) {
      src = s;
      dst = d0;
      len = (int)l;
    }
  }
  if (len <= CG_SHORT)
    for (int k = 0; k < len; ++k) blob[dst + k] = text[src + k];
  uint64_t m = __ballot(len > CG_SHORT);
  while (m) {                                                  // wave-uniform: one long string per turn
    const int j = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int l = __shfl(len, j, 64);
    const long s = __shfl((int)src, j, 64);                    // src < nbytes < 2^31
    const long d = ((long)__shfl((int)(dst >> 32), j, 64) << 32) | (uint32_t)__shfl((int)dst, j, 64);
    for (int k = lane; k < l; k += 64) blob[d + k] = text[s + k];
  }
}

// the checks of snvrag_vcf_cols_span and snvrag_vcf_cols_gather (reported under the entry's name)
static int vcf_cols_args(const char* where, const uint8_t* text, int64_t nbytes, int64_t n_lines, const void* index,
                         const int32_t* spans, const void* out) {
  SNV_CHECK_AS(where, non_null(text, index, spans, out), "null pointer");
  SNV_CHECK_AS(where, nbytes >= 1 && nbytes < (1LL << 31), "nbytes must be in [1, 2^31)");
  SNV_CHECK_AS(where, n_lines >= 0 && n_lines <= nbytes, "n_lines must be in [0, nbytes]");
  SNV_CHECK_AS(where, aligned(16, text) && aligned(8, index) && aligned(4, spans),
               "text must be 16-byte aligned, the offsets 8-byte aligned, spans 4-byte aligned");
  return 0;
}

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace snvrag

using namespace snvrag;

extern "C" size_t snvrag_vcf_line_index_ws_bytes(int64_t nbytes) {
  if (nbytes < 0) return 0;
  const size_t nb = (size_t)((nbytes + LI_SPAN - 1) / LI_SPAN);
  return up16(4 * nb) + 8 * nb + 16;
}

extern "C" int snvrag_vcf_line_index(const uint8_t* text, int64_t nbytes, int64_t max_lines, int64_t* line_off,
                                     int64_t* n_lines, void* ws, size_t ws_bytes, void* stream) {
  SNV_CHECK_PTRS(text, line_off, n_lines, ws);
  SNV_CHECK_ARG(nbytes >= 1 && nbytes < (1LL << 31), "nbytes must be in [1, 2^31)");
  SNV_CHECK_ARG(max_lines >= 0, "max_lines must not be negative");
  SNV_CHECK_ARG(aligned(16, text, ws) && aligned(8, line_off),
                "text and ws must be 16-byte aligned, line_off 8-byte aligned");
  SNV_CHECK_ARG(ws_bytes >= snvrag_vcf_line_index_ws_bytes(nbytes), "workspace too small");
  const int nb = (int)((nbytes + LI_SPAN - 1) / LI_SPAN);
  int32_t* counts = static_cast<int32_t*>(ws);
  int64_t* base = reinterpret_cast<int64_t*>(static_cast<uint8_t*>(ws) + up16(4 * (size_t)nb));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(vcf_line_count_kernel, dim3(nb), dim3(LI_THREADS), 0, s, text, (long)nbytes, counts);
  SNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(vcf_line_scan_kernel, dim3(1), dim3(LI_THREADS), 0, s, counts, nb, base, (long)nbytes,
                     (long)max_lines, line_off, n_lines);
  SNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(vcf_line_write_kernel, dim3(nb), dim3(LI_THREADS), 0, s, text, (long)nbytes, base,
                     (long)max_lines, line_off);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t snvrag_vcf_parse_ws_bytes(int64_t n_lines, int64_t S) {
  if (n_lines < 0 || S < 1) return 0;
  const size_t tiles = (size_t)((S + FX_TILE - 1) / FX_TILE);
  return up16((size_t)n_lines) + up16((size_t)n_lines * tiles) + 16;
}

extern "C" int snvrag_vcf_parse_gt(const uint8_t* text, int64_t nbytes, const int64_t* line_off, int64_t n_lines,
                                   int64_t S, int force_general, int32_t* pos, uint32_t* flags, uint8_t* codes,
                                   int64_t ld_codes, void* ws, size_t ws_bytes, void* stream) {
  SNV_CHECK_PTRS(text, line_off, pos, flags, codes, ws);
  SNV_CHECK_ARG(nbytes >= 1 && nbytes < (1LL << 31), "nbytes must be in [1, 2^31)");
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 29), "S must be in [1, 2^29)");
  SNV_CHECK_ARG(n_lines >= 0 && n_lines <= nbytes, "n_lines must be in [0, nbytes]");
  SNV_CHECK_ARG(ld_codes >= S && ld_codes % 4 == 0, "ld_codes must be a multiple of 4, at least S");
  SNV_CHECK_ARG(aligned(16, text, ws) && aligned(4, codes),
                "text and ws must be 16-byte aligned, codes 4-byte aligned");
  SNV_CHECK_ARG(ws_bytes >= snvrag_vcf_parse_ws_bytes(n_lines, S), "workspace too small");
  if (n_lines == 0) return 0;
  const int64_t tiles = (S + FX_TILE - 1) / FX_TILE;
  SNV_CHECK_ARG(n_lines * tiles < (1LL << 31), "n_lines * tiles must be below 2^31");
  uint8_t* redo = static_cast<uint8_t*>(ws);
  uint8_t* tile_or = redo + up16((size_t)n_lines);
  hipStream_t s = as_stream(stream);
  SNV_HIP(hipMemsetAsync(redo, force_general ? 1 : 0, (size_t)n_lines, s));
  if (!force_general) {
    hipLaunchKernelGGL(vcf_parse_fixed_kernel, dim3((unsigned)(n_lines * tiles)), dim3(FX_THREADS), 0, s, text,
                       (long)nbytes, line_off, (int)S, (int)tiles, redo, tile_or, pos, flags, codes, (long)ld_codes);
    SNV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(vcf_parse_general_kernel, dim3((unsigned)((n_lines + 3) / 4)), dim3(256), 0, s, text,
                     (long)nbytes, line_off, (long)n_lines, (int)S, (int)tiles, redo, tile_or, pos, flags, codes,
                     (long)ld_codes);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_vcf_pack_rows(const uint8_t* codes, int64_t ld_codes, int64_t n_lines, int64_t S,
                                    int64_t site0, uint8_t* alt_bits, uint8_t* miss_bits, int64_t ld_bits,
                                    void* stream) {
  SNV_CHECK_PTRS(codes, alt_bits, miss_bits);
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 29), "S must be in [1, 2^29)");
  SNV_CHECK_ARG(n_lines >= 0 && n_lines < (1LL << 40), "n_lines must be in [0, 2^40)");
  SNV_CHECK_ARG(ld_codes >= S && ld_codes % 4 == 0, "ld_codes must be a multiple of 4, at least S");
  SNV_CHECK_ARG(site0 >= 0 && site0 % 64 == 0, "site0 must be a non-negative multiple of 64");
  SNV_CHECK_ARG(ld_bits % 8 == 0 && ld_bits * 8 >= site0 + n_lines, "ld_bits must be a multiple of 8 that holds site0 + n_lines sites");
  SNV_CHECK_ARG(aligned(4, codes) && aligned(8, alt_bits, miss_bits),
                "codes must be 4-byte aligned, the bit rows 8-byte aligned");
  if (n_lines == 0) return 0;
  const int64_t stiles = (S + PK_SMP - 1) / PK_SMP, rtiles = (n_lines + PK_REC - 1) / PK_REC;
  SNV_CHECK_ARG(stiles * rtiles < (1LL << 31), "tiles must be below 2^31");
  hipLaunchKernelGGL(vcf_pack_rows_kernel, dim3((unsigned)(stiles * rtiles)), dim3(PK_THREADS), 0, as_stream(stream),
                     codes, (long)ld_codes, (long)n_lines, (int)S, (int)stiles, alt_bits, miss_bits, (long)ld_bits,
                     (long)(site0 / 8));
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_panel_gather_bits(const uint8_t* bits, int64_t N, int64_t ld_bits, int64_t n_src_sites,
                                        const int32_t* site_idx, int64_t n, int64_t n_sites_pad, int packed,
                                        uint8_t* out, void* stream) {
  SNV_CHECK_PTRS(bits, site_idx, out);
  SNV_CHECK_ARG(N >= 0 && ld_bits >= 1, "N must not be negative, ld_bits at least 1");
  SNV_CHECK_ARG(n_src_sites >= 0 && n_src_sites <= 8 * ld_bits, "n_src_sites must be in [0, 8 ld_bits]");
  SNV_CHECK_ARG(n >= 0 && n <= n_sites_pad && n_sites_pad % 8 == 0 && n_sites_pad < (1LL << 31),
                "n must be in [0, n_sites_pad], n_sites_pad a multiple of 8 below 2^31");
  if (N == 0 || n_sites_pad == 0) return 0;
  const int64_t out_ld = packed ? n_sites_pad / 8 : n_sites_pad;
  const int64_t blocks = (N * out_ld + 255) / 256;
  hipLaunchKernelGGL(panel_gather_bits_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                     as_stream(stream), bits, (long)N, (long)ld_bits, (long)n_src_sites, site_idx, (int)n,
                     (long)out_ld, packed, out);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_vcf_unpack_gt(const uint8_t* alt_bits, const uint8_t* miss_bits, int64_t ld_bits, int64_t S,
                                    int64_t n_sites, int8_t* gt, void* stream) {
  SNV_CHECK_PTRS(alt_bits, miss_bits, gt);
  SNV_CHECK_ARG(S >= 1 && S < (1LL << 29), "S must be in [1, 2^29)");
  SNV_CHECK_ARG(n_sites >= 0 && ld_bits * 8 >= n_sites, "ld_bits must hold n_sites sites");
  SNV_CHECK_ALIGN(2, "gt must be 2-byte aligned", gt);
  if (n_sites == 0) return 0;
  const int64_t sblocks = (S + 255) / 256, rblocks = (n_sites + 7) / 8;
  SNV_CHECK_ARG(sblocks * rblocks < (1LL << 31), "blocks must be below 2^31");
  hipLaunchKernelGGL(vcf_unpack_gt_kernel, dim3((unsigned)(sblocks * rblocks)), dim3(256), 0, as_stream(stream),
                     alt_bits, miss_bits, (long)ld_bits, (int)S, (long)n_sites, (int)sblocks, gt);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_vcf_cols_span(const uint8_t* text, int64_t nbytes, const int64_t* line_off, int64_t n_lines,
                                    int32_t* spans, void* stream) {
  if (int rc = vcf_cols_args("snvrag_vcf_cols_span", text, nbytes, n_lines, line_off, spans, spans)) return rc;
  if (n_lines == 0) return 0;
  hipLaunchKernelGGL(vcf_cols_span_kernel, dim3((unsigned)((n_lines + 3) / 4)), dim3(256), 0, as_stream(stream), text,
                     (long)nbytes, line_off, (long)n_lines, spans);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_vcf_cols_gather(const uint8_t* text, int64_t nbytes, const int32_t* spans, int64_t n_lines,
                                      const int64_t* off, uint8_t* blob, int64_t blob_bytes, void* stream) {
  if (int rc = vcf_cols_args("snvrag_vcf_cols_gather", text, nbytes, n_lines, off, spans, blob)) return rc;
  SNV_CHECK_ARG(blob_bytes >= 0, "blob_bytes must not be negative");
  if (n_lines == 0) return 0;
  hipLaunchKernelGGL(vcf_cols_gather_kernel, dim3((unsigned)((4 * n_lines + 255) / 256)), dim3(256), 0,
                     as_stream(stream), text, (long)nbytes, spans, (long)n_lines, off, blob, (long)blob_bytes);
  SNV_LAUNCH_CHECK();
  return 0;
}
