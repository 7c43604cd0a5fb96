// RFC 1951 inflate of one BGZF block, written once for the device kernel (csrc/inflate.hip) and for a plain
// host program (tests/test_inflate_core_cpu.py compiles one under AddressSanitizer): the bit reader, the
// code-length / table builder, the single-symbol decode and the block loop are the same text on both sides.
// No intrinsics; every pointer comes with its bound.  The specification is src/dataset/bgzf.py
// inflate_block_host: the same status codes, the first condition met in stream order wins.
//
// The decode is a canonical walk (one bit per step over count[1..15], as Mark Adler's puff does): the tables
// are count u16 [16] and symbol u16 [n] per code, 0.7 KiB in all, so a wave's tables fit beside its output
// window in the LDS.  Where the bytes go is the caller's: infl_block takes a sink with
//   put(pos, byte)                   out[pos] = byte
//   stored(pos, src, n)              out[pos .. pos + n) = src[0 .. n)           (src inside the payload)
//   match(pos, dist, len)            out[pos + i] = out[pos - dist + i % dist], i < len  (= a byte-by-byte copy)
// and calls them only with pos + n <= isize and dist <= pos.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INFL_HD __host__ __device__ __forceinline__
#else
#define INFL_HD inline
#endif

namespace snvrag {

enum InflStatus {
  INFL_OK = 0,
  INFL_BAD_TYPE = 1,      // reserved block type 3
  INFL_BAD_STORED = 2,    // stored LEN != ~NLEN
  INFL_BAD_LENGTHS = 3,   // HLIT > 286 or HDIST > 30; an oversubscribed code; an incomplete one other than a distance
                          // code of one 1-bit code; a repeat with no previous length or past HLIT + HDIST; no code for 256
  INFL_BAD_SYMBOL = 4,    // literal/length 286-287, distance 30-31, or bits that no code of an incomplete tree matches
  INFL_BAD_DISTANCE = 5,  // a distance that reaches in front of the block's output
  INFL_INPUT_END = 6,     // the bit position passed 8 * in_len
  INFL_OUTPUT_FULL = 7,   // output would pass ISIZE (or the block's range leaves the text buffer)
  INFL_OUTPUT_SHORT = 8,  // the stream ended short of ISIZE
  INFL_BAD_CRC = 9
};

constexpr int INFL_MAX_ISIZE = 65536, INFL_MAXBITS = 15, INFL_MAXLCODES = 286, INFL_MAXDCODES = 30,
              INFL_FIXLCODES = 288;

// ---- bit reader: a 64-bit window refilled four bytes at a time; bytes at or past len read as zero --------
struct InflBits {
  const uint8_t* p;
  int64_t len;     // bytes
  int64_t next;    // index of the next byte to load (may pass len: zeros are shifted in)
  uint64_t buf;
  int cnt;         // valid bits in buf
};

INFL_HD void infl_bits_init(InflBits& b, const uint8_t* p, int64_t len) {
  b.p = p;
  b.len = len;
  b.next = 0;
  b.buf = 0;
  b.cnt = 0;
}

INFL_HD void infl_refill(InflBits& b) {      // cnt < 32 -> cnt >= 32
  uint32_t w = 0;
  if (b.next + 4 <= b.len) {
    __builtin_memcpy(&w, b.p + b.next, 4);
  } else {
    for (int i = 0; i < 4; ++i)
      if (b.next + i < b.len) w |= (uint32_t)b.p[b.next + i] << (8 * i);
  }
  b.buf |= (uint64_t)w << b.cnt;
  b.next += 4;
  b.cnt += 32;
}

// bits consumed so far; the input is exhausted once this passes 8 * len
INFL_HD int64_t infl_bitpos(const InflBits& b) { return 8 * b.next - b.cnt; }
INFL_HD bool infl_over(const InflBits& b) { return infl_bitpos(b) > 8 * b.len; }

INFL_HD uint32_t infl_get(InflBits& b, int n) {      // n in [0, 16]
  if (b.cnt < 32) infl_refill(b);
  const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
  b.buf >>= n;
  b.cnt -= n;
  return v;
}

// ---- canonical Huffman code: count[l] = codes of length l, symbol[] = symbols in code order -------------
// Returns < 0 oversubscribed, 0 complete, > 0 incomplete (the code space left over).  offs: 16 u16 of scratch.
INFL_HD int infl_build(const uint16_t* length, int n, uint16_t* count, uint16_t* symbol, uint16_t* offs) {
  for (int l = 0; l <= INFL_MAXBITS; ++l) count[l] = 0;
  for (int s = 0; s < n; ++s) count[length[s]] = (uint16_t)(count[length[s]] + 1);
  int left = 1;
  for (int l = 1; l <= INFL_MAXBITS; ++l) {
    left <<= 1;
    left -= count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < INFL_MAXBITS; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (int s = 0; s < n; ++s)
    if (length[s] != 0) {
      symbol[offs[length[s]]] = (uint16_t)s;
      offs[length[s]] = (uint16_t)(offs[length[s]] + 1);
    }
  return left;
}

// One symbol; -1 when 15 bits match no code (an incomplete code).  Consumes at least one bit.
INFL_HD int infl_decode(InflBits& b, const uint16_t* count, const uint16_t* symbol) {
  if (b.cnt < 32) infl_refill(b);
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= INFL_MAXBITS; ++l) {
    code |= (int)(b.buf & 1u);
    b.buf >>= 1;
    b.cnt -= 1;
    const int c = count[l];
    if (code - c < first) return symbol[index + (code - first)];
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// The tables of one wave / one host call: 1 404 bytes.
struct InflTables {
  uint16_t lencnt[16], distcnt[16], offs[16];
  uint16_t lensym[INFL_FIXLCODES], distsym[INFL_MAXDCODES];
  uint16_t lengths[19 + INFL_MAXLCODES + INFL_MAXDCODES + 1];   // the code-length code's 19, then HLIT + HDIST <= 316
};

INFL_HD uint16_t infl_len_base(int s) {       // s = symbol - 257 in [0, 29)
  return s < 8 ? (uint16_t)(3 + s) : s == 28 ? (uint16_t)258 : (uint16_t)(3 + ((4 + (s & 3)) << ((s >> 2) - 1)));
}
INFL_HD int infl_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
INFL_HD uint32_t infl_dist_base(int s) {      // s in [0, 30)
  return s < 4 ? (uint32_t)(1 + s) : 1u + ((2u + (uint32_t)(s & 1)) << ((s >> 1) - 1));
}
INFL_HD int infl_dist_extra(int s) { return s < 4 ? 0 : (s >> 1) - 1; }

INFL_HD void infl_fixed_tables(InflTables& t) {
  for (int s = 0; s < INFL_FIXLCODES; ++s) t.lengths[s] = (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  infl_build(t.lengths, INFL_FIXLCODES, t.lencnt, t.lensym, t.offs);
  for (int s = 0; s < INFL_MAXDCODES; ++s) t.lengths[s] = 5;
  infl_build(t.lengths, INFL_MAXDCODES, t.distcnt, t.distsym, t.offs);
}

// The header of a dynamic block -> the two codes.  Status.
INFL_HD int infl_dynamic_tables(InflBits& b, InflTables& t) {
  const int nlen = (int)infl_get(b, 5) + 257, ndist = (int)infl_get(b, 5) + 1, ncode = (int)infl_get(b, 4) + 4;
  if (infl_over(b)) return INFL_INPUT_END;
  if (nlen > INFL_MAXLCODES || ndist > INFL_MAXDCODES) return INFL_BAD_LENGTHS;
  for (int i = 0; i < 19; ++i) t.lengths[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    // the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 0x022caa324e804a30ull, hi = 0x3c2e1346cull;
    const int pos = (int)(i < 12 ? (lo >> (5 * i)) & 31u : (hi >> (5 * (i - 12))) & 31u);
    t.lengths[pos] = (uint16_t)infl_get(b, 3);
  }
  if (infl_over(b)) return INFL_INPUT_END;
  if (infl_build(t.lengths, 19, t.lencnt, t.lensym, t.offs) != 0) return INFL_BAD_LENGTHS;
  int index = 0;
  while (index < nlen + ndist) {                  // each turn consumes at least one bit
    const int sym = infl_decode(b, t.lencnt, t.lensym);
    if (infl_over(b)) return INFL_INPUT_END;
    if (sym < 0) return INFL_BAD_LENGTHS;         // (a complete code always matches)
    if (sym < 16) {
      t.lengths[19 + index++] = (uint16_t)sym;
    } else {
      int len = 0, rep;
      if (sym == 16) {
        if (index == 0) return INFL_BAD_LENGTHS;
        len = t.lengths[19 + index - 1];
        rep = 3 + (int)infl_get(b, 2);
      } else if (sym == 17) {
        rep = 3 + (int)infl_get(b, 3);
      } else {
        rep = 11 + (int)infl_get(b, 7);
      }
      if (infl_over(b)) return INFL_INPUT_END;
      if (index + rep > nlen + ndist) return INFL_BAD_LENGTHS;
      while (rep--) t.lengths[19 + index++] = (uint16_t)len;
    }
  }
  if (t.lengths[19 + 256] == 0) return INFL_BAD_LENGTHS;
  // (the code-length code's tables are dead from here: lencnt / lensym are rebuilt)
  if (infl_build(t.lengths + 19, nlen, t.lencnt, t.lensym, t.offs) != 0) return INFL_BAD_LENGTHS;
  const int left = infl_build(t.lengths + 19 + nlen, ndist, t.distcnt, t.distsym, t.offs);
  // RFC 1951 3.2.7: one distance code is sent as one bit; one code of zero bits means no distance is used
  if (left < 0 || (left > 0 && t.distcnt[0] + t.distcnt[1] != ndist)) return INFL_BAD_LENGTHS;
  return INFL_OK;
}

// Inflate payload[0, in_len) into the sink, which holds exactly isize bytes.  Returns the status (never 9:
// the CRC is the caller's) and the bytes produced in *produced.  Every turn of every loop consumes at least one
// input bit or emits at least one byte, and stops once the input (8 in_len bits) or the output (isize) is passed.
template <class Sink>
INFL_HD int infl_block(const uint8_t* payload, int64_t in_len, int64_t isize, InflTables& t, Sink& sink,
                       int64_t* produced) {
  InflBits b;
  infl_bits_init(b, payload, in_len);
  int64_t pos = 0, base = 0;                     // the reader b stands on payload[base, in_len)
  int status = INFL_OK;
  for (;;) {
    const uint32_t last = infl_get(b, 1), type = infl_get(b, 2);
    if (infl_over(b)) { status = INFL_INPUT_END; break; }
    if (type == 3) { status = INFL_BAD_TYPE; break; }
    if (type == 0) {
      const int64_t at = base + ((infl_bitpos(b) + 7) >> 3);   // the next byte boundary
      if (at + 4 > in_len) { status = INFL_INPUT_END; break; }
      const uint32_t len = payload[at] | ((uint32_t)payload[at + 1] << 8);
      const uint32_t nlen = payload[at + 2] | ((uint32_t)payload[at + 3] << 8);
      if (len != (~nlen & 0xffffu)) { status = INFL_BAD_STORED; break; }
      // bytes in stream order: input runs out first where both bounds break
      const int64_t have = in_len - (at + 4), room = isize - pos;
      if ((int64_t)len > have && have < room) { status = INFL_INPUT_END; break; }
      if ((int64_t)len > room) { status = INFL_OUTPUT_FULL; break; }
      sink.stored(pos, payload + at + 4, (int)len);
      pos += len;
      base = at + 4 + len;                                     // a fresh reader on the rest
      infl_bits_init(b, payload + base, in_len - base);
    } else {
      if (type == 1) {
        infl_fixed_tables(t);
      } else {
        status = infl_dynamic_tables(b, t);
        if (status != INFL_OK) break;
      }
      for (;;) {
        int sym = infl_decode(b, t.lencnt, t.lensym);
        if (infl_over(b)) { status = INFL_INPUT_END; break; }
        if (sym < 0) { status = INFL_BAD_SYMBOL; break; }
        if (sym < 256) {
          if (pos >= isize) { status = INFL_OUTPUT_FULL; break; }
          sink.put(pos, (uint8_t)sym);
          ++pos;
          continue;
        }
        if (sym == 256) break;
        sym -= 257;
        if (sym >= 29) { status = INFL_BAD_SYMBOL; break; }
        const int len = infl_len_base(sym) + (int)infl_get(b, infl_len_extra(sym));
        if (infl_over(b)) { status = INFL_INPUT_END; break; }
        const int ds = infl_decode(b, t.distcnt, t.distsym);
        if (infl_over(b)) { status = INFL_INPUT_END; break; }
        if (ds < 0 || ds >= 30) { status = INFL_BAD_SYMBOL; break; }
        const int64_t dist = (int64_t)infl_dist_base(ds) + infl_get(b, infl_dist_extra(ds));
        if (infl_over(b)) { status = INFL_INPUT_END; break; }
        if (dist > pos) { status = INFL_BAD_DISTANCE; break; }
        if (pos + len > isize) { status = INFL_OUTPUT_FULL; break; }
        sink.match(pos, (int)dist, len);
        pos += len;
      }
      if (status != INFL_OK) break;
    }
    if (last) break;
  }
  if (status == INFL_OK && pos != isize) status = INFL_OUTPUT_SHORT;
  *produced = pos;
  return status;
}

// ---- CRC-32 (gzip: polynomial 0xEDB88320, reflected) ---------------------------------------------------
constexpr uint32_t INFL_CRC_POLY = 0xEDB88320u;

INFL_HD uint32_t infl_crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (INFL_CRC_POLY & (0u - (c & 1u)));
  return c;
}
// the register after the bytes p[0, n), from register c (no pre- or post-inversion); table: 256 entries
INFL_HD uint32_t infl_crc_raw(uint32_t c, const uint8_t* p, int64_t n, const uint32_t* table) {
  for (int64_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return c;
}
// a(x) b(x) mod P in the reflected representation (bit 31 = x^0)
INFL_HD uint32_t infl_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (INFL_CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 n) mod P: multiplying a register by it is what n zero bytes do to it
INFL_HD uint32_t infl_crc_x8n(int64_t n) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;      // x^0, x^8
  while (n) {
    if (n & 1) r = infl_crc_mul(r, sq);
    sq = infl_crc_mul(sq, sq);
    n >>= 1;
  }
  return r;
}

}  // namespace snvrag
