// RFC 1951 deflate of one BGZF member, written once for the device kernel (csrc/deflate.hip) and for a plain
// host program (tests/deflate_core_main.cc, built under AddressSanitizer by tests/test_deflate_core_cpu.py).
// Input: n bytes, 0 <= n <= 0xff00.  Output: the complete member (18-byte header with the BC subfield, raw
// deflate payload, CRC-32, ISIZE), never longer than n + 31 <= 65 536 bytes; no byte past n + 31 is touched.
//
// How the lanes share the work.  defl_member is called by every lane of a workgroup with the same arguments
// and a context Ctx that gives lane(), nlanes(), sync() (the workgroup barrier) and the integer LDS atomics
// amax / aadd / aor / axor.  Every wide step is a loop `for (i = lane; i < count; i += nlanes)` whose turns
// are independent of each other or meet only in a commutative integer atomic, so what it leaves in the state
// does not depend on nlanes or on which lane ran which turn; the serial steps run on lane 0.  The host runs
// the same text with one lane and sync() empty and therefore produces the device's bytes.  Every branch
// around a sync() tests a value that all lanes read from the state after a sync(): control flow is uniform.
//
// The member is cut into sub-blocks of DEFL_T positions, one dynamic-code deflate block each:
//   match     in batches of DEFL_BATCH positions: every position of the batch reads the hash head of its
//             three bytes (the latest position of an earlier batch with that hash), compares up to 258 bytes
//             and records (length, distance); then the batch is inserted, the largest position winning
//             (amax).  The batch size is part of the format of the result, not of the launch.
//   chain     lane 0 walks the greedy token chain and marks the token starts.
//   count     histogram of literal/length and distance symbols over the marked positions (aadd).
//   codes     leaves ranked by (count, symbol) by all lanes; the two-queue Huffman merge, the depth
//             limit (counts halved until the deepest leaf fits), the canonical codes and the run-length
//             coded header on lane 0.  A tree with fewer than two used symbols gets two 1-bit codes, as zlib
//             writes it, so every tree sent is complete.
//   pack      DEFL_SEGS segments of positions: bit totals per segment, an exclusive scan, then every
//             segment ORs its tokens into the zeroed staging words (aor).
// The coded form is abandoned for one stored block as soon as the payload would pass n + 5 bytes, before
// those bytes are written: the slot is never touched past the final member.
#pragma once
#include <stdint.h>

#include "inflate_core.h"

#define DEFL_HD INFL_HD

namespace snvrag {

constexpr int DEFL_MAX_IN = 0xff00;                 // input bytes per member
constexpr int DEFL_FRAME = 26, DEFL_MAX_MEMBER = 65536;
constexpr int DEFL_T = 8192;                        // positions per sub-block (one deflate block)
constexpr int DEFL_BATCH = 256;                     // positions matched against the same hash heads
constexpr int DEFL_HASH_BITS = 12;
constexpr int DEFL_SEGS = 256, DEFL_SEG = DEFL_T / DEFL_SEGS;
constexpr int DEFL_MIN_MATCH = 3, DEFL_MAX_MATCH = 258, DEFL_WINDOW = 32768;
constexpr int DEFL_TOO_FAR = 4096;                  // a 3-byte match farther back costs more than its literals
constexpr int DEFL_STAGE_WORDS = (2 * DEFL_T + 1024) / 4;   // 16 bits per position, the header, slack
constexpr int DEFL_NLIT = 286, DEFL_NDIST = 30, DEFL_NCL = 19, DEFL_DBASE = 288, DEFL_NSYM = 320;
constexpr uint32_t DEFL_TOKEN = 0x80000000u;        // match record: length | (distance - 1) << 9 | DEFL_TOKEN
static_assert(DEFL_MAX_IN + 5 + DEFL_FRAME <= DEFL_MAX_MEMBER, "the stored form fits a member");
static_assert(DEFL_T % DEFL_BATCH == 0 && DEFL_T % DEFL_SEGS == 0, "whole batches and segments");

struct DeflState {                                  // 77 KiB: the LDS of one workgroup
  uint32_t head[1 << DEFL_HASH_BITS];               // latest position + 1 with that hash, 0 = none
  uint32_t rec[DEFL_T];
  uint32_t stage[DEFL_STAGE_WORDS];
  uint32_t crc_tab[256];
  uint32_t freq[DEFL_NSYM];                         // literal/length 0 .. 285, distance DEFL_DBASE + 0 .. 29
  uint32_t code[DEFL_NSYM];                         // bit-reversed code | length << 16
  uint32_t seg[DEFL_SEGS];
  uint32_t key[DEFL_NLIT];
  uint32_t hw[2 * DEFL_NLIT];                       // node weights: sorted leaves, then the merged nodes
  uint32_t cl_freq[DEFL_NCL], cl_code[DEFL_NCL];
  uint16_t hpar[2 * DEFL_NLIT], hord[DEFL_NLIT];
  uint16_t hdr[DEFL_NLIT + DEFL_NDIST];             // code-length symbol | extra value << 8
  uint16_t cnt[16], next[16];
  uint8_t hdep[2 * DEFL_NLIT];
  uint8_t len[DEFL_NSYM];
  uint8_t cl_len[DEFL_NCL];
  int32_t n_hdr, chain_pos, out_bytes, carry_bits, stored, body_start, blk_end;
  uint32_t carry_byte, crc;
};

// A context for one lane that runs everything (the host program).
struct DeflSerial {
  DEFL_HD int lane() const { return 0; }
  DEFL_HD int nlanes() const { return 1; }
  DEFL_HD void sync() {}
  DEFL_HD void amax(uint32_t* p, uint32_t v) { if (*p < v) *p = v; }
  DEFL_HD void aadd(uint32_t* p, uint32_t v) { *p += v; }
  DEFL_HD void aor(uint32_t* p, uint32_t v) { *p |= v; }
  DEFL_HD void axor(uint32_t* p, uint32_t v) { *p ^= v; }
};

DEFL_HD uint32_t defl_hash(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9E3779B1u) >> (32 - DEFL_HASH_BITS);
}

// common prefix of in[a ..] and in[b ..], at most maxlen; a < b and b + maxlen <= n
DEFL_HD int defl_match_len(const uint8_t* in, int a, int b, int maxlen) {
  int k = 0;
  while (k + 8 <= maxlen) {
    uint64_t x, y;
    __builtin_memcpy(&x, in + a + k, 8);
    __builtin_memcpy(&y, in + b + k, 8);
    if (x != y) return k + (__builtin_ctzll(x ^ y) >> 3);
    k += 8;
  }
  while (k < maxlen && in[a + k] == in[b + k]) ++k;
  return k;
}

DEFL_HD int defl_len_sym(int len) {                 // len in [3, 258] -> symbol - 257
  if (len == DEFL_MAX_MATCH) return 28;
  const int l = len - 3;
  if (l < 8) return l;
  const int e = 29 - __builtin_clz((unsigned)l);
  return 4 * e + 4 + ((l >> e) & 3);
}
DEFL_HD int defl_dist_sym(int dist) {               // dist in [1, 32768]
  const int d = dist - 1;
  if (d < 4) return d;
  const int e = 30 - __builtin_clz((unsigned)d);
  return 2 * e + 2 + ((d >> e) & 1);
}

DEFL_HD uint32_t defl_reverse(uint32_t c, int l) {
  uint32_t r = 0;
  for (int i = 0; i < l; ++i) r |= ((c >> i) & 1u) << (l - 1 - i);
  return r;
}

template <class Ctx>
DEFL_HD void defl_put(Ctx& ctx, uint32_t* stage, int bitpos, uint32_t v, int nb) {      // nb <= 32
  if (nb == 0) return;
  const uint64_t x = (uint64_t)v << (bitpos & 31);
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (lo) ctx.aor(stage + (bitpos >> 5), lo);
  if (hi) ctx.aor(stage + (bitpos >> 5) + 1, hi);
}

// The bits of one token: (v0, n0) the literal or the length code with its extra bits, (v1, n1) the distance's.
DEFL_HD void defl_token(const DeflState& S, uint32_t r, uint8_t lit, uint32_t& v0, int& n0, uint32_t& v1, int& n1) {
  const int L = (int)(r & 511u);
  if (L == 0) {
    const uint32_t c = S.code[lit];
    v0 = c & 0xffffu, n0 = (int)(c >> 16), v1 = 0, n1 = 0;
    return;
  }
  const int ls = defl_len_sym(L);
  uint32_t c = S.code[257 + ls];
  int cl = (int)(c >> 16);
  v0 = (c & 0xffffu) | ((uint32_t)(L - infl_len_base(ls)) << cl), n0 = cl + infl_len_extra(ls);
  const int d = (int)((r >> 9) & 0x7fffu) + 1, ds = defl_dist_sym(d);
  c = S.code[DEFL_DBASE + ds];
  cl = (int)(c >> 16);
  v1 = (c & 0xffffu) | ((uint32_t)(d - (int)infl_dist_base(ds)) << cl), n1 = cl + infl_dist_extra(ds);
}

// Serial half of defl_tree (lane 0): S.hord holds the used symbols in (count, symbol) order.
DEFL_HD void defl_tree_serial(DeflState& S, const uint32_t* freq, int n, int maxbits, uint8_t* lens) {
  int m = 0;
  for (int s = 0; s < n; ++s) {
    lens[s] = 0;
    m += freq[s] != 0;
  }
  if (m == 0) {
    lens[0] = lens[1] = 1;
    return;
  }
  if (m == 1) {
    const int s = S.hord[0];
    lens[s] = 1;
    lens[s == 0 ? 1 : 0] = 1;
    return;
  }
  for (int i = 0; i < m; ++i) S.hw[i] = freq[S.hord[i]];
  for (;;) {
    int i = 0, j = m;
    for (int next = m; next < 2 * m - 1; ++next) {          // the two lightest nodes; a leaf wins a tie
      uint32_t w = 0;
      for (int t = 0; t < 2; ++t) {
        const int pick = (i < m && (j >= next || S.hw[i] <= S.hw[j])) ? i++ : j++;
        w += S.hw[pick];
        S.hpar[pick] = (uint16_t)next;
      }
      S.hw[next] = w;
    }
    S.hdep[2 * m - 2] = 0;
    int maxd = 0;
    for (int node = 2 * m - 3; node >= 0; --node) {         // a parent was made after its children
      const int d = S.hdep[S.hpar[node]] + 1;
      S.hdep[node] = (uint8_t)d;
      if (node < m && d > maxd) maxd = d;
    }
    if (maxd <= maxbits) break;
    for (int k = 0; k < m; ++k) S.hw[k] = (S.hw[k] + 1) >> 1;   // monotone: the order stays; ends at all ones
  }
  for (int i = 0; i < m; ++i) lens[S.hord[i]] = S.hdep[i];
}

// Code lengths, at most maxbits, of the n symbols with counts freq (each below 2^23).  All lanes call it.
template <class Ctx>
DEFL_HD void defl_tree(Ctx& ctx, DeflState& S, const uint32_t* freq, int n, int maxbits, uint8_t* lens) {
  const int lane = ctx.lane(), nl = ctx.nlanes();
  for (int s = lane; s < n; s += nl) S.key[s] = freq[s] ? ((freq[s] << 9) | (uint32_t)s) : 0u;
  ctx.sync();
  for (int s = lane; s < n; s += nl) {
    const uint32_t k = S.key[s];
    if (k) {
      int r = 0;
      for (int j = 0; j < n; ++j) r += (S.key[j] != 0 && S.key[j] < k);
      S.hord[r] = (uint16_t)s;
    }
  }
  ctx.sync();
  if (lane == 0) defl_tree_serial(S, freq, n, maxbits, lens);
  ctx.sync();
}

DEFL_HD void defl_codes(DeflState& S, const uint8_t* lens, int n, uint32_t* code) {     // lane 0
  for (int l = 0; l < 16; ++l) S.cnt[l] = 0;
  for (int s = 0; s < n; ++s) S.cnt[lens[s]] = (uint16_t)(S.cnt[lens[s]] + 1);
  S.cnt[0] = 0;
  uint32_t c = 0;
  for (int l = 1; l < 16; ++l) {
    c = (c + S.cnt[l - 1]) << 1;
    S.next[l] = (uint16_t)c;
  }
  for (int s = 0; s < n; ++s) {
    const int l = lens[s];
    if (l) {
      code[s] = defl_reverse(S.next[l], l) | ((uint32_t)l << 16);
      S.next[l] = (uint16_t)(S.next[l] + 1);
    } else {
      code[s] = 0;
    }
  }
}

DEFL_HD int defl_cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// lane 0: the code lengths of hlit + hdist symbols as code-length symbols with repeats; counts them
DEFL_HD void defl_header_rle(DeflState& S, int hlit, int hdist) {
  const int total = hlit + hdist;
  int i = 0, nh = 0;
  auto L = [&](int q) -> int { return q < hlit ? S.len[q] : S.len[DEFL_DBASE + q - hlit]; };
  auto emit = [&](int sym, int extra) {
    S.hdr[nh++] = (uint16_t)(sym | (extra << 8));
    S.cl_freq[sym] += 1;
  };
  while (i < total) {
    const int v = L(i);
    int run = 1;
    while (i + run < total && L(i + run) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        emit(18, r - 11);
        run -= r;
      }
      if (run >= 3) {
        emit(17, run - 3);
        run = 0;
      }
    } else {
      emit(v, 0);
      --run;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        emit(16, r - 3);
        run -= r;
      }
    }
    while (run-- > 0) emit(v, 0);
  }
  S.n_hdr = nh;
}

// The member of in[0, n) at out[0, return value).  Nothing past out[n + 31) is touched.
template <class Ctx>
DEFL_HD int defl_member(Ctx& ctx, DeflState& S, const uint8_t* in, int n, uint8_t* out) {
  const int lane = ctx.lane(), nl = ctx.nlanes();
  for (int i = lane; i < (1 << DEFL_HASH_BITS); i += nl) S.head[i] = 0;
  for (int i = lane; i < 256; i += nl) S.crc_tab[i] = infl_crc_table_entry((uint32_t)i);
  if (lane == 0) {
    S.chain_pos = 0, S.out_bytes = 0, S.carry_bits = 0, S.carry_byte = 0, S.crc = 0;
    S.stored = n == 0;
  }
  ctx.sync();
  {                                                 // CRC-32: segments joined by x^(8 n) mod P
    const int seglen = (n + DEFL_SEGS - 1) / DEFL_SEGS;
    for (int sg = lane; sg < DEFL_SEGS; sg += nl) {
      const int lo = sg * seglen < n ? sg * seglen : n, hi = lo + seglen < n ? lo + seglen : n;
      if (hi > lo || sg == 0) {
        const uint32_t r = infl_crc_raw(sg == 0 ? 0xffffffffu : 0u, in + lo, hi - lo, S.crc_tab);
        ctx.axor(&S.crc, infl_crc_mul(r, infl_crc_x8n(n - hi)));
      }
    }
  }
  const int nblk = (n + DEFL_T - 1) / DEFL_T;
  for (int k = 0; k < nblk; ++k) {
    ctx.sync();
    if (S.stored) break;
    const int base = k * DEFL_T, cnt = n - base < DEFL_T ? n - base : DEFL_T;
    const bool last = k == nblk - 1;
    // ---- match ----
    for (int b0 = 0; b0 < cnt; b0 += DEFL_BATCH) {
      for (int q = lane; q < DEFL_BATCH; q += nl) {
        const int p = b0 + q, i = base + p;
        if (p < cnt) {
          uint32_t r = 0;
          if (i + DEFL_MIN_MATCH <= n) {
            const uint32_t c = S.head[defl_hash(in + i)];
            const int d = i - ((int)c - 1);
            if (c != 0 && d <= DEFL_WINDOW) {
              const int room = n - i < DEFL_MAX_MATCH ? n - i : DEFL_MAX_MATCH;
              const int len = defl_match_len(in, i - d, i, room);
              if (len > DEFL_MIN_MATCH || (len == DEFL_MIN_MATCH && d <= DEFL_TOO_FAR))
                r = (uint32_t)len | ((uint32_t)(d - 1) << 9);
            }
          }
          S.rec[p] = r;
        }
      }
      ctx.sync();
      for (int q = lane; q < DEFL_BATCH; q += nl) {
        const int p = b0 + q, i = base + p;
        if (p < cnt && i + DEFL_MIN_MATCH <= n) ctx.amax(&S.head[defl_hash(in + i)], (uint32_t)i + 1u);
      }
      ctx.sync();
    }
    for (int w = lane; w < DEFL_STAGE_WORDS; w += nl) S.stage[w] = 0;
    for (int s = lane; s < DEFL_NSYM; s += nl) S.freq[s] = 0;
    for (int s = lane; s < DEFL_NCL; s += nl) S.cl_freq[s] = 0;
    // ---- chain ----
    if (lane == 0) {
      int pos = S.chain_pos;
      const int end = base + cnt;
      while (pos < end) {
        const uint32_t r = S.rec[pos - base];
        S.rec[pos - base] = r | DEFL_TOKEN;
        const int L = (int)(r & 511u);
        pos += L ? L : 1;
      }
      S.chain_pos = pos;
    }
    ctx.sync();
    // ---- count ----
    for (int p = lane; p < cnt; p += nl) {
      const uint32_t r = S.rec[p];
      if (r & DEFL_TOKEN) {
        const int L = (int)(r & 511u);
        if (L) {
          ctx.aadd(&S.freq[257 + defl_len_sym(L)], 1u);
          ctx.aadd(&S.freq[DEFL_DBASE + defl_dist_sym((int)((r >> 9) & 0x7fffu) + 1)], 1u);
        } else {
          ctx.aadd(&S.freq[in[base + p]], 1u);
        }
      }
    }
    if (lane == 0) ctx.aadd(&S.freq[256], 1u);
    ctx.sync();
    // ---- codes ----
    defl_tree(ctx, S, S.freq, DEFL_NLIT, INFL_MAXBITS, S.len);
    defl_tree(ctx, S, S.freq + DEFL_DBASE, DEFL_NDIST, INFL_MAXBITS, S.len + DEFL_DBASE);
    int hlit = DEFL_NLIT, hdist = DEFL_NDIST;
    if (lane == 0) {
      defl_codes(S, S.len, DEFL_NLIT, S.code);
      defl_codes(S, S.len + DEFL_DBASE, DEFL_NDIST, S.code + DEFL_DBASE);
      while (hlit > 257 && S.len[hlit - 1] == 0) --hlit;
      while (hdist > 1 && S.len[DEFL_DBASE + hdist - 1] == 0) --hdist;
      defl_header_rle(S, hlit, hdist);
    }
    ctx.sync();
    defl_tree(ctx, S, S.cl_freq, DEFL_NCL, 7, S.cl_len);
    if (lane == 0) {
      defl_codes(S, S.cl_len, DEFL_NCL, S.cl_code);
      const uint64_t lo = 0x022caa324e804a30ull, hi = 0x3c2e1346cull;      // the order 16 17 18 0 8 7 9 ...
      auto order = [&](int q) -> int { return (int)(q < 12 ? (lo >> (5 * q)) & 31u : (hi >> (5 * (q - 12))) & 31u); };
      int hclen = DEFL_NCL;
      while (hclen > 4 && S.cl_len[order(hclen - 1)] == 0) --hclen;
      int hdr_bits = 3 + 14 + 3 * hclen;
      for (int q = 0; q < S.n_hdr; ++q) hdr_bits += S.cl_len[S.hdr[q] & 255] + defl_cl_extra(S.hdr[q] & 255);
      int64_t body = 0;
      for (int s = 0; s < DEFL_NLIT; ++s)
        body += (int64_t)S.freq[s] * (S.len[s] + (s > 256 ? infl_len_extra(s - 257) : 0));
      for (int s = 0; s < DEFL_NDIST; ++s)
        body += (int64_t)S.freq[DEFL_DBASE + s] * (S.len[DEFL_DBASE + s] + infl_dist_extra(s));
      const int64_t end_bits = S.carry_bits + hdr_bits + body;
      if (S.out_bytes + ((end_bits + 7) >> 3) > (int64_t)n + 5 || end_bits + 64 > (int64_t)DEFL_STAGE_WORDS * 32) {
        S.stored = 1;                               // the stored form is not larger: take it
      } else {
        DeflSerial one;
        int bp = S.carry_bits;
        S.stage[0] = S.carry_byte;
        defl_put(one, S.stage, bp, (last ? 1u : 0u) | (2u << 1), 3), bp += 3;
        defl_put(one, S.stage, bp, (uint32_t)(hlit - 257), 5), bp += 5;
        defl_put(one, S.stage, bp, (uint32_t)(hdist - 1), 5), bp += 5;
        defl_put(one, S.stage, bp, (uint32_t)(hclen - 4), 4), bp += 4;
        for (int q = 0; q < hclen; ++q) defl_put(one, S.stage, bp, S.cl_len[order(q)], 3), bp += 3;
        for (int q = 0; q < S.n_hdr; ++q) {
          const int sym = S.hdr[q] & 255, cl = (int)(S.cl_code[sym] >> 16);
          defl_put(one, S.stage, bp, S.cl_code[sym] & 0xffffu, cl), bp += cl;
          defl_put(one, S.stage, bp, (uint32_t)(S.hdr[q] >> 8), defl_cl_extra(sym)), bp += defl_cl_extra(sym);
        }
        S.body_start = bp;
        S.blk_end = (int)end_bits;
      }
    }
    ctx.sync();
    if (S.stored) break;
    // ---- pack ----
    for (int sg = lane; sg < DEFL_SEGS; sg += nl) {
      const int p1 = (sg + 1) * DEFL_SEG < cnt ? (sg + 1) * DEFL_SEG : cnt;
      uint32_t bits = 0;
      for (int p = sg * DEFL_SEG; p < p1; ++p) {
        const uint32_t r = S.rec[p];
        if (r & DEFL_TOKEN) {
          uint32_t v0, v1;
          int n0, n1;
          defl_token(S, r, in[base + p], v0, n0, v1, n1);
          bits += (uint32_t)(n0 + n1);
        }
      }
      S.seg[sg] = bits;
    }
    ctx.sync();
    if (lane == 0) {
      uint32_t run = (uint32_t)S.body_start;
      for (int sg = 0; sg < DEFL_SEGS; ++sg) {
        const uint32_t b = S.seg[sg];
        S.seg[sg] = run;
        run += b;
      }
    }
    ctx.sync();
    for (int sg = lane; sg < DEFL_SEGS; sg += nl) {
      const int p1 = (sg + 1) * DEFL_SEG < cnt ? (sg + 1) * DEFL_SEG : cnt;
      int bp = (int)S.seg[sg];
      for (int p = sg * DEFL_SEG; p < p1; ++p) {
        const uint32_t r = S.rec[p];
        if (r & DEFL_TOKEN) {
          uint32_t v0, v1;
          int n0, n1;
          defl_token(S, r, in[base + p], v0, n0, v1, n1);
          defl_put(ctx, S.stage, bp, v0, n0), bp += n0;
          defl_put(ctx, S.stage, bp, v1, n1), bp += n1;
        }
      }
    }
    if (lane == 0) {
      const int cl = (int)(S.code[256] >> 16);
      defl_put(ctx, S.stage, S.blk_end - cl, S.code[256] & 0xffffu, cl);
    }
    ctx.sync();
    const int nflush = last ? (S.blk_end + 7) >> 3 : S.blk_end >> 3;
    for (int j = lane; j < nflush; j += nl) out[18 + S.out_bytes + j] = (uint8_t)(S.stage[j >> 2] >> (8 * (j & 3)));
    ctx.sync();
    if (lane == 0) {
      S.carry_byte = last ? 0u : (S.stage[nflush >> 2] >> (8 * (nflush & 3))) & 0xffu;
      S.carry_bits = S.blk_end & 7;
      S.out_bytes += nflush;
    }
  }
  ctx.sync();
  int mlen;
  if (S.stored) {
    if (lane == 0) {
      out[18] = 1;
      const uint32_t un = (uint32_t)n, nn = ~un;
      out[19] = (uint8_t)un, out[20] = (uint8_t)(un >> 8);
      out[21] = (uint8_t)nn, out[22] = (uint8_t)(nn >> 8);
    }
    for (int i = lane; i < n; i += nl) out[23 + i] = in[i];
    mlen = 18 + 5 + n + 8;
  } else {
    mlen = 18 + S.out_bytes + 8;
  }
  if (lane == 0) {
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) out[i] = h[i];
    out[16] = (uint8_t)(mlen - 1), out[17] = (uint8_t)((mlen - 1) >> 8);
    const uint32_t crc = S.crc ^ 0xffffffffu;
    for (int i = 0; i < 4; ++i) {
      out[mlen - 8 + i] = (uint8_t)(crc >> (8 * i));
      out[mlen - 4 + i] = (uint8_t)((uint32_t)n >> (8 * i));
    }
  }
  return mlen;
}

}  // namespace snvrag
