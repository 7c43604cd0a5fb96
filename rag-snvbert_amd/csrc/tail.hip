// Transformer block tail as ONE kernel on 32x32x16 bf16 MFMAs (gfx950), eval:
//
//   x1  = LN1(x + att W_o^T + b_o)                     multi_head_attention.py:51, sublayer.py:15-16
//   x   = LN2(x1 + lrelu(LN_f(lrelu(x1 W1^T + b1)) W2^T + b2))   feed_forward.py:18-21
//
// A workgroup owns 128 token rows: 4 waves (one per SIMD, up to 512 registers each) x 32
// rows.  Every MFMA computes a TRANSPOSED 32x32 tile (32 weight rows x 32 tokens), so the
// weight fragment (A operand, 1 KiB) read from LDS feeds 2 x 32 x 32 x 16 FLOP — twice the
// work per LDS byte of a 16x16x32 tile — and each lane ends up holding one token's values.
//
// Operands:
//   * activations (att, then x1) live in VGPRs as B fragments for the whole launch
//     (96 registers at D = 384); the LDS is ONE ring of 16 KiB weight slabs streamed
//     once per workgroup by LDS-DMA, 7 slabs (112 KiB) in flight, one barrier per slab
//     placed PF fragments before the slab boundary so LDS reads run ahead across it;
//   * the 4D hidden of a 64-unit chunk stays in registers: phase-1 accumulators are
//     packed straight into phase-2 B fragments (k order baked into W2');
//   * the FFN LayerNorm is folded: W2' = W2 diag(g_f), c1 = rowsum W2',
//     b2' = b2 + W2 b_f, LN_f(h) W2^T + b2 = rstd (h W2'^T) - rstd mean c1 + b2'.
// Lane (token n = lane % 32, half hh = lane / 32) holds output features 32T + 16hh + i
// (i < 16) of tile T: weight ROWS are permuted at pack time (out_feat), the input
// feature order of every B fragment (in_feat) is shared by W_o', W1 and the
// activation loads, so the LN epilogues, the x1 hand-over and the 32-B stores need no
// lane exchange except one xor-32 shuffle per row reduction.
#include "common.h"
#include "mfma32.h"

namespace snvrag {

constexpr int TL_NSLOT = 9;                 // ring slots (144 KiB)
constexpr int TL_ROWS = 128;
constexpr int TL_VEC_LDS = 11 * 1024;       // b1 [4D] + g1, be1, b_o [D] (f32, D <= 384)

template <int D> struct TailShape {
  static constexpr int NT = D / 32;             // 32-feature output tiles
  static constexpr int KS = D / 16;             // 16-wide k steps over D
  static constexpr int NCH = 4 * D / 64;        // 64-unit hidden chunks
  static constexpr int FW1 = 2 * KS;            // W1 fragments per chunk
  static constexpr int FW2 = 4 * NT;            // W2' fragments per chunk
  static constexpr int FPC = FW1 + FW2;         // fragments per chunk
  static constexpr int SPC = FPC / 16;          // slabs per chunk
  static constexpr int FPRE = NT * KS;          // W_o' fragments
  static constexpr int NPRE = FPRE / 16;        // W_o' slabs
  static constexpr int NSLAB = NPRE + NCH * SPC;
  static_assert(FW1 % 16 == 0 && FW2 % 16 == 0 && FPRE % 16 == 0, "parts are whole slabs");
};

// hidden unit (within a 64-unit chunk) at k = 8 kh + j of phase-2 k-step s2 (columns of W2')
__host__ __device__ constexpr int tail_hid(int s2, int kh, int j) {
  return 32 * (s2 >> 1) + 8 * ((8 * (s2 & 1) + j) >> 2) + 4 * kh + ((8 * (s2 & 1) + j) & 3);
}

// wait until at most `younger` (<= MAXY) slabs of this wave (4 LDS-DMA instructions each) are in flight
template <int MAXY> __device__ __forceinline__ void tl_wait(int younger) {
  static_assert(4 * MAXY <= 63, "vmcnt range");
  if constexpr (MAXY <= 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if (younger >= MAXY) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * MAXY) : "memory");
      return;
    }
    tl_wait<MAXY - 1>(younger);
  }
}

struct TailArgs {
  int M;
  const bf16* act;      // PRE: att [M, D]; else x1 [M, D]
  const bf16* resid;    // PRE: x (residual of LN1) [M, D]
  bf16* out;            // [M, D] (PRE: may alias resid)
  const char* ws;       // weight stream (snvrag_tail_pack)
  const float* vec;     // [b1 4D | b2' | c1 | g2 | be2]
  const float* b_o; const float* g1; const float* be1;
  float eps;
  unsigned long long* stamps;   // STAMP (diagnostics): [workgroup][wave][TL_NSTAMP] s_memtime stamps
  int desync;                   // > 0: first-round phase step in cycles (stagger_wait, mfma32.h)
};

// diagnostic stamp points of STAMP (slot 0: s_memrealtime at entry, 1..: s_memtime)
constexpr int TL_NSTAMP = 10;
enum { TS_REAL0 = 0, TS_START, TS_PROLOGUE, TS_PROJ, TS_LN1, TS_FFN, TS_EPI, TS_END, TS_REAL1 };

// Modes: PRE = the whole tail (snvrag_tail_forward); !PRE = the FFN half from x1
// (snvrag_tail_ffn_forward); NC > 0 = projection (snvrag_proj_forward): out[M, NC*D] =
// act W^T + b over NC output chunks of D features (the QKV projection: NC = 3), on the same
// stream / ring / read machinery.
// STAMP (diagnostics, option tail_variant 4 with a snvrag_tail_stamps buffer): the kernel plus
// per-wave s_memtime stamps at the phase boundaries into p.stamps; a separate instantiation,
// so no stamp executes in the real kernel.
// TL_PF, the A fragments read ahead of the MFMA that uses them: 8 in the tail modes (r3: 4
// 1.634 ms, 8 1.659 ms spilling; r5: 8 faster), 4 in the projection.  The stamped kernel reads
// 4 ahead, NOT the default's 8: its phase numbers in DESIGN.md were recorded at 4 and stay
// comparable only with the same code.
template <int D, bool PRE, int NC = 0, bool STAMP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void tail_kernel(TailArgs p) {
  using S = TailShape<D>;
  constexpr int NT = S::NT, KS = S::KS;
  constexpr bool PROJ = NC > 0;
  static_assert(!(PROJ && PRE) && !(PROJ && STAMP), "modes");
  constexpr int TL_PF = (PROJ || STAMP) ? 4 : 8;
  constexpr int NSLAB = (PRE ? S::NPRE : 0) + S::NCH * S::SPC;      // slabs consumed by this launch
  constexpr int RING = TL_NSLOT * SLAB_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float* sv = reinterpret_cast<float*>(smem + RING);               // b1 [4D], g1, be1, b_o
  // wave index as a scalar: every LDS / stream offset below stays in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tid = threadIdx.x, lane = tid & 63;
  const int ln = lane & 31, hh = lane >> 5;
  const long row = (long)blockIdx.x * TL_ROWS + wave * 32 + ln;
  const long rc = row < p.M ? row : (long)p.M - 1;
  // (STAMP) stamp: every lane writes the same value to the same slot through a vector store
  // (branch-free: an exec-masked store splits the unrolled stream into blocks and changes the
  // register allocation being measured)
  auto stamp = [&](int slot, bool real = false) {
    if constexpr (STAMP) {
      const unsigned long long t = real ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();
      __builtin_nontemporal_store(t, p.stamps + ((long)blockIdx.x * 4 + wave) * TL_NSTAMP + slot);
    }
  };
  stamp(TS_REAL0, true);
  if (p.desync > 0 && blockIdx.x < 256) stagger_wait(p.desync);   // de-synchronised rounds (mfma32.h)
  stamp(TS_START);

  // ---- vector tables to LDS first (their loads are waited on at once), then the activations
  // as B fragments (k-step s: features in_feat(s, hh, 0..7)); the residual rows of PRE are
  // loaded after the weight prologue (below) and only needed at LN1, so their HBM burst runs
  // under the out-projection MFMAs
  for (int i = tid; i < (PROJ ? NC : 4) * D; i += 256) sv[i] = p.vec[i];
  if constexpr (PRE)
    for (int i = tid; i < D; i += 256) { sv[4 * D + i] = p.g1[i]; sv[5 * D + i] = p.be1[i]; sv[6 * D + i] = p.b_o[i]; }
  u32x4 xr[KS];                                      // x1 B fragments (PRE: produced by LN1)
  u32x4 xa[(PRE || PROJ) ? KS : 1];                  // PRE: att B fragments; PROJ: x
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    // (default cache policy: non-temporal activation loads/stores measured 8 % slower)
    const u32x4 v = *reinterpret_cast<const u32x4*>(p.act + rc * D + in_feat(s, hh, 0));
    if constexpr (PRE || PROJ) xa[s] = v; else xr[s] = v;
  }

  // ---- weight stream: buffer_load ... lds with scalar offsets; chunks rotated per workgroup
  const int rot = (int)(blockIdx.x % (PROJ ? NC : S::NCH));
  constexpr int STREAM_SLABS = PROJ ? NC * S::NPRE : S::NSLAB;
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.ws, (short)0, STREAM_SLABS * SLAB_BYTES, 0x00020000);
  const int voff = lane * 16;
  // FFN block order (software pipeline, see the chunk loop): with the stream's blocks
  // B(2c) = W1(c), B(2c+1) = W2'(c) (H slabs each) and r = rot, block s of the launch is
  //   s = 0: W1(r);  s = 2k-1 < 2N-1: W1(r+k) = B(2r+s+1);  s = 2k >= 2: W2'(r+k-1) = B(2r+s-1);
  //   s = 2N-1: W2'(r+N-1) = B(2r+s)   (block indices mod 2N)
  constexpr int H = S::FW1 / 16;                     // slabs per W1 (= per W2') block
  constexpr int NB2 = 2 * S::NCH;
  int is_slot = 0;                                   // ring slot (byte offset) of the next issue
  int is_i = 0;                                      // launch slab index of the next issue
  // stream byte offset of launch slab is_i, branch-free (selects only: a branch here splits the
  // unrolled MFMA stream into basic blocks and the register allocator then spills across them)
  auto src_of = [&](int i) -> int {
    if constexpr (PROJ) {                            // chunks rot, rot + 1, ... (mod NC), NPRE slabs each
      const int cc = i / S::NPRE, j = i - cc * S::NPRE;
      const int c = (rot + cc) % NC;
      return (c * S::NPRE + j) * SLAB_BYTES;
    }
    constexpr int NP = PRE ? S::NPRE : 0;
    const int q = i - NP > 0 ? i - NP : 0;
    const int s = q / H, j = q - s * H;              // FFN block, slab within it
    int m = 2 * rot + s + ((s == 0 || s == NB2 - 1) ? 0 : (s & 1) ? 1 : -1);
    m = m >= NB2 ? m - NB2 : m;
    m = m >= NB2 ? m - NB2 : m;                      // (overrun issues run past s = 2N - 1)
    const int ffn = (S::NPRE + m * H + j) * SLAB_BYTES;
    return i < NP ? i * SLAB_BYTES : ffn;
  };
  // Issues run NSLOT - 2 slabs past the end of the launch's stream (the wrapped stream
  // continues, so the addresses stay valid): every sync then has the same number of slabs in
  // flight behind the one it waits for — one constant vmcnt, no per-slab branches.  The
  // overrun lands in slots nobody reads; the epilogue drains it before reusing the ring.
  auto issue_next = [&]() {
    auto* dst = (__attribute__((address_space(3))) void*)(ring + is_slot + wave * 4 * FRAG_BYTES);
    const int src = src_of(is_i);
    ++is_i;
    unroll([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      // (instruction offset 0: the slab offset rides in soffset, the LDS slot in M0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) char*)dst + j * FRAG_BYTES, 16,
                                               voff, src + (wave * 4 + j) * FRAG_BYTES, 0, 0);
    }, std::make_integer_sequence<int, 4>{});
    is_slot = is_slot + SLAB_BYTES == RING ? 0 : is_slot + SLAB_BYTES;
  };
#pragma unroll
  for (int g = 0; g < TL_NSLOT - 1; ++g) issue_next();
  // PRE: the residual rows x, behind the weight prologue in the vmcnt order (NRR loads)
  constexpr int NRR = PRE ? 2 * NT : 0;
  u32x4 rr[PRE ? 2 * NT : 1];
  if constexpr (PRE) {
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
        rr[2 * T + h2] = *reinterpret_cast<const u32x4*>(p.resid + rc * D + 32 * T + 16 * hh + 8 * h2);
  }
  static_assert(4 * (TL_NSLOT - 2) + NRR <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (TL_NSLOT - 2) + NRR) : "memory");
  __syncthreads();                                   // slab 0, the activations + the vector tables visible
  stamp(TS_PROLOGUE);

  // read side: rd_slot = ring slot of the current part's first slab
  int rd_slot = 0;
  auto rdA = [&](auto j_tag, auto fi_tag) -> u32x4 {   // fragment fi of the part's slab j
    constexpr int j = decltype(j_tag)::value, fi = decltype(fi_tag)::value;
    int so = rd_slot + j * SLAB_BYTES;
    so = so >= RING ? so - RING : so;
    return *reinterpret_cast<const u32x4*>(ring + so + lane * 16 + fi * FRAG_BYTES);
  };
  // sync before the first read of slab g (reached PF fragments before its boundary)
  // (g is a compile-time constant where it matters: PRE's first NSLOT - 2 slabs, issued before
  // the residual loads, have those NRR loads behind them in the vmcnt order)
  auto sync = [&](auto g_tag) {
    constexpr int g = decltype(g_tag)::value;
    if constexpr (PRE && g >= 0 && g <= TL_NSLOT - 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (TL_NSLOT - 3) + NRR) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (TL_NSLOT - 3)) : "memory");
    __builtin_amdgcn_s_barrier();
    issue_next();                                    // slab g - 2 + NSLOT into the slot of slab g - 2
  };

  u32x4 a[TL_PF];

  // consume NF fragments (whole slabs) of the part starting at ring slot rd_slot: mma(f, A) per
  // fragment, LDS reads PF ahead (into the next part), one sync per slab
  // G0: the part's first launch slab when known at compile time (PRE), else -1
  // STOP: no reads past the part (the caller re-primes a[] with prime() before the next part)
  auto run = [&](auto nf_tag, auto g0_tag, auto&& mma, auto stop_tag) {
    constexpr int NF = decltype(nf_tag)::value;
    constexpr int G0 = decltype(g0_tag)::value;
    constexpr bool STOP = decltype(stop_tag)::value;
    static_assert(NF % 16 == 0, "parts are whole slabs");
    unroll([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      const u32x4 cur = a[f % TL_PF];
      if constexpr ((f & 15) == 16 - TL_PF) {
        // fence the scheduler at every slab sync: bounds the register live ranges of the
        // fully unrolled stream (hipcc otherwise hoists work across slabs and spills)
        __builtin_amdgcn_sched_barrier(0);
        sync(std::integral_constant<int, (G0 < 0 ? -1 : G0 + (f >> 4) + 1)>{});
      }
      mma(fc, cur);
      // (past the end of the stream this reads stale ring bytes that are never used)
      constexpr int qn = f + TL_PF;
      if constexpr (!STOP || qn < NF)
        a[f % TL_PF] = rdA(std::integral_constant<int, (qn >> 4)>{}, std::integral_constant<int, (qn & 15)>{});
      // pipeline shape for the scheduler: MFMA f, then the read PF fragments ahead
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }, std::make_integer_sequence<int, NF>{});
    rd_slot += (NF / 16) * SLAB_BYTES;
    rd_slot = rd_slot >= RING ? rd_slot - RING : rd_slot;
  };
  auto prime = [&]() {
    unroll([&](auto ic) { a[decltype(ic)::value] = rdA(std::integral_constant<int, 0>{}, ic); },
              std::make_integer_sequence<int, TL_PF>{});
  };

  // (ao: out-projection accumulators; acc: FFN accumulators, born in the first chunk with a zero
  // C operand — explicit zero vectors here get materialised in VGPRs and spilled)
  f32x16 acc[NT];
  prime();
  if constexpr (PROJ) {
    // ---- per output chunk: acc = x W_c^T (zero C operand at k-step 0); + bias -> bf16 in yo.
    // The NT x 2 stores of chunk c go out PPS per slab during chunk c + 1's stream (bounds-
    // checked buffer stores: rows >= M fall outside the resource and are dropped): a burst of
    // stores right before a sync would hold that sync's vmcnt wait until they completed.
    const uint32_t sv_lane = lds_byte_addr(sv) + 64 * hh;   // &sv[16 hh]
    const long out_bytes = (long)p.M * NC * D * 2;
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.out, (short)0, (int)(out_bytes < 0x7fffffffL ? out_bytes : 0x7fffffffL), 0x00020000);
    const int row_off = (int)(row * (NC * D) + 16 * hh) * 2;          // bytes; row < 2^31 / (2 NC D)
    constexpr int PPS = (NT + S::NPRE - 1) / S::NPRE;                 // store pairs per slab
    u32x4 yo[2 * NT];
    int yo_off = 0;                                                   // byte offset of yo's chunk
    auto store_pair = [&](auto t_tag) {
      constexpr int T = decltype(t_tag)::value;
      if constexpr (T < NT) {
        __builtin_amdgcn_raw_buffer_store_b128(yo[2 * T], ors, yo_off + 64 * T, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(yo[2 * T + 1], ors, yo_off + 64 * T + 16, 0, 0);
      }
    };
    auto chunk = [&](int c, auto stores_tag) {
      constexpr bool STORES = decltype(stores_tag)::value;
      unroll([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        run(std::integral_constant<int, 4 * NT>{}, std::integral_constant<int, -1>{}, [&](auto fc, const u32x4& A) {
          constexpr int f = decltype(fc)::value;
          if constexpr (g == 0 && f < NT) acc[f] = mfma32(A, xa[f / NT], f32x16{});
          else acc[f % NT] = mfma32(A, xa[4 * g + f / NT], acc[f % NT]);
          if constexpr (STORES && (f & 15) == 16 - TL_PF) {
            constexpr int slab = g * (NT / 4) + (f >> 4);
            unroll([&](auto pc) { store_pair(std::integral_constant<int, slab * PPS + decltype(pc)::value>{}); },
                      std::make_integer_sequence<int, PPS>{});
          }
        }, std::false_type{});
      }, std::make_integer_sequence<int, KS / 4>{});
#pragma unroll
      for (int T = 0; T < NT; ++T) {
        // bias of features c D + 32 T + 16 hh + 0..15 (reads + wait in one asm: a compiler LDS
        // read would wait for the whole in-flight weight stream, see the FFN bias)
        u32x4 bv[4];
        asm volatile(
            "ds_read_b128 %0, %4 offset:0\n ds_read_b128 %1, %4 offset:16\n ds_read_b128 %2, %4 offset:32\n"
            " ds_read_b128 %3, %4 offset:48\n s_waitcnt lgkmcnt(0)"
            : "=&v"(bv[0]), "=&v"(bv[1]), "=&v"(bv[2]), "=&v"(bv[3])
            : "v"(sv_lane + 4 * (c * D + 32 * T)));
        float y[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] = acc[T][i] + __uint_as_float(bv[i >> 2][i & 3]);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
          yo[2 * T + h2] = u32x4{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                                 pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
      }
      yo_off = row_off + c * D * 2;
    };
    chunk(rot, std::false_type{});
#pragma unroll 1
    for (int cc = 1; cc < NC; ++cc) chunk((rot + cc) % NC, std::true_type{});
    unroll([&](auto tc) { store_pair(tc); }, std::make_integer_sequence<int, NT>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stream overrun has landed before exit
    return;
  }
  if constexpr (PRE) {
    // PRE: the out-projection accumulates onto b_o; LN1 adds the residual x (loaded late, see rr)
    f32x16 ao[NT];
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int i = 0; i < 16; ++i) ao[T][i] = sv[6 * D + 32 * T + 16 * hh + i];
    // ---- ao += att W_o'^T;  fragment f: k-step f / NT, tile f % NT.  A runtime loop over
    // groups of 4 k-steps (4 NT fragments = whole slabs): the att fragments of the group are
    // xa[0..3], shifted down after each group (a straight-line 288-MFMA body makes hipcc
    // shuffle the accumulators between AGPRs)
    static_assert(KS % 4 == 0 && (4 * NT) % 16 == 0, "groups of 4 k-steps are whole slabs");
    unroll([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      run(std::integral_constant<int, 4 * NT>{}, std::integral_constant<int, g * (NT / 4)>{}, [&](auto fc, const u32x4& A) {
        constexpr int f = decltype(fc)::value;
        ao[f % NT] = mfma32(A, xa[4 * g + f / NT], ao[f % NT]);
      }, std::bool_constant<g == KS / 4 - 1>{});
    }, std::make_integer_sequence<int, KS / 4>{});
    stamp(TS_PROJ);
    // ---- x1 = LN1(ao) -> xr (B fragments): pass 1 sums v and v^2, pass 2 normalises
    // (v re-read from the AGPR accumulators, never all held in VGPRs)
    float sum = 0.f, sq = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float v = ao[T][i] + bf_at(rr[2 * T + (i >> 3)], i & 7);
        ao[T][i] = v;
        sum += v;
        sq = fmaf(v, v, sq);
      }
#pragma unroll
    for (int T = 0; T < NT; ++T) asm volatile("" : "+a"(ao[T]));
    asm volatile("" ::: "memory");
    sum = xsum32(sum);
    sq = xsum32(sq);
    const float mean = sum * (1.0f / D);
    const float rstd = 1.0f / sqrtf(fmaxf(sq * (1.0f / D) - mean * mean, 0.f) + p.eps);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      float y[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ft = 32 * T + 16 * hh + i;
        y[i] = (ao[T][i] - mean) * rstd * sv[4 * D + ft] + sv[5 * D + ft];
      }
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
        xr[2 * T + h2] = u32x4{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                               pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
    }
    // the FFN's first fragments are read only now: read ahead across LN1 they were live through
    // it and spilled, and their scratch reloads waited on vmcnt(0), i.e. drained the weight ring
    prime();
  }
  stamp(TS_LN1);
  // x1 opaque from here on: otherwise hipcc folds the epilogue's bf16 -> f32 unpacking of x1
  // into LN1 (it knows pack(y)) and carries 192 unpacked floats through the FFN loop
#pragma unroll
  for (int k = 0; k < KS; ++k) asm volatile("" : "+v"(xr[k]));

  // ---- FFN over 64-unit hidden chunks, software-pipelined: the MFMAs of phase 1 (W1) of
  // chunk k run while the VALU epilogue of chunk k-1 (LeakyReLU, LN_f sums, bf16 packing of
  // its hidden into phase-2 B fragments) is interleaved between them; then phase 2 (W2') of
  // chunk k-1.  Stream order: W1(0), W1(1), W2'(0), W1(2), W2'(1), ..., W2'(N-1).
  float st1 = 0.f, st2 = 0.f;
  const uint32_t sv_lane = lds_byte_addr(sv) + 16 * hh;
  f32x16 h0[2], h1[2];                               // hidden of even / odd chunks (ping-pong)
  u32x4 hf[4];                                       // phase-2 B fragments (k-step 2t + q)
  auto epi_pair = [&](const f32x16 (&hc)[2], int m) {   // hidden values 2m, 2m+1 of hc (m < 16)
    const int t = m >> 3, i = 2 * (m & 7);
    float x0 = hc[t][i], x1 = hc[t][i + 1];
    x0 = lrelu(x0);
    x1 = lrelu(x1);
    st1 += x0 + x1;
    st2 = fmaf(x0, x0, fmaf(x1, x1, st2));
    hf[2 * t + (i >> 3)][(i & 7) >> 1] = pack2(x0, x1);
  };
  // phase 1 of chunk k into hn: h^T = W1_c x1^T + b1 (fragment f: k-step f / 2, tile f % 2; the
  // bias is the C operand of the first k-step, hidden unit of acc element i: 8(i/4) + 4hh + i%4),
  // with the epilogue of the previous chunk (hc) interleaved when EPI
  auto phase1 = [&](int k, f32x16 (&hn)[2], const f32x16 (&hc)[2], auto epi_tag) {
    constexpr bool EPI = decltype(epi_tag)::value;
    const int c = k + rot >= S::NCH ? k + rot - S::NCH : k + rot;
    const uint32_t b1 = sv_lane + 256 * c;          // &sv[64 c + 4 hh]
    u32x4 bv[8];
    // bv[r] = floats 32 (r / 4) + 8 (r % 4) .. + 3 of the chunk's bias: reads and their wait in ONE
    // asm statement (outputs early-clobber: the address stays intact until the last read)
    asm volatile(
        "ds_read_b128 %0, %8 offset:0\n ds_read_b128 %1, %8 offset:32\n ds_read_b128 %2, %8 offset:64\n"
        " ds_read_b128 %3, %8 offset:96\n ds_read_b128 %4, %8 offset:128\n ds_read_b128 %5, %8 offset:160\n"
        " ds_read_b128 %6, %8 offset:192\n ds_read_b128 %7, %8 offset:224\n s_waitcnt lgkmcnt(0)"
        : "=&v"(bv[0]), "=&v"(bv[1]), "=&v"(bv[2]), "=&v"(bv[3]), "=&v"(bv[4]), "=&v"(bv[5]), "=&v"(bv[6]), "=&v"(bv[7])
        : "v"(b1));
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) hn[t][4 * r + e] = __uint_as_float(bv[4 * t + r][e]);
    run(std::integral_constant<int, S::FW1>{}, std::integral_constant<int, -1>{}, [&](auto fc, const u32x4& A) {
      constexpr int f = decltype(fc)::value;
      hn[f & 1] = mfma32(A, xr[f >> 1], hn[f & 1]);
      constexpr int SP = S::FW1 / 16;                // 16 epilogue pairs spread over the MFMAs
      if constexpr (EPI && f % SP == 0) epi_pair(hc, f / SP);
    }, std::false_type{});
  };
  // phase 2 of the chunk whose hidden sits in hf: out^T += W2'_c h_c^T (fragment f: k-step
  // f / NT, output tile f % NT); the first one starts acc with a zero C operand
  auto phase2 = [&](auto first_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    run(std::integral_constant<int, S::FW2>{}, std::integral_constant<int, -1>{}, [&](auto fc, const u32x4& A) {
      constexpr int f = decltype(fc)::value;
      if constexpr (FIRST && f < NT) acc[f] = mfma32(A, hf[0], f32x16{});
      else acc[f % NT] = mfma32(A, hf[f / NT], acc[f % NT]);
    }, std::false_type{});
  };
  // even chunks in h0, odd in h1: no hidden copies (a loop-carried copy makes hipcc shuffle
  // the accumulator registers at every back edge)
  static_assert(S::NCH % 2 == 0 && S::NCH >= 4, "chunk pairs");
  phase1(0, h0, h1, std::false_type{});
  phase1(1, h1, h0, std::true_type{});
  phase2(std::true_type{});
  phase1(2, h0, h1, std::true_type{});
  phase2(std::false_type{});
#pragma unroll 1
  for (int k = 3; k + 1 < S::NCH; k += 2) {
    phase1(k, h1, h0, std::true_type{});
    phase2(std::false_type{});
    phase1(k + 1, h0, h1, std::true_type{});
    phase2(std::false_type{});
  }
  phase1(S::NCH - 1, h1, h0, std::true_type{});
  phase2(std::false_type{});
#pragma unroll
  for (int m = 0; m < 16; ++m) epi_pair(h1, m);
  phase2(std::false_type{});

  stamp(TS_FFN);
  // ---- epilogue: out = LN2(x1 + lrelu(rstd_f acc - rstd_f mean_f c1 + b2'))
  st1 = xsum32(st1);
  st2 = xsum32(st2);
  const float hm = st1 * (1.0f / (4 * D));
  const float hr = 1.0f / sqrtf(fmaxf(st2 * (1.0f / (4 * D)) - hm * hm, 0.f) + p.eps);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stream overrun has landed
  __syncthreads();                                   // every wave is done with the ring
  float* ev = reinterpret_cast<float*>(ring);        // [b2' | c1 | g2 | be2]
  for (int i = wave * 64 + lane_id(); i < 4 * D; i += 256) ev[i] = p.vec[4 * D + i];   // fresh tid (no spill)
  __syncthreads();
  stamp(TS_EPI);
  const float* b2 = ev;
  const float* c1 = ev + D;
  const float* g2 = ev + 2 * D;
  const float* be2 = ev + 3 * D;
  // pass 1: v = x1 + lrelu(rstd_f (acc - mean_f c1) + b2') written back over acc, sums of v and
  // v^2; pass 2 normalises v in place of acc and stores
  float sum = 0.f, sq = 0.f;
#pragma unroll
  for (int T = 0; T < NT; ++T)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ft = 32 * T + 16 * hh + i;
      float u = hr * fmaf(-hm, c1[ft], acc[T][i]) + b2[ft];
      u = lrelu(u);
      const float v = u + bf_at(xr[2 * T + (i >> 3)], i & 7);
      acc[T][i] = v;
      sum += v;
      sq = fmaf(v, v, sq);
      // one tile's vector-table reads at a time: hoisted over all tiles they held ~30 registers
      // while x1 is still live, and x1 was spilled during the last chunk
      if (i == 15) asm volatile("" ::: "memory");
    }
#pragma unroll
  for (int T = 0; T < NT; ++T) asm volatile("" : "+a"(acc[T]));
  asm volatile("" ::: "memory");
  sum = xsum32(sum);
  sq = xsum32(sq);
  const float mean = sum * (1.0f / D);
  const float rstd = 1.0f / sqrtf(fmaxf(sq * (1.0f / D) - mean * mean, 0.f) + p.eps);
  const float nmr = -mean * rstd;
  auto v2 = [&](int T, int i) { return fmaf(acc[T][i], rstd, nmr); };
  // the row recomputed from a fresh lane id (kept live from the prologue it was spilled)
  const long row_e = (long)blockIdx.x * TL_ROWS + wave * 32 + (lane_id() & 31);
  if (row_e < p.M) {
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      float y[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ft = 32 * T + 16 * hh + i;
        y[i] = fmaf(v2(T, i), g2[ft], be2[ft]);
      }
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
        *reinterpret_cast<u32x4*>(p.out + row_e * D + 32 * T + 16 * hh + 8 * h2) =
            u32x4{pack2(y[8 * h2], y[8 * h2 + 1]), pack2(y[8 * h2 + 2], y[8 * h2 + 3]),
                  pack2(y[8 * h2 + 4], y[8 * h2 + 5]), pack2(y[8 * h2 + 6], y[8 * h2 + 7])};
    }
  }
  if constexpr (STAMP) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the row stores have left
    stamp(TS_END);
    stamp(TS_REAL1, true);
  }
}

// One thread per 16-byte piece (8 bf16) of the stream: slab order = consumption order
// (W_o' fragments, then per 64-unit chunk: W1 then W2').  Fragment lane l = (m = l % 32,
// kh = l / 32) holds A[m][8 kh .. 8 kh + 7].
__global__ void tail_pack_kernel(int D, long n_pieces, const bf16* __restrict__ wo, const bf16* __restrict__ w1,
                                 const bf16* __restrict__ w2g, bf16* __restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pieces) return;
  const int NT = D / 32, KS = D / 16, FW1 = 2 * KS, FW2 = 4 * NT, FPC = FW1 + FW2, FPRE = NT * KS;
  const long F = p / 64;
  const int l = (int)(p % 64), m = l & 31, kh = l >> 5;
  bf16 v[8];
  if (F < FPRE) {
    const int s = (int)(F / NT), T = (int)(F % NT);
    const int n = out_feat(T, m);
    for (int j = 0; j < 8; ++j) v[j] = wo[(long)n * D + in_feat(s, kh, j)];
  } else {
    const long g = F - FPRE;
    const int c = (int)(g / FPC), f = (int)(g % FPC);
    if (f < FW1) {
      const int s = f >> 1, t = f & 1;
      const long hid = (long)c * 64 + 32 * t + m;
      for (int j = 0; j < 8; ++j) v[j] = w1[hid * D + in_feat(s, kh, j)];
    } else {
      const int f2 = f - FW1, s2 = f2 / NT, T = f2 % NT;
      const int n = out_feat(T, m);
      for (int j = 0; j < 8; ++j) v[j] = w2g[(long)n * 4 * D + (long)c * 64 + tail_hid(s2, kh, j)];
    }
  }
  for (int j = 0; j < 8; ++j) out[p * 8 + j] = v[j];
}

// Projection stream: per output chunk c (rows c D .. c D + D - 1 of W [NC D, D]), fragments
// F = s NT + T (k-step s, tile T) like the tail's W_o' part.
__global__ void proj_pack_kernel(int D, long n_pieces, const bf16* __restrict__ w, bf16* __restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pieces) return;
  const int NT = D / 32, KS = D / 16, FPRE = NT * KS;
  const long F = p / 64;
  const int l = (int)(p % 64), m = l & 31, kh = l >> 5;
  const int c = (int)(F / FPRE), f = (int)(F % FPRE);
  const int s = f / NT, T = f % NT;
  const long n = (long)c * D + out_feat(T, m);
  for (int j = 0; j < 8; ++j) out[p * 8 + j] = w[n * D + in_feat(s, kh, j)];
}

template <int D, int NC>
static int launch_proj(const TailArgs& a, hipStream_t s) {
  auto kern = tail_kernel<D, false, NC>;
  constexpr size_t lds = (size_t)TL_NSLOT * SLAB_BYTES + NC * D * 4;
  static_assert(NC * D * 4 <= TL_VEC_LDS && lds <= 160 * 1024, "LDS budget");
  return SNV_LAUNCH_LDS(kern, dim3((unsigned)cdiv(a.M, TL_ROWS)), dim3(256), lds, s, a);
}

static unsigned long long* g_tail_stamps = nullptr;   // snvrag_tail_stamps (diagnostics)
unsigned long long* diag_stamps() { return g_tail_stamps; }

// the wide-row tail's first-round stagger (launch_tail below and snvrag_tail_qkv_forward)
static int tailw_desync(int M) { return stagger_step(cdiv(M, TL_ROWS), 8 * 256, options().tail_desync, 10000); }

template <int D, bool PRE>
static int launch_tail(TailArgs a, hipStream_t s) {
  const int var = (int)options().tail_variant;
  // the wide-row form (tailw.hip): every weight fragment loaded once per workgroup into the
  // registers of the one wave that uses it
  if constexpr (PRE && D == 384)
    if (var == 0 && options().tail_wide) {
      // (first-round stagger 10 k cycles: tools/tailw_desync.py, two boxes: 1.409 / 1.403 ms vs
      // 1.454 / 1.399 at tail_kernel's 25 k and 1.444 without; r6: 4 k was 1 % faster alone
      // (tools/tailw_desync_sweep.py) but 0.7 % slower inside the bench step, 1.363 vs 1.353 ms,
      // profiles/r6_tail_desync_bench_ab.txt — 10 k kept)
      return tailw_launch(a.M, a.act, a.resid, a.out, a.ws, a.vec, a.b_o, a.g1, a.be1, a.eps, tailw_desync(a.M),
                          options().tail_wide == 2 ? 1 : 0, nullptr, nullptr, nullptr, s);   // 2: phase stamps
    }
  // default: 8 fragments read ahead (r5: 1.530 vs 1.553 ms at 4, mean of 5 sessions of
  // tools/tail_micro.py at M = 527 360).  tail_variant 4 with a stamp buffer: the stamped kernel
  // (tools/tail_micro.py), which reads 4 ahead (see tail_kernel); any other value runs the default
  auto kern = tail_kernel<D, PRE>;
  if constexpr (D == 384)
    if (var == 4 && g_tail_stamps) {
      kern = tail_kernel<D, PRE, 0, true>;
      a.stamps = g_tail_stamps;
    }
  // first-round phase step: only when every CU runs several rounds (the delay is paid once).
  // Default 1/8 of a block's ~200 k cycles at D = 384 (tools/tail_micro.py, M = 527 360:
  // 1.668 ms without, 1.611 / 1.593 / 1.602 ms at 12 k / 25 k / 40 k), scaled with the D^2 work
  a.desync = stagger_step(cdiv(a.M, TL_ROWS), 8 * 256, options().tail_desync, 25000 * D / 384 * D / 384);
  constexpr size_t lds = (size_t)TL_NSLOT * SLAB_BYTES + 7 * D * 4;     // ring + b1, g1, be1, b_o
  static_assert(7 * D * 4 <= TL_VEC_LDS && lds <= 160 * 1024, "LDS budget");
  return SNV_LAUNCH_LDS(kern, dim3((unsigned)cdiv(a.M, TL_ROWS)), dim3(256), lds, s, a);
}

static bool tail_d_ok(int D) { return D == 128 || D == 256 || D == 384; }

static size_t tail_bytes(int D) {
  return !tail_d_ok(D) ? 0 : dispatch_d(D, [](auto d) { return (size_t)TailShape<d()>::NSLAB * SLAB_BYTES; });
}

}  // namespace snvrag

using namespace snvrag;

extern "C" size_t snvrag_tail_pack_bytes(int D) { return tail_bytes(D); }

extern "C" int snvrag_tail_stamps(void* buf) {
  g_tail_stamps = (unsigned long long*)buf;
  return 0;
}

extern "C" int snvrag_tail_pack(int D, const void* w_o, const void* w1, const void* w2g, void* out, void* stream) {
  SNV_CHECK_ARG(tail_d_ok(D), "block tail needs D in {128, 256, 384}");
  SNV_CHECK_PTRS(w_o, w1, w2g, out);
  const long pieces = (long)(tail_bytes(D) / 16);
  hipLaunchKernelGGL(tail_pack_kernel, dim3((unsigned)cdiv(pieces, 256)), dim3(256), 0, as_stream(stream), D, pieces,
                     (const bf16*)w_o, (const bf16*)w1, (const bf16*)w2g, (bf16*)out);
  SNV_LAUNCH_CHECK();
  return 0;
}

static int tail_common(int64_t M, int D, bool pre, const TailArgs& a, void* stream) {
  hipStream_t s = as_stream(stream);
  evlog_begin(s);
  const int rc = pre ? dispatch_d(D, [&](auto d) { return launch_tail<d(), true>(a, s); })
                     : dispatch_d(D, [&](auto d) { return launch_tail<d(), false>(a, s); });
  if (rc) return rc;
  evlog_end(s, EV_BLOCK, 2.0 * M * (double)D * D * (pre ? 9 : 8));
  return 0;
}

extern "C" int snvrag_tail_forward(int64_t M, int D, const void* att, void* x, const void* wstream, const float* b_o,
                                   const float* ln1_g, const float* ln1_b, const float* ffn_vec, float eps,
                                   void* stream) {
  SNV_CHECK_ARG(tail_d_ok(D), "block tail needs D in {128, 256, 384}");
  SNV_CHECK_PTRS(att, x, wstream, b_o, ln1_g, ln1_b, ffn_vec);
  SNV_CHECK_ARG(att != x, "att and x must not alias");
  SNV_CHECK_M(M);
  SNV_CHECK_ALIGN(16, "pointers must be 16-byte aligned", att, x, wstream, ffn_vec);
  if (M == 0) return 0;
  const TailArgs a{(int)M, (const bf16*)att, (const bf16*)x, (bf16*)x, (const char*)wstream, ffn_vec, b_o, ln1_g,
                   ln1_b, eps, nullptr, 0};
  return tail_common(M, D, true, a, stream);
}

// the block tail and the next layer's QKV projection in one launch (tailw.hip, the projection phase)
extern "C" int snvrag_tail_qkv_forward(int64_t M, int D, const void* att, void* x, const void* wstream,
                                       const float* b_o, const float* ln1_g, const float* ln1_b,
                                       const float* ffn_vec, float eps, const void* qkv_pw, const float* b_qkv,
                                       void* qkv_out, void* stream) {
  SNV_CHECK_ARG(D == 384, "the fused tail + QKV needs D = 384");
  SNV_CHECK_ARG(options().tail_variant == 0 && (options().tail_wide == 1 || options().tail_wide == 2),
                "the fused tail + QKV runs on the wide-row tail only (tail_wide 1 / 2, tail_variant 0)");
  SNV_CHECK_PTRS(att, x, wstream, b_o, ln1_g, ln1_b, ffn_vec, qkv_pw, b_qkv, qkv_out);
  SNV_CHECK_ARG(att != x && qkv_out != x && qkv_out != att, "att, x and qkv_out must not alias");
  SNV_CHECK_M(M);
  SNV_CHECK_ARG((long)M * 3 * D * 2 < (1L << 31), "qkv_out past 2 GiB: run snvrag_tail_forward and a projection");
  SNV_CHECK_ALIGN(16, "pointers must be 16-byte aligned", att, x, wstream, ffn_vec, qkv_pw, b_qkv, qkv_out);
  if (M == 0) return 0;
  hipStream_t s = as_stream(stream);
  evlog_begin(s);
  const int rc = tailw_launch((int)M, att, x, x, wstream, ffn_vec, b_o, ln1_g, ln1_b, eps, tailw_desync((int)M),
                              (int)options().tail_wide - 1, qkv_pw, b_qkv, qkv_out, s);
  if (rc) return rc;
  evlog_end(s, EV_BLOCK, (18.0 + 6.0) * M * (double)D * D);     // the tail's 18 M D^2 + the projection's 6 M D^2
  return 0;
}

extern "C" int snvrag_tail_ffn_forward(int64_t M, int D, const void* x1, void* out, const void* wstream,
                                       const float* ffn_vec, float eps, void* stream) {
  SNV_CHECK_ARG(tail_d_ok(D), "block tail needs D in {128, 256, 384}");
  SNV_CHECK_PTRS(x1, out, wstream, ffn_vec);
  SNV_CHECK_ARG(x1 != out, "x1 and out must not alias");
  SNV_CHECK_M(M);
  SNV_CHECK_ALIGN(16, "pointers must be 16-byte aligned", x1, out, wstream, ffn_vec);
  if (M == 0) return 0;
  const TailArgs a{(int)M, (const bf16*)x1, nullptr, (bf16*)out, (const char*)wstream, ffn_vec, nullptr, nullptr,
                   nullptr, eps, nullptr, 0};
  return tail_common(M, D, false, a, stream);
}

static size_t proj_bytes(int D, int NC) {
  return !tail_d_ok(D) ? 0 : dispatch_d(D, [&](auto d) { return (size_t)NC * TailShape<d()>::NPRE * SLAB_BYTES; });
}

extern "C" size_t snvrag_proj_pack_bytes(int D, int NC) { return proj_bytes(D, NC); }

extern "C" int snvrag_proj_pack(int D, int NC, const void* w, void* out, void* stream) {
  SNV_CHECK_ARG(tail_d_ok(D) && (NC == 1 || NC == 3), "projection needs D in {128, 256, 384}, NC in {1, 3}");
  SNV_CHECK_PTRS(w, out);
  const long pieces = (long)(proj_bytes(D, NC) / 16);
  hipLaunchKernelGGL(proj_pack_kernel, dim3((unsigned)cdiv(pieces, 256)), dim3(256), 0, as_stream(stream), D, pieces,
                     (const bf16*)w, (bf16*)out);
  SNV_LAUNCH_CHECK();
  return 0;
}

extern "C" int snvrag_proj_forward(int64_t M, int D, int NC, const void* x, const void* wstream, const float* bias,
                                   void* out, void* stream) {
  SNV_CHECK_ARG(tail_d_ok(D) && (NC == 1 || NC == 3), "projection needs D in {128, 256, 384}, NC in {1, 3}");
  SNV_CHECK_PTRS(x, wstream, bias, out);
  SNV_CHECK_ARG(x != out, "x and out must not alias");
  SNV_CHECK_M(M);
  SNV_CHECK_ALIGN(16, "pointers must be 16-byte aligned", x, out, wstream);
  if (M == 0) return 0;
  hipStream_t s = as_stream(stream);
  const TailArgs a{(int)M, (const bf16*)x, nullptr, (bf16*)out, (const char*)wstream, bias, nullptr, nullptr,
                   nullptr, 0.f, nullptr, 0};
  evlog_begin(s);
  int rc;
  if (D == 384 && options().proj_wide && (long)M * NC * D * 2 < 0x7fffffffL) {
    // the wide-row projection (tailw.hip): first-round stagger as the block tail's
    const int desync = stagger_step(cdiv(M, TL_ROWS), 8 * 256, options().sg_desync, 8000);
    rc = projw_launch((int)M, NC, x, wstream, bias, out, desync, s);
  } else {
    rc = dispatch_d(D, [&](auto d) { return NC == 1 ? launch_proj<d(), 1>(a, s) : launch_proj<d(), 3>(a, s); });
  }
  if (rc) return rc;
  evlog_end(s, EV_GEMM, 2.0 * M * (double)D * D * NC);
  return 0;
}
