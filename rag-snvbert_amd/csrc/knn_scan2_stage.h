// One staged block of S2_R haplotypes against this wave's query tiles: B fragment reads from the
// swizzled LDS stage, MFMAs, threshold filter and candidate compaction.  Statement text included
// by scan2_body (knn.hip) inside its stage loop, once for the u8 stage fill and once for the bit
// form, so both run the same code on the same 0/1-byte stage (identical keys by construction).
// Expects in scope: it, smem, NST, STAGE, ROWB, S2_R, KS, LIMBS, QTW, li, lg, wave, lane, k, a,
// th, cnt, mul, cand, r_begin, r_end, ref_offset.
{
    const char* st = smem + (it % NST) * STAGE;
    const long r0 = r_begin + (long)it * S2_R;
    // B fragments (16 haplotypes x 64 sites) of both 16-row groups as one stream,
    // read PF ahead of their MFMAs so LDS latency hides under the MFMA chain
    constexpr int RG = S2_R / 16, F = RG * KS, PF = 4;
    auto bfrag = [&](int f) {
      const int row = 16 * (f / KS) + li, ks = f % KS;
      return *reinterpret_cast<const i32x4*>(st + row * ROWB + (((4 * ks + lg) ^ (row & 15)) << 4));
    };
    i32x4 bq[PF];
#pragma unroll
    for (int f = 0; f < PF; ++f) bq[f] = bfrag(f);
    i32x4 acc[RG][QTW][LIMBS];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
      for (int t = 0; t < QTW; ++t)
#pragma unroll
        for (int lb = 0; lb < LIMBS; ++lb) acc[rg][t][lb] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const i32x4 b = bq[f % PF];
      if (f + PF < F) bq[f % PF] = bfrag(f + PF);
#pragma unroll
      for (int t = 0; t < QTW; ++t)
#pragma unroll
        for (int lb = 0; lb < LIMBS; ++lb)
          acc[f / KS][t][lb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[lb][t][f % KS], b, acc[f / KS][t][lb], 0, 0, 0);
    }
    // pin the interleave (hipcc otherwise sinks each read to just before its MFMA):
    // PF reads, then per fragment {1 read, QTW*LIMBS MFMAs}
    __builtin_amdgcn_sched_group_barrier(0x100, PF, 0);
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if (f + PF < F) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, QTW * LIMBS, 0);
    }
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
      const long r = r0 + 16 * rg + li;
      const bool rv = r < r_end;
#pragma unroll
      for (int t = 0; t < QTW; ++t) {
        uint64_t* buf = cand + (wave * QTW + t) * 16 * S2_CAP;
        int dd[4];
        bool anyp = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dd[i] = LIMBS == 2 ? acc[rg][t][0][i] * 128 + acc[rg][t][1][i] : acc[rg][t][0][i] * mul[t][i];
          anyp |= dd[i] < th[t][i];
        }
        if (!__ballot(rv && anyp)) continue;   // the common case once the threshold is tight
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = dd[i];
          const bool pass = rv && d < th[t][i];
          const uint64_t m = __ballot(pass);
          if (m) {
            const uint32_t gb = (uint32_t)(m >> (16 * lg)) & 0xFFFFu;
            if (pass) {
              const int pre = __popc(gb & ((1u << li) - 1u));
              buf[(4 * lg + i) * S2_CAP + cnt[t][i] + pre] = make_key(d, (uint32_t)(r + ref_offset));
            }
            cnt[t][i] += __popc(gb);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint64_t need = __ballot(cnt[t][i] > S2_TH);
          while (need) {
            const int src = __builtin_ctzll(need);
            const int g = src >> 4;
            need &= ~(0xFFFFull << (16 * g));
            int nc, nt;
            compact_row2(buf, 4 * g + i, __shfl(cnt[t][i], src, 64), k, lane, nc, nt);
            if (lg == g) { cnt[t][i] = nc; th[t][i] = nt; }
          }
        }
      }
    }
}
