// MODEL 3: VolSDF with the SIREN SDF network + View head
// One schedule of render_ls_kernel (csrc/ls_kernel.h), included INSIDE the pass loop of the kernel body: the text of this file is
// the body of one `if constexpr (MODEL == ...)` statement and sees the kernel's locals.  Split out of render_ls.hip in round 5
// (VERDICT r04 next-7): a schedule is edited in its own file; the headline instantiation's ISA is pinned by tests/test_isa_guard.py.
    if constexpr (MODEL == 3) {
      // ================= VolSDF, SIREN SDF network + View head: EP = sample position + compositing of the previous pass
      auto none_l = [](int) { return 0; };
      auto none_m = [](int, int, bool) { return 0; };
      if (NB == 4 || owner) {
        prev_dn = own_dn;
        const TsPair tcur = ts_load(pass);
        TsPair tprev = tcur;
        if (prev >= 0) tprev = ts_load(prev);
        own_setup(pass);
        const Geom q = geom(pass, blk, tcur);
        if (prev >= 0) composite(prev_geom(prev, tprev), oc[0], density);
        float v2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v2[e] = 0.f;
        fwrite<PREC>(ib + (blk * 4 + 1) * FR + lane * 16, make_frag<PREC>(v2));  // (the latent of the last pass sat here)
        if (hi == 0) { v2[0] = q.px; v2[1] = q.py; v2[2] = q.pz; }
        fwrite<PREC>(ib + blk * 4 * FR + lane * 16, make_frag<PREC>(v2));
      }
      {
        f32x16 bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 0 * 1024, t, lane);
        if constexpr (PREC == NA_PREC_F16X) x::pairs_prefetch(XR, wrs, xpair, lane, 0, 1);
        SYNC();
        if (prev >= 0) combine(prev);
        if constexpr (PREC == NA_PREC_F16X) {
          bvx[0] = bv[0]; bvx[1] = bv[1];
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
        }
      }
      if constexpr (PREC == NA_PREC_F16X) {
        // ---- NA_PREC_F16X: sdf.init (pair 0), L0 (skip pair 1 + records 0..3), L1, L2, L3 (skip pair 2 + records 12..15), L4,
        // sdf.out (records 20..23, row-major), then the View half (pairs 3..12, records 24..43)
        x::pairs<0, 1, NB>(acc, bvx, XR, wrs, xpair, ib, lane);
        SYNC();
        {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(1);
          if (owner) activate_init<PREC, NA_ACT_SIN, 1>(ib, blk, lane);
          x::pairs_prefetch(XR, wrs, xpair, lane, 1, 1);
        }
        SYNC();
        x::pairs<1, 1, NB>(acc, bvx, XR, wrs, xpair, ib, lane);
        x::recs<2, NB, false, XNR>(acc, bvx, XR, wrs, xrec, 0, hb, lane);                    // L0 (skip)
        SYNC();
#pragma unroll 1
        for (int i = 0; i < 2; ++i) {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(2 + i);
          SYNC();
          x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, 4 + 4 * i, hb, lane);             // L1, L2
          SYNC();
        }
        {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(4);
          x::pairs_prefetch(XR, wrs, xpair, lane, 2, 1);
        }
        SYNC();
        x::pairs<2, 1, NB>(acc, bvx, XR, wrs, xpair, ib, lane);
        x::recs<2, NB, false, XNR>(acc, bvx, XR, wrs, xrec, 12, hb, lane);                   // L3 (skip)
        SYNC();
        {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(5);
        }
        SYNC();
        x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, 16, hb, lane);                     // L4
        SYNC();
        // sdf.out split by BLOCK like PlainNeRF's first.out (NB = 2): every row group runs two tiles for ONE block, rg & 1 -- row
        // groups 0, 1 the two latent tiles (rows 0..63: the 32 values of an MFMA lane of the View MLP's latent group end up in one
        // lane), row groups 2, 3 the signed-distance tile (row 64) and an all-zero tile.  Then the View half on records: 24 view.init
        // (the latent group) | 25 skip group + 26..29 (view.L0) | 30.. L1..L3 | 42..45 view.out; pairs 3, 4 = the geometry chunk
        static_assert(NB == 2, "sdf.out by block");
        f32x16 ol[2][1];
        {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          bvx[0] = bias_tile(wrs, bias_rg + 6 * 1024, rg < 2 ? 0 : 2, lane);
          bvx[1] = bias_tile(wrs, bias_rg + 6 * 1024, rg < 2 ? 1 : 3, lane);  // (slot 3: zeros)
        }
        SYNC();
        x::recs<2, 1, true, XNR>(ol, bvx, XR, wrs, xrec, 20, hb + (rg & 1) * x::BLKH, lane);  // sdf.out
        SYNC();
        {
          xbias(7);
          geo_setup(pass);
          if (rg < 2) {
            // the latent group of block rg: raw rows into the wave's own (idle) K64 region of block 1 for the skip connection, the
            // group itself into the init region
            char* st = hb + x::BLKH + rg * x::KQ + lane * 16;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              *(f32x4*)(st + c * 1024) = f32x4{ol[0][0][4 * c], ol[0][0][4 * c + 1], ol[0][0][4 * c + 2], ol[0][0][4 * c + 3]};
              *(f32x4*)(st + 4096 + c * 1024) = f32x4{ol[1][0][4 * c], ol[1][0][4 * c + 1], ol[1][0][4 * c + 2], ol[1][0][4 * c + 3]};
            }
            x::store_block<NA_ACT_NONE, 4>(ib + rg * x::KQ, ol[0][0], ol[1][0], lane, a.sat_gen);
          } else if (hi == 0) {
            ((float*)hb)[(rg & 1) * 32 + ln] = ol[0][0][0];  // the signed distance of block rg & 1 (lane = step), for its owner
          }
          x::pairs_prefetch(XR, wrs, xpair, lane, 3, 1);
        }
        SYNC();
        if (owner) {  // signed distance -> Laplace density (src/utils.py:50-58, src/nerf.py:1000-1003), composited one pass later
          const float sdfv = ((const float*)hb)[blk * 32 + ln];
          const float sc = a.beta[0];
          const float scaled = (-sdfv) / sc;
          const float cdf = scaled <= 0.f ? fast_exp(scaled) * 0.5f : 1.f - fast_exp(-scaled) * 0.5f;  // (no fminf / fmaxf: they drop a NaN distance)
          density = (1.0f / sc) * cdf;
        }
        {
          GeoRaw graw[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) graw[b] = geo_load(b);
          x::recs<2, NB, true, XNR, 1, 1, 0, 4>(acc, bvx, XR, wrs, xrec, 24, hb, lane, ib);     // view.init: latent group + geometry
          x::geo_pair<1, NB>(acc, XR, wrs, xpair, lane, graw, geo_make, false);                  // (pair 3 sits in ring slot 1)
        }
        SYNC();
        {
          x::store_acts<NA_ACT_SIN, NB, 0, 1>(acc, hb, rg, lane, a.sat_gen);
          if (rg < 2) {  // sin(latent) for the skip connection, from the raw rows (before block 1's store overwrites their region)
            const char* st = hb + x::BLKH + rg * x::KQ + lane * 16;
            f32x16 l0, l1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const f32x4 u = *(const f32x4*)(st + c * 1024), w = *(const f32x4*)(st + 4096 + c * 1024);
              l0[4 * c] = u[0]; l0[4 * c + 1] = u[1]; l0[4 * c + 2] = u[2]; l0[4 * c + 3] = u[3];
              l1[4 * c] = w[0]; l1[4 * c + 1] = w[1]; l1[4 * c + 2] = w[2]; l1[4 * c + 3] = w[3];
            }
            x::store_block<NA_ACT_SIN, 4>(ib + rg * x::KQ, l0, l1, lane, a.sat_gen);
          }
          x::store_acts<NA_ACT_SIN, NB, 1, 2>(acc, hb, rg, lane, a.sat_gen);
          xbias(8);
          XR.pr[0] = x::wpair(wrs, lane, xpair, 4);
        }
        SYNC();
        {
          GeoRaw graw[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) graw[b] = geo_load(b);
          x::recs<2, NB, true, XNR, 5, 1, 1, 4>(acc, bvx, XR, wrs, xrec, 25, hb, lane, ib);     // view.L0: skip group, K = 256, geometry
          x::geo_pair<0, NB>(acc, XR, wrs, xpair, lane, graw, geo_make, true);
        }
        SYNC();
#pragma unroll 1
        for (int i = 0; i < 3; ++i) {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(9 + i);
          SYNC();
          x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, 30 + 4 * i, hb, lane);        // view.L1..L3
          SYNC();
        }
        f32x16 ocx[1][1], bo1[1];
        {
          bo1[0] = bias_tile(wrs, bias_rg + 12 * 1024, 0, lane);
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
        }
        SYNC();
        x::recs<1, 1, true, XNR>(ocx, bo1, XR, wrs, xrec, 42, hb + blk * x::BLKH, lane);   // view.out (block per wave)
        oc[0] = ocx[0][0];
        SYNC();
        prev = pass;
        continue;
      }
      m_hidden<PREC, 0, 2, 0, 0, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // sdf.init
      SYNC();
#define NA_SIN_EPILOGUE(PH, NCHUNK)                                                              \
      {                                                                                            \
        f32x16 bv[2];                                                                              \
        store_acts<PREC, NA_ACT_SIN, 0, 1>(acc, hb, rg, lane);                                     \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + (PH) * 1024, t, lane); \
        store_acts<PREC, NA_ACT_SIN, 1, 2>(acc, hb, rg, lane);                                     \
        if ((NCHUNK) > 0 && owner) activate_init<PREC, NA_ACT_SIN, ((NCHUNK) > 0 ? (NCHUNK) : 1)>(ib, blk, lane); \
        _Pragma("unroll") for (int t = 0; t < 2; ++t)                                              \
          _Pragma("unroll") for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];                        \
      }                                                                                            \
      SYNC();
      NA_SIN_EPILOGUE(1, 1)
      m_hidden<PREC, 2, 1, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L0 (skip)
      SYNC();
      NA_SIN_EPILOGUE(2, 0)
      m_hidden<PREC, 3, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L1
      SYNC();
      NA_SIN_EPILOGUE(3, 0)
      m_hidden<PREC, 3, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L2
      SYNC();
      NA_SIN_EPILOGUE(4, 0)
      m_hidden<PREC, 3, 1, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L3 (skip)
      SYNC();
      NA_SIN_EPILOGUE(5, 0)
      m_hidden<PREC, 0, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L4
      SYNC();
      f32x16 oq[NB];  // sdf.out: this row group's tile (0, 1: latent rows 0..63; 2: the signed distance, row 64) for the NB blocks
      {
        const f32x16 bo = bias_tile(wrs, bias_rg + 6 * 1024, rg < 2 ? rg : 2, lane);
#pragma unroll
        for (int b = 0; b < NB; ++b) oq[b] = bo;
        store_acts<PREC, NA_ACT_SIN>(acc, hb, rg, lane);
      }
      SYNC();
      m_out_rows<PREC, 0, false>(oq, ring, cur, wrs, wvoff, hb, lane);
      SYNC();
      {
        f32x16 bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 7 * 1024, t, lane);
        geo_setup(pass);
        if (rg < 2) {
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            Frag<PREC> f0, f1;
            acc_to_frags<PREC, NA_ACT_NONE>(oq[b], f0, f1);
            char* dst = ib + (b * 4 + 2 * rg) * FR + lane * 16;
            fwrite<PREC>(dst, f0);
            fwrite<PREC>(dst + FR, f1);
          }
        } else if (rg == 2 && hi == 0) {
#pragma unroll
          for (int b = 0; b < NB; ++b) ((float*)hb)[b * 32 + ln] = oq[b][0];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
      }
      SYNC();
      if (owner) {  // signed distance -> Laplace density (src/utils.py:50-58, src/nerf.py:1000-1003), composited one pass later
        const float sdfv = ((const float*)hb)[blk * 32 + ln];
        const float sc = a.beta[0];
        const float scaled = (-sdfv) / sc;
        const float cdf = scaled <= 0.f ? fast_exp(scaled) * 0.5f : 1.f - fast_exp(-scaled) * 0.5f;  // (no fminf / fmaxf: they drop a NaN distance)
        density = (1.0f / sc) * cdf;
      }
      m_hidden<PREC, 0, 4, 1, 0, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);  // view.init
      SYNC();
      NA_SIN_EPILOGUE(8, 4)
      m_hidden<PREC, 1, 4, 2, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);  // view.L0 (skip)
      SYNC();
      NA_SIN_EPILOGUE(9, 0)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);
      SYNC();
      NA_SIN_EPILOGUE(10, 0)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);
      SYNC();
      NA_SIN_EPILOGUE(11, 0)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);
      SYNC();
#undef NA_SIN_EPILOGUE
      {
        oc[0] = bias_tile(wrs, bias_rg + 12 * 1024, 0, lane);
        store_acts<PREC, NA_ACT_SIN>(acc, hb, rg, lane);
      }
      SYNC();
      m_out<PREC, 2, 1, true, PPP>(oc, ring, cur, wrs, wvoff, hb, lane, blk);
      ring_skip<PREC, 2, 2, true, PPP>(ring, cur, wrs, wvoff);
      SYNC();
      prev = pass;
      continue;
    }
