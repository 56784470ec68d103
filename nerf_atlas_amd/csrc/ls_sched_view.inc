// MODEL 2: the View reflectance half alone, on given features
// One schedule of render_ls_kernel (csrc/ls_kernel.h), included INSIDE the pass loop of the kernel body: the text of this file is
// the body of one `if constexpr (MODEL == ...)` statement and sees the kernel's locals.  Split out of render_ls.hip in round 5
// (VERDICT r04 next-7): a schedule is edited in its own file; the headline instantiation's ISA is pinned by tests/test_isa_guard.py.
    if constexpr (MODEL == 2) {
      // ================= View head + compositing: EP = compositing of the previous pass + this pass's density / latent rows
      auto none_l = [](int) { return 0; };
      auto none_m = [](int, int, bool) { return 0; };
      if (NB == 4 || owner) {
        prev_dn = own_dn;
        TsPair tprev = {0.f, 0.f};
        if (prev >= 0) tprev = ts_load(prev);
        const Loc L = locate(pass, blk);
        const int t = L.tb * 32 + ln;
        const float* row = a.feat + ((int64_t)(t < a.T ? t : a.T - 1) * a.R + L.ray) * a.feat_ld;
        typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
        const float sdfv = row[0];
        f32x4u lat[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // chunk c, slot 8 hi + e <-> latent 16 c + pi_perm(8 hi + e): two runs of four columns
          lat[c][0] = *(const f32x4u*)(row + 1 + 16 * c + 4 * hi);
          lat[c][1] = *(const f32x4u*)(row + 1 + 16 * c + 8 + 4 * hi);
        }
        own_setup(pass);
        if (prev >= 0) composite(prev_geom(prev, tprev), oc[0], density);
        if (a.beta == nullptr) {
          // column 0 is a density logit (NeRFAE's rows): PlainNeRF's law sigma = softplus(d - 1) (src/nerf.py:60-73), computed as the
          // PlainNeRF schedules compute it; `composite` takes the result as it is (max(sigma, 0) changes nothing)
          density = fast_softplus(sdfv - 1.0f);
        } else {  // Laplace density of this pass's sample (src/utils.py:50-58, src/nerf.py:1000-1003), composited one pass later
          const float sc = a.beta[0];
          const float scaled = (-sdfv) / sc;
          const float cdf = scaled <= 0.f ? fast_exp(scaled) * 0.5f : 1.f - fast_exp(-scaled) * 0.5f;  // (no fminf / fmaxf: they drop a NaN distance)
          density = (1.0f / sc) * cdf;
        }
        if constexpr (PREC == NA_PREC_F16X) {
          // the latent is ONE K64 group of the init region in the hidden format (f16 fragments | R | T), like the [hash | x] and
          // latent groups of PlainNeRF: the lane (sample, k half hi) that loaded the 4 x 8 values of its slots converts them
          f32x16 n0, n1;
#pragma unroll
          for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              n0[8 * c + e] = lat[c][0][e]; n0[8 * c + 4 + e] = lat[c][1][e];
              n1[8 * c + e] = lat[2 + c][0][e]; n1[8 * c + 4 + e] = lat[2 + c][1][e];
            }
          x::store_block<NA_ACT_NONE, 4>(ib + blk * x::KQ, n0, n1, lane, a.sat_gen);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v8[e] = lat[c][0][e]; v8[4 + e] = lat[c][1][e]; }
            fwrite<PREC>(ib + (blk * 4 + c) * FR + lane * 16, make_frag<PREC>(v8));
          }
        }
      }
      geo_setup(pass);
      {
        f32x16 bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 0 * 1024, t, lane);
        if constexpr (PREC == NA_PREC_F16X) x::pairs_prefetch(XR, wrs, xpair, lane, 0, MODEL == 2 ? 2 : 1);
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
        // ---- NA_PREC_F16X: the View half -- records 0 view.init (the latent group) | 1 skip group + 2..5 (view.L0) | 6.. L1..L3 |
        // 18..21 view.out; pairs 0, 1 = the 5-wide geometry chunk of init and skip layer
        {
          GeoRaw graw[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) graw[b] = geo_load(b);
          x::recs<2, NB, true, XNR, 1, 1, 0, 4>(acc, bvx, XR, wrs, xrec, 0, hb, lane, ib);      // view.init: latent group + geometry
          x::geo_pair<0, NB>(acc, XR, wrs, xpair, lane, graw, geo_make, false);
        }
        SYNC();
        {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(1);
          if (owner) {  // sin(latent) for the skip connection: the rows again (L2), through the activation, into the same group
            const Loc L = locate(pass, blk);
            const int t = L.tb * 32 + ln;
            const float* row = a.feat + ((int64_t)(t < a.T ? t : a.T - 1) * a.R + L.ray) * a.feat_ld;
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            f32x16 n0, n1;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const f32x4u p0 = *(const f32x4u*)(row + 1 + 16 * c + 4 * hi), p1 = *(const f32x4u*)(row + 1 + 16 * c + 8 + 4 * hi);
              const f32x4u q0 = *(const f32x4u*)(row + 33 + 16 * c + 4 * hi), q1 = *(const f32x4u*)(row + 33 + 16 * c + 8 + 4 * hi);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                n0[8 * c + e] = p0[e]; n0[8 * c + 4 + e] = p1[e];
                n1[8 * c + e] = q0[e]; n1[8 * c + 4 + e] = q1[e];
              }
            }
            x::store_block<NA_ACT_SIN, 4>(ib + blk * x::KQ, n0, n1, lane, a.sat_gen);
          }
          XR.pr[0] = x::wpair(wrs, lane, xpair, 1);
        }
        SYNC();
        {
          GeoRaw graw[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) graw[b] = geo_load(b);
          x::recs<2, NB, true, XNR, 5, 1, 1, 4>(acc, bvx, XR, wrs, xrec, 1, hb, lane, ib);      // view.L0: skip group, K = 256, geometry
          x::geo_pair<0, NB>(acc, XR, wrs, xpair, lane, graw, geo_make, true);
        }
        SYNC();
#pragma unroll 1
        for (int i = 0; i < 3; ++i) {
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
          xbias(2 + i);
          SYNC();
          x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, 6 + 4 * i, hb, lane);        // view.L1..L3
          SYNC();
        }
        f32x16 ocx[1][1], bo1[1];
        {
          bo1[0] = bias_tile(wrs, bias_rg + 5 * 1024, 0, lane);
          x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
        }
        SYNC();
        x::recs<1, 1, true, XNR>(ocx, bo1, XR, wrs, xrec, 18, hb + blk * x::BLKH, lane);   // view.out (block per wave)
        oc[0] = ocx[0][0];
        SYNC();
        prev = pass;
        continue;
      }
      m_hidden<PREC, 0, 4, 1, 0, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);  // view.init
      SYNC();
#define NA_VIEW_EPILOGUE(PH, FIRST)                                                              \
      {                                                                                            \
        f32x16 bv[2];                                                                              \
        store_acts<PREC, NA_ACT_SIN, 0, 1>(acc, hb, rg, lane);                                     \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + (PH) * 1024, t, lane); \
        store_acts<PREC, NA_ACT_SIN, 1, 2>(acc, hb, rg, lane);                                     \
        if ((FIRST) && owner) activate_init<PREC, NA_ACT_SIN, 4>(ib, blk, lane);                   \
        _Pragma("unroll") for (int t = 0; t < 2; ++t)                                              \
          _Pragma("unroll") for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];                        \
      }                                                                                            \
      SYNC();
      NA_VIEW_EPILOGUE(1, true)
      m_hidden<PREC, 1, 4, 2, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);  // L0 (skip)
      SYNC();
      NA_VIEW_EPILOGUE(2, false)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L1
      SYNC();
      NA_VIEW_EPILOGUE(3, false)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L2
      SYNC();
      NA_VIEW_EPILOGUE(4, false)
      m_hidden<PREC, 2, 0, 0, 16, false, PPP>(acc, ring, cur, wrs, wvoff, hb, ib, lane, none_l, none_m);  // L3
      SYNC();
#undef NA_VIEW_EPILOGUE
      {
        oc[0] = bias_tile(wrs, bias_rg + 5 * 1024, 0, lane);
        store_acts<PREC, NA_ACT_SIN>(acc, hb, rg, lane);
      }
      SYNC();
      m_out<PREC, 2, 1, true, PPP>(oc, ring, cur, wrs, wvoff, hb, lane, blk);
      ring_skip<PREC, 2, 2, true, PPP>(ring, cur, wrs, wvoff);
      SYNC();
      prev = pass;
      continue;
    }
