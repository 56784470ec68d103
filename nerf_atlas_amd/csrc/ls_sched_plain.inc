// MODEL 0 / 6: PlainNeRF (hash MLP + View head) -- the headline schedule -- and its mip (IPE) variant
// One schedule of render_ls_kernel (csrc/ls_kernel.h), included INSIDE the pass loop of the kernel body: the text of this file is
// the body of one `if constexpr (MODEL == ...)` statement and sees the kernel's locals.  Split out of render_ls.hip in round 5
// (VERDICT r04 next-7): a schedule is edited in its own file; the headline instantiation's ISA is pinned by tests/test_isa_guard.py.
    // ================= EP: hash encoder of this pass (round 4: the compositing of a pass runs at the end of that pass, in
    // the view.out phase, which is 2.5 k cycles of MFMAs opposite the partner's 8 k-cycle EP; ts / ray of this pass were
    // requested there too, so EP is the cross-block carry + positions + gathers: the group-wide critical path of the three
    // slots around the pass boundary is 17 k instead of 20 k cycles)
    // The 4 x 8 table gathers of this lane half go out one level at a time (35 live registers).  They are TA-bound (64
    // distinct 128-B lines per instruction, 8 MiB of tables): ~10k cycles per group and pass whether issued as four rounds,
    // two or one (measured); spreading the levels over the epilogues of the other layers was slower still (every gathering
    // wave stalls ~3k cycles per round and those epilogues have ~1.8k cycles of slack).
    // (MODEL 0 in NA_PREC_F16X: the encoder has left this phase -- the shadow waves run it under the previous pass's view.out, below)
    STAMP(0);
    if (prev >= 0) combine(prev);  // (partials: written before the barrier that closed view.out; EP does not touch their chunk)
    if constexpr (PREC == NA_PREC_F16X) {
      if constexpr (MIP) {
        geo_setup(pass); mip_setup();
        hash_group_ep(pass);
        gen_ipe(std::integral_constant<int, NA_ACT_NONE>{});
      } else {
        // MODEL 0: the [hash | x] group of this pass was produced under the previous pass's view.out by the shadow waves (pregather,
        // ls_kernel.h); what is left here are their raw values for E1's re-entry, whose stash was still being read until the barrier
        if (!owner) pregather_stash();
        STAMP(7);
      }
    } else
    if (NB == 4 || owner) {  // (bf16x3: row groups 2,3 own no block -- nothing to encode or composite)
      STAMP(8);
      STAMP(9);
      const Geom q = geom(pass, blk, tnext);
      STAMP(10);
      __builtin_amdgcn_sched_barrier(0);
      STAMP(1);
      // bf16x3: levels 2,3 of this lane half are gathered by the partner row group rg + 2 (below), which owns no block
      constexpr int KEND = NB == 4 ? 4 : 2;
      HashGather hg;
#pragma unroll
      for (int k = 0; k < KEND; ++k) {
        hash_level_issue(q.px, q.py, q.pz, a.tables, (hi ? a.res.n[4 + k] : a.res.n[k]), 4 * hi + k, hg);
        hash_finish(k, hg);
        __builtin_amdgcn_sched_barrier(0);
        STAMP(3 + k);
      }
      float v2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v2[e] = 0.f;
      if (hi == 0) { v2[0] = q.px; v2[1] = q.py; v2[2] = q.pz; v2[3] = q.px; v2[4] = q.py; v2[5] = q.pz; }
      fwrite<PREC>(ib + blk * 4 * FR + lane * 16 + 2 * FR, make_frag<PREC>(v2));
      STAMP(7);
    } else {
      // bf16x3, row groups 2 and 3: half of the hash encoder of block rg - 2 (levels 2,3 of each lane half), so that the
      // exposed phase is two gather rounds long instead of four
      const Geom q = geom(pass, blk, tnext);
      HashGather hg;
#pragma unroll
      for (int k = 2; k < 4; ++k) {
        hash_level_issue(q.px, q.py, q.pz, a.tables, (hi ? a.res.n[4 + k] : a.res.n[k]), 4 * hi + k, hg);
        hash_finish(k, hg);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {
      f32x16 bv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 0 * 1024, t, lane);
      SYNC();
      if constexpr (PREC == NA_PREC_F16X) {
        bvx[0] = bv[0]; bvx[1] = bv[1];  // (C operand of first.init's first products)
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
      }
    }
    if constexpr (PREC == NA_PREC_F16X) {
      // ================= NA_PREC_F16X: the same twelve phases on pairs (init / geometry chunks) and records (hidden K)
      // the bias of the NEXT phase waits in bvx and becomes the C operand of that phase's first MFMAs (no accumulator init)
      auto load_bias2 = [&](int ph) {
#pragma unroll
        for (int t = 0; t < 2; ++t) bvx[t] = bias_tile(wrs, bias_rg + ph * 1024, t, lane);
      };
      // records per pass (44, parity of the index = scale slot): 0 first.init | 1 skip group + 2..5 first.L0 | 6.. L1..L3 |
      // 18..21 first.out | 22 view.init | 23 skip group + 24..27 view.L0 | 28.. L1..L3 | 40..43 view.out
      // MODEL 6 (mip): 52 records -- 0..2 first.init ([hash | x], IPE 0, IPE 1) | 3 skip group + 4..7 hidden + 8, 9 IPE (first.L0) |
      // 10.. L1..L3 | 22..25 first.out | 26..28 view.init (latent, IPE 0, IPE 1) | 29 skip group + 30..33 + 34, 35 IPE (view.L0) |
      // 36.. L1..L3 | 48..51 view.out; the IPE groups of a skip layer are regenerated (through the activation) between the
      // layer's two MFMA phases, whose accumulators stay in registers
      constexpr int IPS = 2 * x::KQ;  // block stride of the parked IPE groups
      constexpr int RL1 = MIP ? 10 : 6, ROUT = MIP ? 22 : 18, RVI = MIP ? 26 : 22, RVL0 = MIP ? 29 : 23, RVL1 = MIP ? 36 : 28,
                    RVO = MIP ? 48 : 40;
      if constexpr (MIP) x::recs<2, NB, true, XNR, 3, 1, 0, 3, false, IPS, 3, 2>(acc, bvx, XR, wrs, xrec, 0, hb, lane, ib);
      else x::recs<2, NB, true, XNR, 1, 1, 0, 3>(acc, bvx, XR, wrs, xrec, 0, hb, lane, ib);  // first.init: the [hash | x] group
      SYNC();
      {
        x::store_acts<NA_ACT_LEAKY_RELU, NB, 0, 1>(acc, hb, rg, lane, a.sat_gen);
        if constexpr (MIP) reenter_hash();
        else if (!owner) reenter_pregather();
        x::store_acts<NA_ACT_LEAKY_RELU, NB, 1, 2>(acc, hb, rg, lane, a.sat_gen);
        load_bias2(1);
      }
      SYNC();
      if constexpr (MIP) {
        x::recs<2, NB, true, XNR, 5, 1, 1, 3>(acc, bvx, XR, wrs, xrec, 3, hb, lane, ib);     // first.L0: skip group + K = 256 ...
        SYNC();
        gen_ipe(std::integral_constant<int, NA_ACT_LEAKY_RELU>{});
        SYNC();
        x::recs<2, NB, false, XNR, 2, 0, 0, 4, false, IPS, 3, 2>(acc, bvx, XR, wrs, xrec, 8, hb, lane);  // ... + the IPE groups
      } else {
        x::recs<2, NB, true, XNR, 5, 1, 1, 3>(acc, bvx, XR, wrs, xrec, 1, hb, lane, ib);     // first.L0: skip group, then K = 256
      }
      SYNC();
#pragma unroll 1
      for (int i = 0; i < 3; ++i) {
        x::store_acts<NA_ACT_LEAKY_RELU, NB>(acc, hb, rg, lane, a.sat_gen);
        load_bias2(2 + i);
        SYNC();
        x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, RL1 + 4 * i, hb, lane);                // first.L1..L3
        SYNC();
      }
      // first.out, split by BLOCK (NB = 2): every row group runs two tiles for ONE block, rg & 1 -- row groups 0, 1 the two
      // latent tiles (rows 0..63: the 32 values of an MFMA lane of the View MLP's latent group end up in one lane, which converts
      // them like a hidden epilogue), row groups 2, 3 the density tile (row 64) and an all-zero tile.  One code path for the
      // four waves: a wave-dependent choice between two instantiations of the record loop made the compiler reconcile the
      // weight registers at the join through scratch memory (165 spilled registers, every phase 30 % slower).
      static_assert(NB == 2, "first.out by block");
      f32x16 ol[2][1];
      {
        x::store_acts<NA_ACT_LEAKY_RELU, NB>(acc, hb, rg, lane, a.sat_gen);
        bvx[0] = bias_tile(wrs, bias_rg + 5 * 1024, rg < 2 ? 0 : 2, lane);
        bvx[1] = bias_tile(wrs, bias_rg + 5 * 1024, rg < 2 ? 1 : 3, lane);  // (slot 3: zeros)
      }
      SYNC();
      x::recs<2, 1, true, XNR>(ol, bvx, XR, wrs, xrec, ROUT, hb + (rg & 1) * x::BLKH, lane);
      SYNC();
      {
        load_bias2(6);
        geo_setup(pass);
        if (rg < 2) {
          // the latent group of block rg: raw rows into the (idle) K64 region of wave rg + 2, which converts them for the skip
          // connection in E7, the group itself into the init region
          char* st = hb + x::BLKH + (rg + 2) * x::KQ + lane * 16;  // (that wave's K64 region of block 1: its E7 stores it last)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            *(f32x4*)(st + c * 1024) = f32x4{ol[0][0][4 * c], ol[0][0][4 * c + 1], ol[0][0][4 * c + 2], ol[0][0][4 * c + 3]};
            *(f32x4*)(st + 4096 + c * 1024) = f32x4{ol[1][0][4 * c], ol[1][0][4 * c + 1], ol[1][0][4 * c + 2], ol[1][0][4 * c + 3]};
          }
          x::store_block<NA_ACT_NONE, 4, true>(ib + rg * x::KQ, ol[0][0], ol[1][0], lane, a.sat_gen);
        } else {
          // density of block rg & 1 -> the spare dword of the latent group's T operand (lane = step), where it waits for the
          // compositing at the end of the pass: carried in a register it was the one value spilled AND re-stored every pass
          if (hi == 0) *(float*)(ib + (rg & 1) * x::KQ + 6144 + 1024 + ln * 16 + 12) = ol[0][0][0];
          geo_park(rg & 1);  // view.init's geometry fragment of that block, once for the four waves (these two have the slack)
        }
        if constexpr (MIP) { mip_setup(); gen_ipe(std::integral_constant<int, NA_ACT_NONE>{}); }
        x::pairs_prefetch(XR, wrs, xpair, lane, 0, 1);
      }
      SYNC();
      {
        if constexpr (MIP) x::recs<2, NB, true, XNR, 3, 1, 0, 4, false, IPS, 3, 2>(acc, bvx, XR, wrs, xrec, RVI, hb, lane, ib);
        else x::recs<2, NB, true, XNR, 1, 1, 0, 4>(acc, bvx, XR, wrs, xrec, RVI, hb, lane, ib);  // view.init: latent group + geometry
        x::geo_pair_parked<0, NB, false>(acc, XR, lane, hb);
      }
      SYNC();
      {
        x::store_acts<NA_ACT_SIN, NB, 0, 1>(acc, hb, rg, lane, a.sat_gen);
        if (rg >= 2) {  // sin(latent) of block rg & 1 for the skip connection, from the raw rows (before this wave's block 1 store overwrites their region)
          const char* st = hb + x::BLKH + rg * x::KQ + lane * 16;
          f32x16 l0, l1;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const f32x4 u = *(const f32x4*)(st + c * 1024), w = *(const f32x4*)(st + 4096 + c * 1024);
            l0[4 * c] = u[0]; l0[4 * c + 1] = u[1]; l0[4 * c + 2] = u[2]; l0[4 * c + 3] = u[3];
            l1[4 * c] = w[0]; l1[4 * c + 1] = w[1]; l1[4 * c + 2] = w[2]; l1[4 * c + 3] = w[3];
          }
          x::store_block<NA_ACT_SIN, 4, true>(ib + (rg & 1) * x::KQ, l0, l1, lane, a.sat_gen);
        }
        // view.L0's geometry fragment of block rg, once for the four waves: the parked raw one (in this wave's region of block 1, which
        // the store below overwrites) through the sine, into the spare dwords of the operands this wave has stored by then
        Frag<PREC> gsin;
        if constexpr (!MIP) {
          if (rg < 2) gsin = geo_sin_of_parked(rg);
        }
        x::store_acts<NA_ACT_SIN, NB, 1, 2>(acc, hb, rg, lane, a.sat_gen);
        if constexpr (!MIP) {
          if (rg < 2) x::geo_sin_park(hb, rg, lane, gsin);
        }
        load_bias2(7);
        if constexpr (!MIP) XR.pr[0] = x::wpair(wrs, lane, xpair, 1);  // (the second geometry pair, into the same ring slot: the first one is spent)
      }
      SYNC();
      if constexpr (MIP) {
        x::recs<2, NB, true, XNR, 5, 1, 1, 4>(acc, bvx, XR, wrs, xrec, RVL0, hb, lane, ib);   // view.L0: skip group + K = 256 ...
        SYNC();
        gen_ipe(std::integral_constant<int, NA_ACT_SIN>{});
        XR.pr[0] = x::wpair(wrs, lane, xpair, 1);
        SYNC();
        GeoRaw graw[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) graw[b] = geo_load(b);
        x::recs<2, NB, false, XNR, 2, 0, 0, 4, false, IPS, 3, 2>(acc, bvx, XR, wrs, xrec, RVL0 + 5, hb, lane);  // ... + IPE + geometry
        x::geo_pair<0, NB>(acc, XR, wrs, xpair, lane, graw, geo_make, true);  // (in registers: gen_ipe has rewritten block 0's operands)
      } else {
        x::recs<2, NB, true, XNR, 5, 1, 1, 4>(acc, bvx, XR, wrs, xrec, RVL0, hb, lane, ib);  // view.L0: skip group, K = 256, geometry
        x::geo_pair_parked<0, NB, true>(acc, XR, lane, hb);
      }
      SYNC();
#pragma unroll 1
      for (int i = 0; i < 3; ++i) {
        x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
        load_bias2(8 + i);
        SYNC();
        x::recs<2, NB, true, XNR>(acc, bvx, XR, wrs, xrec, RVL1 + 4 * i, hb, lane);              // view.L1..L3
        SYNC();
      }
      f32x16 ocx[1][1];
      f32x16 bo[1];
      {
        bo[0] = bias_tile(wrs, bias_rg + 11 * 1024, 0, lane);
        x::store_acts<NA_ACT_SIN, NB>(acc, hb, rg, lane, a.sat_gen);
      }
      SYNC();
      if constexpr (MIP) {
        x::recs<1, 1, true, XNR>(ocx, bo, XR, wrs, xrec, RVO, hb + blk * x::BLKH, lane);          // view.out (block per wave)
        oc[0] = ocx[0][0];
        pass_tail(pass);
      } else {
        // MODEL 0: the owner of block blk runs its products and composites; the shadow of the block has no products (nobody reads
        // them) -- the weight registers as the products would leave them, then the next pass's [hash | x] group of the block
        if (owner) x::recs<1, 1, true, XNR>(ocx, bo, XR, wrs, xrec, RVO, hb + blk * x::BLKH, lane);  // view.out (block per wave)
        else x::recs_ring<XNR>(XR, wrs, xrec, RVO, lane);
        if (owner) oc[0] = ocx[0][0];
        pass_tail(pass);
        if (owner) pregather_none();
        else pregather(pass + 1);
      }
      SYNC();
    } else {
    // ================= `first` MLP (LeakyReLU)
    m_hidden<PREC, 0, 3, 0, 0, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, [](int) { return 0; }, [](int, int, bool) { return 0; });
    SYNC();
    {
      f32x16 bv[2];
      train_store(acc, pass, 0);
      // tile 0 first: its 16 x NBLK accumulator registers are dead before the bias of the next layer is loaded
      store_acts<PREC, NA_ACT_LEAKY_RELU, 0, 1>(acc, hb, rg, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 1 * 1024, t, lane);
      store_acts<PREC, NA_ACT_LEAKY_RELU, 1, 2>(acc, hb, rg, lane);
      if (owner) activate_init<PREC, NA_ACT_LEAKY_RELU, 3>(ib, blk, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
    }
    SYNC();
    m_hidden<PREC, 3, 3, 0, 16, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, [](int) { return 0; }, [](int, int, bool) { return 0; });
    SYNC();
    for (int i = 0; i < 3; ++i) {
      f32x16 bv[2];
      train_store(acc, pass, 1 + i);
      // tile 0 first: its 16 x NBLK accumulator registers are dead before the bias of the next layer is loaded
      store_acts<PREC, NA_ACT_LEAKY_RELU, 0, 1>(acc, hb, rg, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + (2 + i) * 1024, t, lane);
      store_acts<PREC, NA_ACT_LEAKY_RELU, 1, 2>(acc, hb, rg, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
      SYNC();
      m_hidden<PREC, 2, 0, 0, 16, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, [](int) { return 0; }, [](int, int, bool) { return 0; });
      SYNC();
    }
    f32x16 oq[NB];  // first.out: this row group's tile (0, 1: latent rows 0..63; 2: density row 64) for the NB blocks
    {
      const f32x16 bo = bias_tile(wrs, bias_rg + 5 * 1024, rg < 2 ? rg : 2, lane);
#pragma unroll
      for (int b = 0; b < NB; ++b) oq[b] = bo;
      train_store(acc, pass, 4);
      store_acts<PREC, NA_ACT_LEAKY_RELU>(acc, hb, rg, lane);
    }
    SYNC();
    // first.out: rows 0..63 = intermediate (-> View latent), row 64 = density
    m_out_rows<PREC, 2, false>(oq, ring, cur, wrs, wvoff, hb, lane);
    SYNC();
    {
      f32x16 bv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 6 * 1024, t, lane);
      geo_setup(pass);  // ray / elev / azim of the group's blocks -> SGPRs, for the two View phases that follow
      train_store_first(oq, pass);
      if (rg < 2) {
        // latent rows 32 rg .. 32 rg + 31 -> init chunks 2 rg, 2 rg + 1 of every block (the View MLP's B fragments)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          Frag<PREC> f0, f1;
          acc_to_frags<PREC, NA_ACT_NONE>(oq[b], f0, f1);
          char* dst = ib + (b * 4 + 2 * rg) * FR + lane * 16;
          fwrite<PREC>(dst, f0);
          fwrite<PREC>(dst + FR, f1);
        }
      } else if (rg == 2 && hi == 0) {
        // density (row 64 = register 0 of the hi = 0 lanes) of block b's 32 samples -> the idle hidden region; block b's
        // owner picks it up after the barrier (it composites the block one pass later)
#pragma unroll
        for (int b = 0; b < NB; ++b) ((float*)hb)[b * 32 + ln] = oq[b][0];
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
    }
    SYNC();
    if (owner) density = ((const float*)hb)[blk * 32 + ln];
    // ================= View MLP (sin)
    m_hidden<PREC, 2, 4, 1, 0, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);
    SYNC();
    {
      f32x16 bv[2];
      train_store(acc, pass, 5);
      // tile 0 first: its 16 x NBLK accumulator registers are dead before the bias of the next layer is loaded
      store_acts<PREC, NA_ACT_SIN, 0, 1>(acc, hb, rg, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + 7 * 1024, t, lane);
      store_acts<PREC, NA_ACT_SIN, 1, 2>(acc, hb, rg, lane);
      if (owner) activate_init<PREC, NA_ACT_SIN, 4>(ib, blk, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
    }
    SYNC();
    m_hidden<PREC, 3, 4, 2, 16, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, geo_load, geo_make);
    SYNC();
    for (int i = 0; i < 3; ++i) {
      f32x16 bv[2];
      train_store(acc, pass, 6 + i);
      // tile 0 first: its 16 x NBLK accumulator registers are dead before the bias of the next layer is loaded
      store_acts<PREC, NA_ACT_SIN, 0, 1>(acc, hb, rg, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = bias_tile(wrs, bias_rg + (8 + i) * 1024, t, lane);
      store_acts<PREC, NA_ACT_SIN, 1, 2>(acc, hb, rg, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[t][b] = bv[t];
      SYNC();
      m_hidden<PREC, 0, 0, 0, 16, false>(acc, ring, cur, wrs, wvoff, hb, ib, lane, [](int) { return 0; }, [](int, int, bool) { return 0; });
      SYNC();
    }
    {
      oc[0] = bias_tile(wrs, bias_rg + 11 * 1024, 0, lane);
      train_store(acc, pass, 9);
      store_acts<PREC, NA_ACT_SIN>(acc, hb, rg, lane);
    }
    SYNC();
    m_out<PREC, 0, 1, true>(oc, ring, cur, wrs, wvoff, hb, lane, blk);
    train_store_rgb(oc[0], pass);
    pass_tail(pass);
    SYNC();
    }  // (PREC != NA_PREC_F16X)
