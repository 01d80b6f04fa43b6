// One iteration of render_kernel_p's persistent loop: the BODY of `for (; g >= 0; idx += waves_per_xcd, g = group_of(idx))`, included
// once per loop nest of the kernel (bts_render_kernel.h) with BTS_ITER_SHARED defined to true (the loop for rays whose samples share
// their texels) or false (the general loop).  Text, not a function or a lambda: the kernels WITHOUT the second loop must compile to
// exactly what they were, and the general loop has to keep its registers (a per-ray special case inside one body cost the common
// path spilled VGPRs before: DESIGN.md section 3).  No include guard on purpose.
{
    constexpr bool SHARED = kTwoLoops && (BTS_ITER_SHARED);
    bool other_loop = false;   // kTwoLoops: the ray belongs to the other loop
    const float nrec_in = nrec, z_pre_in = z_pre, zn_pre_in = zn_pre;   // (put back in that case)
    // the parameters of this iteration: re-read from the kernarg segment where they are used instead of held (and spilled) for the
    // whole life of the kernel (bts_common.h: kernarg_view)
    auto q = kernarg_view<FwdParams>();
    asm volatile("" : "+s"(q));
    IterHead ih(q);   // the geometry's share of the parameters (see IterHead: batching their loads was measured and not kept)
    const int K = BTS_PIN(PinnedSet::K, ih.K), H = ih.H, W = ih.W, nv = BTS_PIN(PinnedSet::nv, ih.nv), fs = BTS_PIN(PinnedSet::fs, ih.fs);
    long ray = lane_ray(g, 0);   // (48-lane mode: lanes 0-47 move on to the group's next ray with every chunk of the loop below)
    // all rays of a group belong to one batch element; g only grows along a wave's chunk list, so the element is tracked by a
    // running boundary (the 64-bit division this replaces was ~140 dependent scalar instructions at the top of every iteration)
    while (g >= sample_end) ++sample, sample_end += groups_per_sample;
    const Cam enc = load_cam(ih.w2c_enc + sample * 16, ih.K_enc + sample * 9);
    const float4* __restrict__ G = reinterpret_cast<const float4*>(ih.proj) + (long)sample * (H >> fs) * (W >> fs) * (HD / 4);
    float ox, oy, oz, dx, dy, dz, near = 0.0f, far = 0.0f;
    const bool from_jitter = BTS_PIN(true, ih.z_samp == nullptr);   // wave-uniform
    if constexpr (ONE_RAY) {  // wave-uniform ray, fetched during the previous iteration (nr0 / nr1 above)
      ox = lane_value(nrec, 0), oy = lane_value(nrec, 1), oz = lane_value(nrec, 2), dx = lane_value(nrec, 3), dy = lane_value(nrec, 4);
      dz = lane_value(nrec, 5), near = lane_value(nrec, 6), far = lane_value(nrec, 7);
    } else {
      const float4 r0 = reinterpret_cast<const float4*>(ih.rays)[ray * 2];
      const float4 r1 = reinterpret_cast<const float4*>(ih.rays)[ray * 2 + 1];
      ox = r0.x, oy = r0.y, oz = r0.z, dx = r0.w, dy = r1.x, dz = r1.y, near = r1.z, far = r1.w;
    }
    const float* zsrc = from_jitter ? ih.jitter : ih.z_samp;
    const float* zrow = zsrc + ray * K;
    float z_cur = z_pre, zn_cur = zn_pre;
    // the samples (or the jitter) of what this wave evaluates next: they land while the current unit is evaluated
    auto prefetch_z = [&](int gg, int it) {
      const long row = lane_ray(gg, it) * K;
      const int kk = min(lane_k(it), K - 1);
      if (from_jitter) z_pre = ih.jitter[row + kk];
      else z_pre = ih.z_samp[row + kk], zn_pre = ih.z_samp[row + min(kk + 1, K - 1)];
    };
    const int g_next = DYN ? g_nx : group_of(idx + waves_per_xcd);   // (DYN: the successor may be a claimed group, see `next_group`)
    if (!pk48 && g_next >= 0) prefetch_z(g_next, 0);
    if constexpr (ONE_RAY) {
      if (g_next >= 0) nrec = ih.rays[(long)g_next * 8 + (lane & 7)];
    }

    float T_carry = 1.0f, depth_part = 0.0f, w_part = 0.0f;
    float Tc_D = 1.0f;   // 48-lane mode: transmittance in front of the fourth ray's current row
    float rgb_part[NVMAX * 3];
#pragma unroll
    for (int i = 0; i < NVMAX * 3; ++i) rgb_part[i] = 0.0f;

    OutP o_rgb = nullptr, o_depth = nullptr;   // (read in the chunk loop with the other output pointers, used behind it as well)
    int white_bkgd = 0;
    for (int kc = 0; kc < (pk48 ? 192 : K); kc += 64) {
      const int it = kc >> 6;
      const int k = pk48 ? lane_k(it) : kc + kl;
      const bool valid = k < K;
      if (pk48) {
        ray = lane_ray(g, it);
        zrow = zsrc + ray * K;
        if (it > 0) z_cur = z_pre, zn_cur = zn_pre;
        if (it < 2) prefetch_z(g, it + 1);
        else if (g_next >= 0) prefetch_z(g_next, 0);
        if (mainl && it > 0) {   // lanes 0-47 start a new ray
          depth_part = 0.0f, w_part = 0.0f;
#pragma unroll
          for (int i = 0; i < NVMAX * 3; ++i) rgb_part[i] = 0.0f;
        }
      }
      // The weights in LDS are the same for every ray: without this the compiler hoists all ~150 weight reads out of the persistent
      // loop and keeps them in VGPRs (then spills the gather buffers).  Make the LDS offsets opaque per iteration.
      int lane_off = lane_off0, h = h0;
      asm volatile("" : "+v"(lane_off), "+v"(h));
      if (kc > 0 && !pk48) {
        const int kk = valid ? k : K - 1;
        z_cur = zrow[kk];
        if (!from_jitter) zn_cur = zrow[min(kk + 1, K - 1)];
      }
      if (from_jitter) {
        // NeRFRenderer.sample_coarse in here (nerf.py:103-123; bit-identical to bts_sample_coarse: the same routine): one launch and
        // 8 B per sample of HBM traffic less per render.  The next sample's depth is the neighbour lane's (rays of more than 64
        // samples: computed from its own jitter, the neighbour of lane 63 belongs to the next chunk).
        const int kk = valid ? k : K - 1;
        const bool lindisp = BTS_PIN(PinnedSet::lindisp, q->lindisp) != 0;
        z_cur = coarse_depth(z_cur, (kc == 0 && !pk48) ? base0 : coarse_base(K, kk), step0, near, far, lindisp);
        zn_cur = dpp_f<kDppWaveShl1>(z_cur, z_cur);
        if (K > 64 || pk48) zn_cur = coarse_depth(zrow[min(kk + 1, K - 1)], coarse_base(K, min(kk + 1, K - 1)), step0, near, far, lindisp);
        if (BTS_PIN(false, q->z_out != nullptr) && valid) q->z_out[ray * K + k] = z_cur;
      }
      const float z = z_cur, z_nx = zn_cur;
      // nerf.py:231  points = o + z * d   (mul, then add)
      const float px = ox + z * dx, py = oy + z * dy, pz = oz + z * dz;
      if constexpr (!ONE_RAY) {
        if (pk48 && it < 2) {   // the next iteration's ray (lanes 0-47 change theirs): its registers are free from here on
          const long rn = lane_ray(g, it + 1);
          const float4 r0 = reinterpret_cast<const float4*>(ih.rays)[rn * 2];
          const float4 r1 = reinterpret_cast<const float4*>(ih.rays)[rn * 2 + 1];
          ox = r0.x, oy = r0.y, oz = r0.z, dx = r0.w, dy = r1.x, dz = r1.y, near = r1.z, far = r1.w;
        }
      }

      // ---------------- encoder view: projection, taps, depth code
      const int code_mode = BTS_PIN(PinnedSet::code_mode, ih.code_mode);
      const Proj pe = code_mode == 1 ? project<true>(enc, px, py, pz) : project<false>(enc, px, py, pz);
      Taps tp = make_taps(pe.x, pe.y, H, W, fs);
      int s00 = 0, s01 = 0, s10 = 0;   // the taps of lane 0's sample, wave-uniform
      if constexpr (kTwoLoops) {
        s00 = __builtin_amdgcn_readfirstlane(tp.o00), s01 = __builtin_amdgcn_readfirstlane(tp.o01), s10 = __builtin_amdgcn_readfirstlane(tp.o10);
        // (lanes k >= K evaluate sample K - 1 again; rays of more than 64 samples stay in the general loop)
        // probe builds, ablate bit 64: EVERY ray takes the shared loop (timing only: wrong rows for rays that do not share their texels)
        const bool shared_ray = K <= 64 && (BTS_ABL(64) || __all((tp.o00 == s00) & (tp.o01 == s01) & (tp.o10 == s10)));
        if (shared_ray != SHARED) {
          nrec = nrec_in, z_pre = z_pre_in, zn_pre = zn_pre_in;
          other_loop = true;
          break;
        }
      }
      float v3[3];
      v3[0] = pe.x, v3[1] = pe.y;
      v3[2] = depth_code(pe, code_mode == 1, BTS_PIN(PinnedSet::inv_z, ih.inv_z) != 0, ih.inv_dmax, ih.inv_range, ih.d_min, ih.range);
      const bool use_empty = (BTS_PIN(PinnedSet::learn_empty, ih.learn_empty) != 0) & pe.invalid;
      const Taps tp_enc = tp;   // as grid_sample has them: a render view that IS the encoder view (FwdParams::enc_view) takes its colour taps from here
      if (use_empty) tp.w00 = tp.w01 = tp.w10 = tp.w11 = 0.0f;  // the empty feature is added after the blend
      tp.w00 *= scale, tp.w01 *= scale, tp.w10 *= scale, tp.w11 *= scale;  // exact: power of two

      float col[NVMAX * 3];
      bool inv[NVMAX];

      // ---------------- tap weights of both point tiles on every lane.  (`o`, the offsets, is read by nothing -- they go through the tap
      // table in LDS -- and costs no instruction, but without its four broadcasts hipcc numbers the tap weights' registers differently
      // in the two-loop kernels: it leaves with the next change that moves those kernels' instruction streams anyway.)
      int o[2][4];
      float wq[2][4];
      bool emp[2];
      {
        unsigned t0, t1;
        bcast_tiles((unsigned)tp.o00, t0, t1), o[0][0] = (int)t0, o[1][0] = (int)t1;
        bcast_tiles((unsigned)tp.o01, t0, t1), o[0][1] = (int)t0, o[1][1] = (int)t1;
        bcast_tiles((unsigned)tp.o10, t0, t1), o[0][2] = (int)t0, o[1][2] = (int)t1;
        bcast_tiles((unsigned)tp.o11, t0, t1), o[0][3] = (int)t0, o[1][3] = (int)t1;
        bcast_tiles(__float_as_uint(tp.w00), t0, t1), wq[0][0] = __uint_as_float(t0), wq[1][0] = __uint_as_float(t1);
        bcast_tiles(__float_as_uint(tp.w01), t0, t1), wq[0][1] = __uint_as_float(t0), wq[1][1] = __uint_as_float(t1);
        bcast_tiles(__float_as_uint(tp.w10), t0, t1), wq[0][2] = __uint_as_float(t0), wq[1][2] = __uint_as_float(t1);
        bcast_tiles(__float_as_uint(tp.w11), t0, t1), wq[0][3] = __uint_as_float(t0), wq[1][3] = __uint_as_float(t1);
        bcast_tiles(use_empty ? 1u : 0u, t0, t1), emp[0] = t0 != 0, emp[1] = t1 != 0;
      }


      float s_raw;
      if (__builtin_expect(__any(pe_needs_exact(v3, ih.freq_factor)), 0)) {
        s_raw = eval_point_exact<C, HD, NB>(lds, G, q->w2c_enc + sample * 16, q->K_enc + sample * 9, H, W, fs, q->code_mode, q->inv_z, q->inv_dmax,
                                            q->inv_range, q->d_min, q->range, q->freq_factor, q->learn_empty, b_out, px, py, pz);
      } else {
      BTS_TICK(0)
      // ---------------- h = bilinear(G) + W_pe . PE + b: gather three blocks ahead, blend between the octaves
      f32x16 acc[HT][2];
      unsigned off_next[4];
      GRows rows;
      GTapRegs taps;   // PINNED: the general loop's tap table rows in registers (gl_read_taps); nothing touches it anywhere else
      if constexpr (SHARED) {
        gs_issue<HD>(gl, G, (unsigned)s00 * (HD * 4u), (unsigned)s01 * (HD * 4u), (unsigned)s10 * (HD * 4u), lane);
      } else {
        // tap table of the wave's 64 samples (byte offsets into G), lane = sample
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        gl.tab[lane * 3 + 0] = (unsigned)tp.o00 * (HD * 4u), gl.tab[lane * 3 + 1] = (unsigned)tp.o01 * (HD * 4u), gl.tab[lane * 3 + 2] = (unsigned)tp.o10 * (HD * 4u);   // o11 = o10 + (o01 - o00)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        gl_prologue<HD, PINNED>(gl, rows, G, off_next, &taps);
      }
      {
        // bias row (times 2^S, fp32): the C operand of the first MFMA of every accumulator tile.  The raw inputs x, y, code ride in
        // the spare k rows of the f16 slices (|x|, |y| <= 2083 here -- beyond that the wave took the exact path above), so the
        // fp32-input MFMAs, which block the VALU for 64 cycles each, are gone from this path.
        f32x16 bias[HT];
        {
          const float* bl = lh + LH::W_RAW + 3 * HD + 4 * h;
#pragma unroll
          for (int ht = 0; ht < HT; ++ht)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float4 v = *reinterpret_cast<const float4*>(bl + ht * 32 + 8 * j);
              bias[ht][4 * j + 0] = v.x, bias[ht][4 * j + 1] = v.y, bias[ht][4 * j + 2] = v.z, bias[ht][4 * j + 3] = v.w;
            }
        }
        SinCos3 raw;
        pe_direct(raw, v3, ih.freq_factor);
        __builtin_amdgcn_sched_barrier(0);
        int lane4 = lane * 4;
        asm volatile("" : "+v"(lane4));  // keep the A-operand reads inside the loop (see lane_off above)
        region_seq_l<HD, 0, SHARED, PINNED>(acc, gl, rows, G, wq, off_next, lh + LH::W_F16 + lane4, LH::TERM_STRIDE, raw, v3, ih.freq_factor, bias, h, &taps);
        if constexpr (NS > kNumFreqs) {   // HD = 64: the last four blocks
          g_step<HD, 12, SHARED, PINNED>(acc, gl, rows, G, wq, off_next, h, &taps), g_step<HD, 13, SHARED, PINNED>(acc, gl, rows, G, wq, off_next, h, &taps);
          g_step<HD, 14, SHARED, PINNED>(acc, gl, rows, G, wq, off_next, h, &taps), g_step<HD, 15, SHARED, PINNED>(acc, gl, rows, G, wq, off_next, h, &taps);
        }
      }
      if (BTS_PIN(PinnedSet::learn_empty, q->learn_empty) && __any(use_empty)) {
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float ev = lh[LH::EMPTY + ht * 32 + mfma_row(q, 0) + 4 * h];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) acc[ht][pt][q] += emp[pt] ? ev : 0.0f;
          }
      }

      // ---------------- ResnetBlockFC layers: h = h + fc_1(relu(fc_0(relu(h))))   (resnetfc.py:53-62)
      int lane4b = lane * 4;
      asm volatile("" : "+v"(lane4b));   // keep the weight reads inside the persistent loop (see lane_off)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float* base = lds + L::BLK + b * L::BLK_STRIDE;
        f32x16 net[HT][2];
#pragma unroll
        for (int ot = 0; ot < HT; ++ot)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = ot * 32 + mfma_row(q, 0) + 4 * h;
            const float bias = lh[LH::BIAS + b * 2 * HD + row];
            net[ot][0][q] = bias, net[ot][1][q] = bias;
          }
        if constexpr (HD == 32) hidden_layer_h(net, acc, lh + LH::W_BLK + (2 * b) * LH::BLK_LAYER_STRIDE + lane4b, LH::BLK_TERM_STRIDE, inv_scale);
        else hidden_layer<HD>(net, acc, base, lane);
#pragma unroll
        for (int ot = 0; ot < HT; ++ot)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = ot * 32 + mfma_row(q, 0) + 4 * h;
            const float bias = lh[LH::BIAS + b * 2 * HD + HD + row];
            acc[ot][0][q] += bias, acc[ot][1][q] += bias;
          }
        if constexpr (HD == 32) hidden_layer_h(acc, net, lh + LH::W_BLK + (2 * b + 1) * LH::BLK_LAYER_STRIDE + lane4b, LH::BLK_TERM_STRIDE, inv_scale);
        else hidden_layer<HD>(acc, net, base + HD * HD + HD, lane);
      }

      BTS_TICK(1)
      // ---------------- lin_out: in-lane dot over the hidden rows this lane holds, then fold the two lane halves
      float p0 = 0.0f, p1 = 0.0f;
      if (BTS_ABL(32)) {
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) p0 += acc[ht][0][0] + acc[ht][0][5] + acc[ht][0][15], p1 += acc[ht][1][0] + acc[ht][1][5] + acc[ht][1][15];
      } else {
        // both point tiles' running sums as ONE packed FMA per hidden row (the same two chains p0, p1 as scalar code: order unchanged)
        f32x2 pp = {0.0f, 0.0f};
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float w2 = lds[L::W_OUT + ht * 32 + mfma_row(q, 0) + 4 * h];
            // w2 as src0: a broadcast from an odd register in src1 is the gfx950 op_sel erratum (tools/check_pk_opsel.py)
            pp = __builtin_elementwise_fma((f32x2){w2, w2}, (f32x2){relu1(acc[ht][0][q]), relu1(acc[ht][1][q])}, pp);
          }
        p0 = pp[0], p1 = pp[1];
      }
      swap32(p0, p1);  // p0 = {tile0.lo, tile1.lo}, p1 = {tile0.hi, tile1.hi}: lane l now holds both halves of ITS sample
      s_raw = __builtin_fmaf(p0 + p1, inv_scale, b_out);
      }
      float sigma = softplus(s_raw);
      if (BTS_PIN(PinnedSet::empty_empty, q->empty_empty)) sigma = pe.invalid ? 0.0f : sigma;
      if (BTS_PIN(false, q->sigma_noise != nullptr)) sigma += q->sigma_noise[ray * K + min(k, K - 1)];   // nerf.py:279-280, the caller drew it
      BTS_TICK(2)

      // ---------------- the iteration's ten output pointers in ONE batch of scalar loads (they are neighbours in the kernarg segment),
      // issued here so that the round trip runs under the colour taps.  Read where they are used -- each inside its own `if (pointer)` --
      // they were ten dependent load / wait / branch steps behind each other in the store section (profiles/r04t: 3.8 k of the training
      // forward's 28 k cycles per iteration).
      // (PINNED: the five arrays of the pinned set, as global pointers -- the stores are global_store with a scalar base, not flat stores
      // with a 64-bit address per lane that also count on lgkmcnt; the other five are null by the set and are not read)
      o_rgb = (OutP)q->rgb, o_depth = (OutP)q->depth, white_bkgd = BTS_PIN(PinnedSet::white_bkgd, q->white_bkgd);
      OutP o_weights = (OutP)q->weights, o_alphas = (OutP)q->alphas, o_invalid = (OutP)q->invalid;
      float *o_rgb_samps = BTS_PIN((float*)nullptr, q->rgb_samps), *o_sigma_raw = BTS_PIN((float*)nullptr, q->sigma_raw);
      float *o_trans = BTS_PIN((float*)nullptr, q->trans), *o_iw = BTS_PIN((float*)nullptr, q->invalid_wsum), *o_ia = BTS_PIN((float*)nullptr, q->invalid_any);
      if constexpr (PINNED) asm volatile("" : "+s"(o_rgb), "+s"(o_depth), "+s"(o_weights), "+s"(o_alphas), "+s"(o_invalid));
      else
      asm volatile("" : "+s"(o_rgb), "+s"(o_depth), "+s"(o_weights), "+s"(o_alphas), "+s"(o_invalid), "+s"(o_rgb_samps), "+s"(o_sigma_raw), "+s"(o_trans),
                   "+s"(o_iw), "+s"(o_ia));

      // ---------------- colours (models_bts.py:218-264): projection into each render view + 4-tap fetch of the rgb0-packed frame.
      // Issued here, after lin_out, rather than before the MFMA phase: the taps' registers are not live across the accumulators
      // (0 spilled VGPRs, 5 % faster).  Round 1 had this order fail parity for nv <= 2 -- that was the packed-FP32 operand-select
      // erratum of gfx950 (tools/ubench/pk_opsel_lanes.hip), not the order; see DESIGN.md section 3.
      // All views of a batch (four at a time) go through the three phases together -- cameras + projections + taps, then the 4 x 4
      // texel loads, then the blends: view after view, each view's loads were waited for before the next view's went out (one memory
      // round trip per view: 25 % of the training forward's iteration at nv = 4, profiles/r04t).  Views beyond nv repeat view nv - 1 so
      // that no branch sits between the loads (a uniform branch per view splits them into blocks the scheduler cannot merge); their
      // results are dropped.
#pragma unroll
      for (int j = 0; j < NVMAX; ++j) col[3 * j] = col[3 * j + 1] = col[3 * j + 2] = 0.0f, inv[j] = pe.invalid;
      if (nv > 0 && !BTS_ABL(8)) {
#pragma unroll
        for (int j0 = 0; j0 < NVMAX; j0 += 4) {
          constexpr int NB4 = NVMAX < 4 ? NVMAX : 4;
          Taps tcs[NB4];
          bool invs[NB4];
#pragma unroll
          for (int b = 0; b < NB4; ++b) {
            const int jj = min(j0 + b, nv - 1);   // uniform
            tcs[b] = tp_enc, invs[b] = pe.invalid;
            if (jj != BTS_PIN(PinnedSet::enc_view, q->enc_view)) {   // wave-uniform
              const Cam cj = load_cam(q->w2c_r + ((long)sample * nv + jj) * 16, q->K_r + ((long)sample * nv + jj) * 9);
              const Proj pc = project<false>(cj, px, py, pz);
              tcs[b] = make_taps(pc.x, pc.y, H, W);
              invs[b] = pc.invalid | pe.invalid;
            }
          }
          float4 tex[NB4][4];
#pragma unroll
          for (int b = 0; b < NB4; ++b) {
            const float4* img = reinterpret_cast<const float4*>(q->imgs) + ((long)sample * nv + min(j0 + b, nv - 1)) * H * W;
            tex[b][0] = img[tcs[b].o00], tex[b][1] = img[tcs[b].o01], tex[b][2] = img[tcs[b].o10], tex[b][3] = img[tcs[b].o11];
          }
          if constexpr (NB4 > 1) __builtin_amdgcn_sched_barrier(0);   // every load of the batch is out before the first blend
#pragma unroll
          for (int b = 0; b < NB4; ++b) {
            const int j = j0 + b;
            const Taps& tc = tcs[b];
            const float4 a = tex[b][0], bb = tex[b][1], cc = tex[b][2], d = tex[b][3];
            const float c0 = ((a.x * tc.w00 + bb.x * tc.w01) + cc.x * tc.w10) + d.x * tc.w11;
            const float c1 = ((a.y * tc.w00 + bb.y * tc.w01) + cc.y * tc.w10) + d.y * tc.w11;
            const float c2 = ((a.z * tc.w00 + bb.z * tc.w01) + cc.z * tc.w10) + d.z * tc.w11;
            if (j < nv) col[3 * j + 0] = c0, col[3 * j + 1] = c1, col[3 * j + 2] = c2, inv[j] = invs[b];
          }
        }
      }

      // ---------------- alpha compositing (nerf.py:225-299): segmented DPP scan over the lanes of each ray
      const float delta = (k + 1 < K) ? (z_nx - z) : 1e10f;
      float alpha = 1.0f - transmittance(delta, sigma);
      if (BTS_PIN(PinnedSet::hard_cap, q->hard_cap) && k == K - 1) alpha = 1.0f;
      const float t = valid ? (1.0f - alpha) + 1e-10f : 1.0f;
      const float incl = seg_scan_mul(t, lpr, kl);
      float excl = dpp_f<kDppWaveShr1>(1.0f, incl);
      if (kl == 0) excl = 1.0f;   // (48-lane mode: lanes 0 and 48)
      const float T = (pk48 ? (mainl ? 1.0f : Tc_D) : T_carry) * excl;
      if (pk48) Tc_D = Tc_D * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
      if (ONE_RAY && K > 64) T_carry = T_carry * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
      const float wgt = valid ? alpha * T : 0.0f;
      BTS_TICK(3)
      // ---------------- per-ray reductions for the loss' invalid-ray policies (loss.py:100-118), instead of weights + invalid in HBM
      if constexpr (EPI) {
        // every view's sum and flag first (no branch between the scans), then ONE block of stores on the ray's last lane: view after
        // view -- scan, ballot, lane branch, two pointer branches, two one-lane stores -- was 16 branches per iteration at nv = 4
        float ws[NVMAX], any[NVMAX];
        const unsigned long long seg = pk48 ? (mainl ? 0x0000FFFFFFFFFFFFull : 0xFFFF000000000000ull)
                                            : (lpr == 64 ? ~0ull : (((1ull << lpr) - 1ull) << ((lane | (lpr - 1)) - (lpr - 1))));
#pragma unroll
        for (int j = 0; j < NVMAX; ++j) {
          ws[j] = seg_scan_add((valid && inv[j]) ? wgt : 0.0f, lpr, kl);       // the last lane of each ray has the sum
          const unsigned long long hit = __ballot(valid && inv[j]);
          any[j] = (hit & seg) ? 1.0f : 0.0f;
        }
        if (pk48 ? (lane == 47 || lane == 63) : kl == lpr - 1) {
          const bool more = pk48 ? (!mainl && it > 0) : kc > 0;   // K > 64: chunk after chunk; 48-lane mode: the fourth ray's rows
          const long idx = ray * nv;
          if (nv == NVMAX && NVMAX % 4 == 0 && !more) {   // the common case: whole rows, nothing to merge with
#pragma unroll
            for (int j4 = 0; j4 < NVMAX / 4; ++j4) {
              if (o_iw) reinterpret_cast<float4*>(o_iw + idx)[j4] = make_float4(ws[4 * j4], ws[4 * j4 + 1], ws[4 * j4 + 2], ws[4 * j4 + 3]);
              if (o_ia) reinterpret_cast<float4*>(o_ia + idx)[j4] = make_float4(any[4 * j4], any[4 * j4 + 1], any[4 * j4 + 2], any[4 * j4 + 3]);
            }
          } else {
#pragma unroll
            for (int j = 0; j < NVMAX; ++j)
              if (j < nv) {
                if (o_iw) o_iw[idx + j] = (more ? o_iw[idx + j] : 0.0f) + ws[j];
                if (o_ia) o_ia[idx + j] = more ? fmaxf(o_ia[idx + j], any[j]) : any[j];
              }
          }
        }
      }
      depth_part = depth_part + wgt * z;
      w_part = w_part + wgt;
#pragma unroll
      for (int i = 0; i < NVMAX * 3; ++i) rgb_part[i] = rgb_part[i] + wgt * col[i];
      if (valid && !BTS_ABL(16)) {
        const long pk = ray * K + k;
        if constexpr (PINNED) {
          // weights, alphas and invalid of the pinned set: the ray's row is the scalar base and the lane's sample a 32-bit offset, the same
          // register for the three arrays (base[pk] is a 64-bit address per lane and array).  Nontemporal: 189 MB per eval frame that the
          // kernel never reads again, through the L2 slices that hold G (measured on its own: profiles/r20a)
          __builtin_nontemporal_store(wgt, &(o_weights + ray * K)[(unsigned)k]), __builtin_nontemporal_store(alpha, &(o_alphas + ray * K)[(unsigned)k]);
          __builtin_nontemporal_store(inv[0] ? 1.0f : 0.0f, &(o_invalid + ray * K)[(unsigned)k]);
        }
        if (BTS_PIN(false, o_weights != nullptr)) o_weights[pk] = wgt;
        if (BTS_PIN(false, o_alphas != nullptr)) o_alphas[pk] = alpha;
        if (o_sigma_raw) o_sigma_raw[pk] = s_raw;
        if (o_trans) o_trans[pk] = T;
        if (BTS_PIN(false, o_invalid != nullptr)) {
#pragma unroll
          for (int j = 0; j < NVMAX; ++j)
            if (j < nv) o_invalid[pk * nv + j] = inv[j] ? 1.0f : 0.0f;
        }
        if (o_rgb_samps) {
          // a sample's nv * 3 colours are contiguous: with every view present they leave as 16- (or 8-) byte pieces -- as 4-byte stores
          // 48 bytes apart between lanes, every instruction touched 24 lines for 4 bytes each (12 of them per sample at nv = 4)
          float* dst = o_rgb_samps + pk * (nv * 3);
          if (nv == NVMAX && (NVMAX * 3) % 4 == 0) {
#pragma unroll
            for (int i = 0; i < NVMAX * 3 / 4; ++i)
              reinterpret_cast<float4*>(dst)[i] = make_float4(col[4 * i], col[4 * i + 1], col[4 * i + 2], col[4 * i + 3]);
          } else if (nv == NVMAX && (NVMAX * 3) % 2 == 0) {
#pragma unroll
            for (int i = 0; i < NVMAX * 3 / 2; ++i) reinterpret_cast<float2*>(dst)[i] = make_float2(col[2 * i], col[2 * i + 1]);
          } else {
#pragma unroll
            for (int i = 0; i < NVMAX * 3; ++i)
              if (i < nv * 3) dst[i] = col[i];
          }
        }
      }
      if (pk48) {
        // per-ray sums of this iteration: lane 47 has the totals of lanes 0-47's ray; lane 63 those of the fourth ray's rows so far
        // (its lanes keep accumulating), written after its last row
        const float dsum = seg_scan_add(depth_part, 48, kl), wsum = seg_scan_add(w_part, 48, kl);
        float csum[NVMAX * 3];
#pragma unroll
        for (int i = 0; i < NVMAX * 3; ++i) csum[i] = i < nv * 3 ? seg_scan_add(rgb_part[i], 48, kl) : 0.0f;
        if (lane == 47 || (lane == 63 && it == 2)) {
          o_depth[ray] = dsum;
#pragma unroll
          for (int i = 0; i < NVMAX * 3; ++i)
            if (i < nv * 3) o_rgb[ray * nv * 3 + i] = white_bkgd ? (csum[i] + 1.0f) - wsum : csum[i];  // nerf.py:301-304
        }
      }
    }
    if constexpr (kTwoLoops) {
      if (other_loop) break;   // leaves the loop of the including kernel WITHOUT advancing: the other loop takes the ray
    }
    BTS_TICK(4)
    // ---------------- per-ray sums: the last lane of each ray ends up with the totals
    if (!pk48) {
      depth_part = seg_scan_add(depth_part, lpr, kl);
      w_part = seg_scan_add(w_part, lpr, kl);
#pragma unroll
      for (int i = 0; i < NVMAX * 3; ++i)
        if (i < nv * 3) rgb_part[i] = seg_scan_add(rgb_part[i], lpr, kl);
      if (kl == lpr - 1) {
        o_depth[ray] = depth_part;
        float out[NVMAX * 3];
#pragma unroll
        for (int i = 0; i < NVMAX * 3; ++i) out[i] = white_bkgd ? (rgb_part[i] + 1.0f) - w_part : rgb_part[i];  // nerf.py:301-304
        if (nv == NVMAX && (NVMAX * 3) % 4 == 0) {   // one lane, whole row: 16-byte stores
#pragma unroll
          for (int i = 0; i < NVMAX * 3 / 4; ++i)
            store4(o_rgb + ray * (NVMAX * 3) + 4 * i, make_float4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]));
        } else {
#pragma unroll
          for (int i = 0; i < NVMAX * 3; ++i)
            if (i < nv * 3) o_rgb[ray * nv * 3 + i] = out[i];
        }
      }
    }
    BTS_TICK(5)
}
#undef BTS_ITER_SHARED
