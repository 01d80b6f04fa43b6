// The body of the projection G = F . w_in[:, :C]^T (bts_prep.hip: project_kernel), included where it runs -- like bts_render_iter.h, text
// and not a function, so that project_kernel stays the instruction stream it was: in project_kernel itself, a grid of its own, and in
// the evaluation frame's prep launch (bts_aux.hip: eval_prep_kernel), whose first work-groups take this role.
// The including scope names: C, HD, FEAT_CL (compile-time); float* wl (C * HD floats of LDS: wl[c*HD + s] = w_in[hidden_of_storage(s)][c],
// G comes out in its storage channel order); feat, mlp (lin_in's weight, (HD, C + kPeDim) row-major: the head of the packed parameter
// vector or the nn.Linear's own tensor), proj, HW, tiles_per_img, n_tiles, tiles, Wm, tw, list as project_kernel's parameters; and the
// macros BTS_PROJ_BLOCK / BTS_PROJ_BLOCKS: this work-group's index among the work-groups of the role, and their number.
// No include guard: one inclusion per including function.
  constexpr int HT = HD / 32;
  constexpr int D_IN = C + kPeDim;
  for (int i = threadIdx.x; i < C * HD; i += blockDim.x) {
    const int c = i / HD, st = i % HD;
    wl[i] = mlp[proj_hidden_of_storage(st) * D_IN + c];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, col = lane & 31;
  // `tiles` (bts_project_features_tiles): only the flagged tiles are computed -- a training step's samples read 38 % of them
  // (exp_kitti_360.yaml's batch), the rest of the map is never looked at and stays as it is.  A tile's flag is fetched one tile ahead.
  // `list` (bts_train_step_fwd, large maps): the flagged tiles as a compact list (compact_tiles_kernel), dealt round-robin -- every wave
  // the same number of tiles to within one instead of a binomial share of the flags it happens to walk over
  const int tile0 = BTS_PROJ_BLOCK * 4 + wave, tstride = BTS_PROJ_BLOCKS * 4;
  const int n_work = list ? min(n_tiles, list[0]) : n_tiles;
  int flag_n = list ? (tile0 < n_work ? list[4 + tile0] : 0) : ((tiles && tile0 < n_tiles) ? (int)tiles[tile0] : 1);
  for (int it = tile0; it < n_work; it += tstride) {   // tile = 64 pixels of one image
    const int fetched = __builtin_amdgcn_readfirstlane(flag_n);
    flag_n = list ? (it + tstride < n_work ? list[4 + it + tstride] : 0) : ((tiles && it + tstride < n_tiles) ? (int)tiles[it + tstride] : 1);
    if (!list && fetched == 0) continue;
    const int tile = list ? fetched : it;
    const int img = tile / tiles_per_img;
    // slot i of the tile is texel p0 + i + (i >> 4) * rs of the image (bts_common.h: a 16 x 4 block, or 64 consecutive texels with rs = 0)
    const int p0 = tile_base(tile - img * tiles_per_img, Wm, tw), rs = tile_rs(Wm, tw);
    const int px0 = p0 + col + (col >> 4) * rs, px1 = p0 + 32 + col + ((32 + col) >> 4) * rs;   // this lane's texels of the two point tiles
    const float* F = feat + (long)img * C * HW;
    float* G = proj + (long)img * HW * HD;
    f32x16 acc[2][HT];
    if constexpr (FEAT_CL) {
      const float4* F4 = reinterpret_cast<const float4*>(F);
      const unsigned q0 = (unsigned)(min(px0, HW - 1) * (C / 4) + h), q1 = (unsigned)(min(px1, HW - 1) * (C / 4) + h);
      float4 v0[C / 8], v1[C / 8];
#pragma unroll
      for (int q = 0; q < C / 8; ++q) v0[q] = F4[q0 + 2 * q], v1[q] = F4[q1 + 2 * q];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) acc[pt][ht] = zero_acc();
#pragma unroll
      for (int q = 0; q < C / 8; ++q) {
        const float* a0 = reinterpret_cast<const float*>(&v0[q]);
        const float* a1 = reinterpret_cast<const float*>(&v1[q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 8 * q + 4 * h + e;
#pragma unroll
          for (int ht = 0; ht < HT; ++ht) {
            const float b = wl[c * HD + ht * 32 + col];
            acc[0][ht] = mfma(a0[e], b, acc[0][ht]);
            acc[1][ht] = mfma(a1[e], b, acc[1][ht]);
          }
        }
      }
    } else {
    // wave-uniform base + 32-bit lane offset (one image's map is far below 4 GB): scalar-base loads, no 64-bit address per load
    const unsigned o0 = (unsigned)(h * HW + min(px0, HW - 1)), o1 = (unsigned)(h * HW + min(px1, HW - 1));
    float a0[C / 2], a1[C / 2];
#pragma unroll
    for (int s = 0; s < C / 2; ++s) {
      const float* row = F + (long)(2 * s) * HW;   // uniform
      a0[s] = row[o0], a1[s] = row[o1];
    }
    __builtin_amdgcn_sched_barrier(0);   // the scheduler otherwise sinks every load to its MFMA (two loads in flight, measured 2.9 TB/s)
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) acc[pt][ht] = zero_acc();
#pragma unroll
    for (int s = 0; s < C / 2; ++s) {
      const int c = 2 * s + h;
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
        const float b = wl[c * HD + ht * 32 + col];
        acc[0][ht] = mfma(a0[s], b, acc[0][ht]);
        acc[1][ht] = mfma(a1[s], b, acc[1][ht]);
      }
    }
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int pix = tile_px_c(p0, pt * 32 + mfma_row(q, 0), 4 * h, rs);   // mfma_row(q, h) = mfma_row(q, 0) + 4 h, (.. & 15) <= 11
        if (pix < HW) {
#pragma unroll
          for (int ht = 0; ht < HT; ++ht) G[(unsigned)(pix * HD + ht * 32 + col)] = acc[pt][ht][q];
        }
      }
  }
#undef BTS_PROJ_BLOCK
#undef BTS_PROJ_BLOCKS
