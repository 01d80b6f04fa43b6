// MLP-predicted colour (BTSNet with sample_color=False, models_bts.py:41-42, 315-321): the field's MLP has four outputs,
// sigma = relu(o0) and rgb = sigmoid(o1..3), there are no colour taps and nv = 1 (the PixelNeRF-style head).
//
// Three kernels, lane = SAMPLE (or point), fp32 throughout, weights read through the constant address space (wave-uniform s_loads):
//   mc_render_kernel   one work-group = R = 256 / K whole rays: every lane evaluates one sample (projection, bilinear G, encoding,
//                      lin_in, blocks, the four-row lin_out), one lane per ray composites front to back from LDS.
//   mc_query_kernel    one lane = one query point (bts_field_query_mlp_color).
//   mc_rows_kernel     pass A of the backward (the row form of bts_bwd_blocks.hip, rowsb_kernel's role): the compositing gradient as a
//                      per-ray suffix recurrence, g_o = (dL/do0, dL/do1..3) per sample, the MLP backward in registers, and per sample
//                      u0 = dL/d(lin_in output) in G's storage order plus the liveness slot g_s = max_o |g_o| (0 exactly when the sample
//                      contributes nothing; NOT dL/do0: a sample with a dead density and a live colour must still reach pass B).  lin_out's
//                      and the blocks' weight gradients are contracted per work-group through LDS, once per 256 samples.
// Passes B (scatter_kernel<HD, true>: dG += w_tap u0) and C (dwpe_rows_kernel: dW_pe, db_in) of bts_bwd_rows.hip run unchanged on
// what pass A leaves.  Replaces nerf.py:210-313 + models_bts.py:266-338 (sample_color=False) + resnetfc.py:132-184 of the reference.
// The MLP and its backward, a sample's alpha, the sums along a ray, the kernels' parameters and passes B and C's launches are
// bts_mc_field.h's, shared with bts_multi_view.hip; this file holds the head's own: the field of one encoder view (mc_field), the sigmoid
// colours and their gradient, and the workspace.
#include "bts_mc_field.h"

namespace bts {

constexpr int kMcOut = 4;         // lin_out rows: density + three colour channels

template <int C, int HD, int NB>
__device__ __forceinline__ void mc_field(const FwdParams& p, const Cam& enc, int sample, float px, float py, float pz, const float* empty_proj,
                                         McAct<C, HD, NB>& a, float (&o)[kMcOut], bool& invalid) {
  const cfp w = as_const(p.mlp);
  const Proj pe = p.code_mode == 1 ? project<true>(enc, px, py, pz) : project<false>(enc, px, py, pz);
  invalid = pe.invalid;
  float v3[3];
  v3[0] = pe.x, v3[1] = pe.y;
  v3[2] = depth_code(pe, p.code_mode == 1, p.inv_z != 0, p.inv_dmax, p.inv_range, p.d_min, p.range);
  // bilinear(G), or the projected empty feature
  if (p.learn_empty && pe.invalid) {
#pragma unroll
    for (int j = 0; j < HD; ++j) a.h0[j] = empty_proj[j];
  } else {
    const Taps tp = make_taps(pe.x, pe.y, p.H, p.W, p.fs);
    const long plane = (long)(p.H >> p.fs) * (p.W >> p.fs);
    mc_bilinear<HD, true>(a.h0, p.proj + (long)sample * plane * HD, tp, 1.0f);
  }
  float enc_in[kPeDim];
  mc_encode(enc_in, v3, p.freq_factor);
  mc_mlp<C, HD, NB, kMcOut>(w, enc_in, a, o);
}

__device__ __forceinline__ float mc_sigmoid(float s) { return sigmoidf(s); }

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mc_render_kernel(const McParams mp) {
  const FwdParams& p = mp.f;
  __shared__ float s_empty[HD];
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_c[kMcThreads][3], s_T[kMcThreads];
  mc_stage_empty<C, HD>(s_empty, p);
  const int K = p.K;
  const long ray0 = (long)blockIdx.x * mp.R;
  const int tid = threadIdx.x;
  const McLane ln = mc_lane(mp, ray0, s_z, [&](long ray, int k) { return mc_depth(p, ray, k); });
  const long i = ln.ray * K + ln.k;
  __syncthreads();
  float o[kMcOut] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool invalid = false;
  if (ln.live) {
    const int sample = (int)(ln.ray / p.Bp);
    const Cam enc = load_cam_v(p.w2c_enc + sample * 16, p.K_enc + sample * 9);
    const float* rr = p.rays + ln.ray * 8;
    const float z = ln.z;
    McAct<C, HD, NB> act;
    mc_field<C, HD, NB>(p, enc, sample, rr[0] + z * rr[3], rr[1] + z * rr[4], rr[2] + z * rr[5], s_empty, act, o, invalid);
    s_a[tid] = mc_alpha(p, s_z, ln.k, i, z, fmaxf(o[0], 0.0f), p.empty_empty && invalid).alpha;   // relu: models_bts.py:317
#pragma unroll
    for (int c = 0; c < 3; ++c) s_c[tid][c] = mc_sigmoid(o[1 + c]);
  }
  __syncthreads();
  // one lane per ray: the transmittance product and the sums
  if (mc_ray_lane(mp, ray0)) {
    const long rw = ray0 + tid;
    const int base = tid * K;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    const McRaySums sums = mc_scan(s_a, s_z, s_T, base, K, [&](int kk, float wk) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] + wk * s_c[base + kk][c];
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) p.rgb[rw * 3 + c] = p.white_bkgd ? rgb[c] + (1.0f - sums.wsum) : rgb[c];
    p.depth[rw] = sums.depth;
  }
  __syncthreads();
  if (ln.live) {
    const float T = s_T[tid], al = s_a[tid];
    if (p.weights) p.weights[i] = al * T;
    if (p.alphas) p.alphas[i] = al;
    if (p.trans) p.trans[i] = T;
    if (p.sigma_raw) p.sigma_raw[i] = o[0];
    if (p.invalid) p.invalid[i] = invalid ? 1.0f : 0.0f;
    if (p.rgb_samps) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.rgb_samps[i * 3 + c] = s_c[tid][c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// field query
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mc_query_kernel(const FwdParams p) {
  __shared__ float s_empty[HD];
  mc_stage_empty<C, HD>(s_empty, p);
  __syncthreads();
  const long P = p.Bp;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)p.n * P) return;
  const int sample = (int)(idx / P);
  const Cam enc = load_cam_v(p.w2c_enc + sample * 16, p.K_enc + sample * 9);
  const float* x = p.xyz + idx * 3;
  McAct<C, HD, NB> act;
  float o[kMcOut];
  bool invalid;
  mc_field<C, HD, NB>(p, enc, sample, x[0], x[1], x[2], s_empty, act, o, invalid);
  float sg = fmaxf(o[0], 0.0f);
  if (p.empty_empty && invalid) sg = 0.0f;
  p.q_sigma[idx] = sg;
  if (p.invalid) p.invalid[idx] = invalid ? 1.0f : 0.0f;
  if (p.rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p.rgb[idx * 3 + c] = p.only_density ? 0.0f : mc_sigmoid(o[1 + c]);   // models_bts.py:336
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward, pass A
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mc_rows_kernel(const McParams mp) {
  const FwdParams& p = mp.f;
  constexpr int ASTR = HD + 1, BSTR = HD + 1;   // mc_mlp_bwd's rows
  __shared__ float s_empty[HD];
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_t[kMcThreads], s_c[kMcThreads][3], s_go[kMcThreads][kMcOut];
  __shared__ float s_A[kMcThreads * ASTR], s_B[kMcThreads * BSTR];
  mc_stage_empty<C, HD>(s_empty, p);
  const MlpLayout ml{C + kPeDim, HD, NB};
  const cfp w = as_const(p.mlp);
  const int K = p.K;
  const int tid = threadIdx.x;
  const bool want_w = mp.d_mlp != nullptr;
  McTile<kMcOut, HD> t_out;
  McTile<HD, HD> t_w1, t_w0;
  t_out.zero(), t_w1.zero(), t_w0.zero();
  for (long grp = blockIdx.x; grp < mp.n_groups; grp += gridDim.x) {
    const long ray0 = grp * mp.R;
    __syncthreads();   // the previous iteration's LDS readers are done
    const McLane ln = mc_lane(mp, ray0, s_z, [&](long ray, int k) { return p.z_samp[ray * K + k]; });
    const long i = ln.ray * K + ln.k;
    __syncthreads();
    // ---- the sample's field, activations kept in registers
    McAct<C, HD, NB> act;
    act.zero();
    float o[kMcOut] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool invalid = false;
    if (ln.live) {
      const int sample = (int)(ln.ray / p.Bp);
      const Cam enc = load_cam_v(p.w2c_enc + sample * 16, p.K_enc + sample * 9);
      const float* rr = p.rays + ln.ray * 8;
      const float z = ln.z;
      mc_field<C, HD, NB>(p, enc, sample, rr[0] + z * rr[3], rr[1] + z * rr[4], rr[2] + z * rr[5], s_empty, act, o, invalid);
      const float o0 = p.sigma_raw[i];   // the forward's (the same value: same routine)
      const McAlpha al = mc_alpha(p, s_z, ln.k, i, z, fmaxf(o0, 0.0f), p.empty_empty && invalid);
      s_a[tid] = al.alpha;
      s_t[tid] = mc_dalpha_dsigma(p, ln.k, al);
#pragma unroll
      for (int c = 0; c < 3; ++c) s_c[tid][c] = p.rgb_samps ? p.rgb_samps[i * 3 + c] : mc_sigmoid(o[1 + c]);
    }
    __syncthreads();
    // ---- one lane per ray: back to front
    if (mc_ray_lane(mp, ray0)) {
      const long rw = ray0 + tid;
      const int base = tid * K;
      float g_rgb[3] = {0.0f, 0.0f, 0.0f}, g_bk = 0.0f;
      if (mp.g_rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g_rgb[c] = mp.g_rgb[rw * 3 + c], g_bk -= g_rgb[c];
      }
      if (!p.white_bkgd) g_bk = 0.0f;                         // rgb += 1 - sum(weights): d/dw_k = -sum(g_rgb)
      const float g_dep = mp.g_depth ? mp.g_depth[rw] : 0.0f;
      float P = 0.0f;
      // not unrolled: the second copy of an unrolled body addresses its loads from the parameter block's pointers, which this kernel keeps
      // parked in VGPR lanes: 42 lane reads per two samples in this serial loop at (32, 32, 1), 34 at (64, 64, 0).  Measured against the
      // unrolled loop (profiles/r26a/bench_pairs.txt): RE10K forward + backward 5.39 -> 5.15 ms, KITTI-raw 2.64 -> 2.63 ms.
      // mv_rows_kernel's loop stays unrolled: its copies read few parked SGPRs (0 lane reads at d_hidden 64 and at (32, 32, 0), 8 at
      // (32, 32, 1), where the parent's has 14), and not unrolled that kernel spills VGPRs at (32, 32, 1) and takes 68 bytes of scratch
      // at two shapes
#pragma unroll 1
      for (int kk = K - 1; kk >= 0; --kk) {
        const long ik = rw * K + kk;
        const float al = s_a[base + kk], T = p.trans[ik];
        const float wk = al * T;
        float gw = g_dep * s_z[base + kk] + g_bk;
        if (mp.g_weights) gw = gw + mp.g_weights[ik];
        float cg[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gw = __builtin_fmaf(g_rgb[c], s_c[base + kk][c], gw), cg[c] = g_rgb[c] * wk;
        s_go[base + kk][0] = mc_suffix_step(mp, ik, gw, al, T, P) * s_t[base + kk];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float cv = s_c[base + kk][c];
          s_go[base + kk][1 + c] = cg[c] * (cv * (1.0f - cv));   // sigmoid'
        }
      }
    }
    __syncthreads();
    // ---- the MLP backward of this lane's sample
    float go[kMcOut] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ln.live) {
      go[0] = s_go[tid][0];
      if (!(o[0] > 0.0f) || (p.empty_empty && invalid)) go[0] = 0.0f;   // relu'(o0), and the empty_empty select
      go[1] = s_go[tid][1], go[2] = s_go[tid][2], go[3] = s_go[tid][3];
    }
    float u0[HD];
    mc_mlp_bwd<C, HD, NB, kMcOut>(w, act, go, ln.live, want_w, mc_rays_here(mp, ray0) * K, s_A, s_B, t_out, t_w1, t_w0, u0);
    if (ln.live) {
      mc_store_row<HD>(mp.u0_ws + i * HD, u0);
      mp.gs_ws[i] = fmaxf(fmaxf(fabsf(go[0]), fabsf(go[1])), fmaxf(fabsf(go[2]), fabsf(go[3])));
    }
  }
  if (want_w) {
    t_out.flush(mp.d_mlp, ml.w_out(), ml.w_out() + kMcOut * HD);
    if constexpr (NB > 0) {
      t_w1.flush(mp.d_mlp, ml.blk_w1(0), ml.blk_b1(0));
      t_w0.flush(mp.d_mlp, ml.blk_w0(0), ml.blk_b0(0));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the kernels' parameters of this head's field: no colour taps, no render views
static FwdParams mc_field_params(const BtsFieldCfg* cfg, const BtsFieldTensors* t) {
  FwdParams p = make_params(cfg, t);
  p.imgs = p.K_r = p.w2c_r = nullptr, p.enc_view = -1;
  return p;
}

int mlp_color_render_fwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, hipStream_t s) {
  McParams mp;
  memset(&mp, 0, sizeof(mp));
  mp.f = mc_field_params(cfg, t);
  if (int rc = mc_render_params(mp, cfg, a, false, "bts_render_fwd_mlp_color")) return rc;
  return with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mc_render_kernel<S::C, S::HD, S::NB><<<(int)mp.n_groups, kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_fwd_mlp_color");
  });
}

int mlp_color_field_query_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int P, int only_density, float* rgb,
                               float* invalid, float* sigma, hipStream_t s) {
  FwdParams p = mc_field_params(cfg, t);
  p.xyz = xyz, p.Bp = P, p.K = 1, p.only_density = only_density;
  p.rgb = rgb, p.invalid = invalid, p.q_sigma = sigma;
  const long pts = (long)cfg->n * P;
  const long blocks = (pts + kMcThreads - 1) / kMcThreads;
  if (blocks > 0x7FFFFFFFL) {
    set_error("%s: too many points in one call (%ld)", "bts_field_query_mlp_color", pts);
    return BTS_E_UNSUPPORTED;
  }
  return with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mc_query_kernel<S::C, S::HD, S::NB><<<(int)blocks, kMcThreads, 0, s>>>(p);
    return mc_status("bts_field_query_mlp_color");
  });
}

// The backward's workspace, the row layout of bts_render_bwd's general path: u0 (B, K, HD) | g_s (B, K) | (16-byte boundary) pass C's
// slot copies.  workspace = null: only `bytes` means something.
struct McWs {
  float *u0, *gs, *flush;
  size_t bytes;
};
static McWs mc_ws_layout(void* workspace, const BtsFieldCfg* cfg, const BtsRenderArgs* a) {
  const size_t samples = (size_t)cfg->n * (size_t)a->rays_per_sample * (size_t)a->K, hd = (size_t)cfg->d_hidden;
  const size_t gs_at = samples * hd * sizeof(float), flush_at = align16(samples * (hd + 1) * sizeof(float));
  const auto at = [&](size_t off) { return workspace ? reinterpret_cast<float*>(static_cast<char*>(workspace) + off) : nullptr; };
  return {at(0), at(gs_at), at(flush_at), flush_at + sizeof(float) * kFlushSlots * kFlushRows * hd};
}

size_t mlp_color_bwd_workspace_impl(const BtsFieldCfg* cfg, const BtsRenderArgs* a) { return mc_ws_layout(nullptr, cfg, a).bytes; }

int mlp_color_render_bwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g, void* workspace,
                              hipStream_t s) {
  McParams mp;
  memset(&mp, 0, sizeof(mp));
  mp.f = mc_field_params(cfg, t);
  if (int rc = mc_render_params(mp, cfg, a, true, "bts_render_bwd_mlp_color")) return rc;
  if (!g->d_proj_nhwc && !g->d_empty_proj && !g->d_mlp_params) return BTS_OK;
  const McWs ws = mc_ws_layout(workspace, cfg, a);
  mp.g_rgb = g->g_rgb, mp.g_depth = g->g_depth, mp.g_weights = g->g_weights, mp.g_alphas = g->g_alphas;
  mp.u0_ws = ws.u0, mp.gs_ws = ws.gs, mp.d_mlp = g->d_mlp_params;
  // How many work-groups reside per CU is set by pass A's LDS and registers: one at d_hidden 64 (143 KB of LDS), one wave per SIMD at
  // (32, 32, 1)
  const int grid = render_grid(mp.f);
  int rc = with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mc_rows_kernel<S::C, S::HD, S::NB><<<mc_rows_grid(mp, grid), kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_bwd_mlp_color");
  });
  if (rc) return rc;
  return mc_launch_passes_bc(mc_pass_params(mp.f, cfg, g, g->d_proj_nhwc, g->d_proj_tiles, ws.gs, ws.flush), ws.u0, cfg, grid, s);
}

}  // namespace bts
