// Everything the lane = SAMPLE fp32 kernels of bts_mlp_color.hip and bts_multi_view.hip share; the two files keep only what is theirs
// (how a sample's feature, density and colour come about).
//   the field    the MLP behind lin_in's feature columns with its activations in registers (McAct, mc_mlp), its backward with the
//                per-work-group weight-gradient contraction (McTile, mc_mlp_bwd, mc_store_row), the projected empty feature, the encoding.
//                Weights are read through the constant address space (wave-uniform s_loads).  NOUT = lin_out's rows: 4 for MLP-predicted
//                colour (density + three channels), 1 for the density MLP.
//   compositing  a work-group iteration's sample set-up (mc_lane), one sample's alpha (mc_alpha, mc_dalpha_dsigma), the front-to-back scan of
//                a ray (mc_scan) and the step of the backward's back-to-front recurrence (mc_suffix_step).  Colour stays with each kernel.
//   host side    the kernels' parameters from a call's arguments (mc_render_params), pass A's grid (mc_rows_grid), passes B and C behind
//                it (mc_pass_params, mc_launch_passes_bc) and the launch status (mc_status).
#pragma once
#include "bts_bwd.h"
#include "bts_host.h"

namespace bts {

constexpr int kMcThreads = 256;   // samples of one work-group iteration (whole rays: K <= 256)

struct McParams {
  FwdParams f;
  int R;              // rays per work-group iteration (kMcThreads / K)
  long n_groups;      // ceil(n * Bp / R)
  // backward
  const float* g_rgb;      // (B, nv * 3)
  const float* g_depth;    // (B)
  const float* g_weights;  // (B, K)
  const float* g_alphas;   // (B, K)
  float* u0_ws;            // (B, K, HD) storage order
  float* gs_ws;            // (B, K) the liveness slot: 0 exactly where the sample contributes nothing
  float* d_mlp;            // packed, or null
};

// everything between a world point and the MLP outputs; h0 = lin_in's output, nn = fc_0's output, h1 = the last hidden layer (before
// lin_out's relu), in hidden order
template <int C, int HD, int NB>
struct McAct {
  float h0[HD];
  float nn[NB > 0 ? HD : 1];
  float h1[NB > 0 ? HD : 1];
  __device__ __forceinline__ float& last(int j) {
    if constexpr (NB > 0) return h1[j];
    else return h0[j];
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < HD; ++j) h0[j] = 0.0f, nn[NB > 0 ? j : 0] = 0.0f, h1[NB > 0 ? j : 0] = 0.0f;
  }
};

// a.h0 holds lin_in's feature part (bilinear G, or the projected empty feature); adds lin_in's encoding columns and bias, runs the blocks
// and lin_out's NOUT rows
template <int C, int HD, int NB, int NOUT>
__device__ __forceinline__ void mc_mlp(const cfp w, const float (&enc_in)[kPeDim], McAct<C, HD, NB>& a, float (&o)[NOUT]) {
  constexpr int D_IN = C + kPeDim;
  const MlpLayout ml{D_IN, HD, NB};
  // lin_in's encoding columns and bias (resnetfc.py:147)
#pragma unroll
  for (int j = 0; j < HD; ++j) {
    float acc = w[ml.b_in() + j];
#pragma unroll
    for (int k = 0; k < kPeDim; ++k) acc = __builtin_fmaf(w[ml.w_in() + j * D_IN + C + k], enc_in[k], acc);
    a.h0[j] = a.h0[j] + acc;
  }
  // ResnetBlockFC (resnetfc.py:53-62): h1 = h0 + fc_1(relu(fc_0(relu(h0))))
  if constexpr (NB > 0) {
    static_assert(NB == 1, "the envelope has at most one block");
#pragma unroll
    for (int j = 0; j < HD; ++j) {
      float acc = w[ml.blk_b0(0) + j];
#pragma unroll
      for (int i = 0; i < HD; ++i) acc = __builtin_fmaf(w[ml.blk_w0(0) + j * HD + i], fmaxf(a.h0[i], 0.0f), acc);
      a.nn[j] = acc;
    }
#pragma unroll
    for (int j = 0; j < HD; ++j) {
      float acc = w[ml.blk_b1(0) + j];
#pragma unroll
      for (int i = 0; i < HD; ++i) acc = __builtin_fmaf(w[ml.blk_w1(0) + j * HD + i], fmaxf(a.nn[i], 0.0f), acc);
      a.h1[j] = a.h0[j] + acc;
    }
  }
  // lin_out (resnetfc.py:183): w_out (NOUT, HD) row-major, b_out (NOUT)
#pragma unroll
  for (int r = 0; r < NOUT; ++r) {
    float acc = w[ml.w_out() + NOUT * HD + r];
#pragma unroll
    for (int j = 0; j < HD; ++j) acc = __builtin_fmaf(w[ml.w_out() + r * HD + j], fmaxf(a.last(j), 0.0f), acc);
    o[r] = acc;
  }
}

// positional encoding (code.py:30-42): [x, y, code, per octave sin(3), "cos"(3)]
__device__ __forceinline__ void mc_encode(float (&enc_in)[kPeDim], const float (&v3)[3], float freq_factor) {
  enc_in[0] = v3[0], enc_in[1] = v3[1], enc_in[2] = v3[2];
  float ff = freq_factor;
#pragma unroll
  for (int oct = 0; oct < kNumFreqs; ++oct) {
    float t[6];
    pe_octave(t, v3, ff);
#pragma unroll
    for (int i = 0; i < 6; ++i) enc_in[3 + 6 * oct + i] = t[i];
    ff = ff * 2.0f;
  }
}

// w_in[:, :C] . empty_feature (the projected empty feature, hidden order) into LDS
template <int C, int HD>
__device__ __forceinline__ void mc_stage_empty(float* empty_proj, const FwdParams& p) {
  const MlpLayout ml{C + kPeDim, HD, 0};
  for (int j = threadIdx.x; j < HD; j += blockDim.x) {
    float a = 0.0f;
    if (p.learn_empty && p.empty_feature)
      for (int c = 0; c < C; ++c) a = __builtin_fmaf(p.mlp[ml.w_in() + j * (C + kPeDim) + c], p.empty_feature[c], a);
    empty_proj[j] = a;
  }
}

// the sample depth of (ray, k): the caller's z_samp, or NeRFRenderer.sample_coarse from the jitter (nerf.py:103-123, as bts_sample_coarse)
__device__ __forceinline__ float mc_depth(const FwdParams& p, long ray, int k) {
  if (p.z_samp) return p.z_samp[ray * p.K + k];
  const float near = p.rays[ray * 8 + 6], far = p.rays[ray * 8 + 7];
  return coarse_depth(p.jitter[ray * p.K + k], coarse_base(p.K, k), 1.0f / (float)p.K, near, far, p.lindisp != 0);
}

// ---------------------------------------------------------------------------------------------------------------
// compositing: one lane per sample, one lane per ray for the sums along it
// ---------------------------------------------------------------------------------------------------------------
// This lane's sample of the work-group iteration that starts at ray0: sample k of ray `ray` (live: there is such a sample).  A live lane's
// depth = depth_of(ray, k) (the forward: mc_depth; the backward: the forward's z_samp) goes into s_z, and to z_out where the caller wants
// the depths back; the caller synchronises before s_z is read.
struct McLane {
  int k;
  long ray;
  bool live;
  float z;
};
template <class F>
__device__ __forceinline__ McLane mc_lane(const McParams& mp, long ray0, float* s_z, F&& depth_of) {
  const FwdParams& p = mp.f;
  const int tid = threadIdx.x, K = p.K;
  const int r_loc = tid / K;
  McLane l;
  l.k = tid - r_loc * K;
  l.ray = ray0 + r_loc;
  l.live = r_loc < mp.R && l.ray < (long)p.n * p.Bp;
  l.z = 0.0f;
  if (l.live) {
    l.z = depth_of(l.ray, l.k);
    s_z[tid] = l.z;
    if (p.z_out) p.z_out[l.ray * K + l.k] = l.z;
  }
  return l;
}
// the lane that sums along ray ray0 + threadIdx.x of the iteration
__device__ __forceinline__ bool mc_ray_lane(const McParams& mp, long ray0) {
  return (int)threadIdx.x < mp.R && ray0 + threadIdx.x < (long)mp.f.n * mp.f.Bp;
}
// the samples of the iteration (whole rays)
__device__ __forceinline__ int mc_rays_here(const McParams& mp, long ray0) { return (int)min((long)mp.R, (long)mp.f.n * mp.f.Bp - ray0); }

// One sample's alpha (nerf.py:276-286).  sg = the density after its activation, empty = the empty_empty select (models_bts.py:323-324);
// i = ray * K + k.  sigma = the density that entered the exponential.
struct McAlpha {
  float alpha, t, delta, sigma;
};
__device__ __forceinline__ McAlpha mc_alpha(const FwdParams& p, const float* s_z, int k, long i, float z, float sg, bool empty) {
  McAlpha a;
  if (empty) sg = 0.0f;
  if (p.sigma_noise) sg = sg + p.sigma_noise[i];                          // nerf.py:279-280
  a.sigma = sg;
  a.delta = k < p.K - 1 ? s_z[threadIdx.x + 1] - z : 1e10f;               // nerf.py:276-277
  a.t = transmittance(a.delta, sg);                                       // exp(-|delta| relu(sigma)), nerf.py:283
  a.alpha = 1.0f - a.t;
  if (p.hard_cap && k == p.K - 1) a.alpha = 1.0f;                         // nerf.py:285-286
  return a;
}
// d alpha / d sigma (relu'(0) = 0)
__device__ __forceinline__ float mc_dalpha_dsigma(const FwdParams& p, int k, const McAlpha& a) {
  return (p.hard_cap && k == p.K - 1) || !(a.sigma > 0.0f) ? 0.0f : fabsf(a.delta) * a.t;
}

// One ray's K samples front to back (nerf.py:288-304) from the alphas and depths in LDS at `base`: T_k into s_T, each(kk, w_k) with
// w_k = alpha_k T_k for whatever the kernel does with the weight (its colours), and the sums of w_k z_k and w_k.
struct McRaySums {
  float depth, wsum;
};
template <class F>
__device__ __forceinline__ McRaySums mc_scan(const float* s_a, const float* s_z, float* s_T, int base, int K, F&& each) {
  float T = 1.0f, wsum = 0.0f, dep = 0.0f;
  for (int kk = 0; kk < K; ++kk) {
    const float al = s_a[base + kk];
    const float wk = al * T;
    s_T[base + kk] = T;
    each(kk, wk);
    dep = dep + wk * s_z[base + kk];
    wsum = wsum + wk;
    T = T * ((1.0f - al) + 1e-10f);
  }
  return {dep, wsum};
}

// One step of the backward's walk back to front along a ray.  P = sum_{j>k} g_w_j alpha_j prod_{k<i<j} (1 - alpha_i + 1e-10), so that
// dL/dalpha_k = g_w_k T_k - T_k P + g_alpha_k without a division (the reference's cumprod gradient, nerf.py:288-289).  gw = dL/dw_k with the
// kernel's colour part in it, i = ray * K + k; returns dL/dalpha_k and moves P on to sample k - 1.
__device__ __forceinline__ float mc_suffix_step(const McParams& mp, long i, float gw, float al, float T, float& P) {
  float ga = gw * T - T * P;
  if (mp.g_alphas) ga = ga + mp.g_alphas[i];
  P = gw * al + ((1.0f - al) + 1e-10f) * P;
  return ga;
}

// per-work-group contraction of one outer-product sum over the iteration's samples: D[r][c] += sum_s A[s][r] B[s][c], c = COLS is the
// constant-1 column (the bias).  Lane t owns entries t, t + 256, ...: they stay in registers for the work-group's whole life.
template <int ROWS, int COLS>
struct McTile {
  static constexpr int N = ROWS * (COLS + 1);
  static constexpr int PER = (N + kMcThreads - 1) / kMcThreads;
  float acc[PER];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int q = 0; q < PER; ++q) acc[q] = 0.0f;
  }
  __device__ __forceinline__ void add(const float* A, int astr, const float* Bm, int bstr, int S) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * kMcThreads;
      if (e < N) {
        const int r = e / (COLS + 1), c = e - r * (COLS + 1);
        float a = acc[q];
        for (int s = 0; s < S; ++s) a = __builtin_fmaf(A[s * astr + r], c < COLS ? Bm[s * bstr + c] : 1.0f, a);
        acc[q] = a;
      }
    }
  }
  // weights at w_off ([ROWS][COLS] row-major), bias at b_off ([ROWS])
  __device__ __forceinline__ void flush(float* d_mlp, int w_off, int b_off) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * kMcThreads;
      if (e < N && acc[q] != 0.0f) {
        const int r = e / (COLS + 1), c = e - r * (COLS + 1);
        flush_add_f32(d_mlp + (c < COLS ? w_off + r * COLS + c : b_off + r), acc[q]);
      }
    }
  }
};

// The MLP backward of this lane's sample: go = dL/d(lin_out's outputs) -> u0 = dL/d(lin_in's output), hidden order.  want_w: lin_out's and
// the blocks' weight gradients are contracted over the iteration's S samples through s_A / s_B (kMcThreads rows of HD + 1 floats each) into
// the work-group's tiles.  Every lane of the work-group calls this (it synchronises).
template <int C, int HD, int NB, int NOUT>
__device__ __forceinline__ void mc_mlp_bwd(const cfp w, McAct<C, HD, NB>& act, const float (&go)[NOUT], bool live, bool want_w, int S, float* s_A,
                                           float* s_B, McTile<NOUT, HD>& t_out, McTile<HD, HD>& t_w1, McTile<HD, HD>& t_w0, float (&u0)[HD]) {
  constexpr int ASTR = HD + 1, BSTR = HD + 1;   // odd strides: a lane's row writes spread over the banks
  const MlpLayout ml{C + kPeDim, HD, NB};
  const int tid = threadIdx.x;
  float g1[HD];   // dL/d(last hidden layer)
#pragma unroll
  for (int j = 0; j < HD; ++j) {
    float a = 0.0f;
#pragma unroll
    for (int r = 0; r < NOUT; ++r) a = __builtin_fmaf(w[ml.w_out() + r * HD + j], go[r], a);
    g1[j] = act.last(j) > 0.0f ? a : 0.0f;
  }
  if (want_w) {   // dW_out += g_o (x) relu(h_last), db_out += g_o
    if (live) {
#pragma unroll
      for (int r = 0; r < NOUT; ++r) s_A[tid * ASTR + r] = go[r];
#pragma unroll
      for (int j = 0; j < HD; ++j) s_B[tid * BSTR + j] = fmaxf(act.last(j), 0.0f);
    }
    __syncthreads();
    t_out.add(s_A, ASTR, s_B, BSTR, S);
    __syncthreads();
  }
  if constexpr (NB > 0) {
    float gn[HD];   // dL/d(fc_0 output)
#pragma unroll
    for (int i = 0; i < HD; ++i) {
      float a = 0.0f;
#pragma unroll
      for (int j = 0; j < HD; ++j) a = __builtin_fmaf(w[ml.blk_w1(0) + j * HD + i], g1[j], a);
      gn[i] = act.nn[i] > 0.0f ? a : 0.0f;
    }
#pragma unroll
    for (int m = 0; m < HD; ++m) {
      float a = 0.0f;
#pragma unroll
      for (int i = 0; i < HD; ++i) a = __builtin_fmaf(w[ml.blk_w0(0) + i * HD + m], gn[i], a);
      u0[m] = g1[m] + (act.h0[m] > 0.0f ? a : 0.0f);   // the residual path + fc_0
    }
    if (want_w) {
      // dW1 += g_h1 (x) relu(nn), db1 += g_h1
      if (live) {
#pragma unroll
        for (int j = 0; j < HD; ++j) s_A[tid * ASTR + j] = g1[j], s_B[tid * BSTR + j] = fmaxf(act.nn[j], 0.0f);
      }
      __syncthreads();
      t_w1.add(s_A, ASTR, s_B, BSTR, S);
      __syncthreads();
      // dW0 += g_nn (x) relu(h0), db0 += g_nn
      if (live) {
#pragma unroll
        for (int j = 0; j < HD; ++j) s_A[tid * ASTR + j] = gn[j], s_B[tid * BSTR + j] = fmaxf(act.h0[j], 0.0f);
      }
      __syncthreads();
      t_w0.add(s_A, ASTR, s_B, BSTR, S);
    }
  } else {
#pragma unroll
    for (int j = 0; j < HD; ++j) u0[j] = g1[j];
  }
}

// u0 (hidden order) as one row of the backward's workspace: G's storage order
template <int HD>
__device__ __forceinline__ void mc_store_row(float* row_, const float (&u0)[HD]) {
  float4* row = reinterpret_cast<float4*>(row_);
#pragma unroll
  for (int s4 = 0; s4 < HD / 4; ++s4)
    row[s4] = make_float4(u0[proj_hidden_of_storage(4 * s4)], u0[proj_hidden_of_storage(4 * s4 + 1)], u0[proj_hidden_of_storage(4 * s4 + 2)],
                          u0[proj_hidden_of_storage(4 * s4 + 3)]);
}

// h0 (hidden order) += c * bilinear(G) at the taps; G = one image's projected map, channels in storage order (models_bts.py:173-182 after
// lin_in's feature columns; ATen's nw, ne, sw, se order)
template <int HD, bool FIRST>
__device__ __forceinline__ void mc_bilinear(float (&h0)[HD], const float* G_, const Taps& tp, float c) {
  const float4* G = reinterpret_cast<const float4*>(G_);
#pragma unroll
  for (int s4 = 0; s4 < HD / 4; ++s4) {
    const float4 t00 = G[(long)tp.o00 * (HD / 4) + s4], t01 = G[(long)tp.o01 * (HD / 4) + s4];
    const float4 t10 = G[(long)tp.o10 * (HD / 4) + s4], t11 = G[(long)tp.o11 * (HD / 4) + s4];
    const float g00[4] = {t00.x, t00.y, t00.z, t00.w}, g01[4] = {t01.x, t01.y, t01.z, t01.w};
    const float g10[4] = {t10.x, t10.y, t10.z, t10.w}, g11[4] = {t11.x, t11.y, t11.z, t11.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = g00[e] * tp.w00;
      v = v + g01[e] * tp.w01;
      v = v + g10[e] * tp.w10;
      v = v + g11[e] * tp.w11;
      if constexpr (FIRST) h0[proj_hidden_of_storage(4 * s4 + e)] = v;
      else h0[proj_hidden_of_storage(4 * s4 + e)] = __builtin_fmaf(c, v, h0[proj_hidden_of_storage(4 * s4 + e)]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
inline int mc_status(const char* who) { return launch_check("%s: kernel launch failed (HIP error %ld)", who); }

// The render kernels' parameters from a call's arguments, on top of the field's (mp.f = make_params(...)): forward (outputs, in-kernel
// sampling) or backward (the forward's saved state, what passes B and C read), R, n_groups and the limit on the rays of one call.
inline int mc_render_params(McParams& mp, const BtsFieldCfg* cfg, const BtsRenderArgs* a, bool bwd, const char* who) {
  FwdParams& p = mp.f;
  p.rays = a->rays, p.z_samp = a->z_samp;
  p.Bp = a->rays_per_sample, p.K = a->K, p.hard_cap = a->hard_alpha_cap, p.white_bkgd = a->white_bkgd;
  p.rgb_samps = a->rgb_samps, p.sigma_raw = a->sigma_raw, p.trans = a->trans, p.sigma_noise = a->sigma_noise;
  const long rays = (long)cfg->n * p.Bp;
  mp.R = kMcThreads / p.K;
  mp.n_groups = (rays + mp.R - 1) / mp.R;
  if (bwd) {
    p.tiles_per_sample = (a->rays_per_sample + 255) / 256;
    p.lpr = 64, p.groups = rays;
  } else {
    p.jitter = a->z_samp ? nullptr : a->jitter, p.z_out = a->z_samp ? nullptr : a->z_samp_out, p.lindisp = a->lindisp;
    p.rgb = a->rgb, p.depth = a->depth, p.weights = a->weights, p.alphas = a->alphas, p.invalid = a->invalid;
  }
  if (bwd ? rays > 0x7FF00000L : mp.n_groups > 0x7FFFFFFFL) {
    set_error("%s: too many rays in one call (%ld)", who, rays);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}

// pass A's grid: persistent, of at most render_grid's size (the weight-gradient partials are flushed once per work-group)
inline int mc_rows_grid(const McParams& mp, int grid) { return (int)(mp.n_groups < grid ? mp.n_groups : grid); }

// Passes B (dG += w_tap u0, d_empty_proj) and C (dW_pe, db_in) of bts_bwd_rows.hip on the rows and liveness slots pass A left: their
// parameters for the map d_proj of the field p (tiles: that map's dirty flags, or null), and the two launches.
inline BwdParams mc_pass_params(const FwdParams& p, const BtsFieldCfg* cfg, const BtsRenderGrads* g, float* d_proj, unsigned char* tiles, float* gs_ws,
                                float* flush_ws) {
  BwdParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.f = p;
  bp.g_rgb = g->g_rgb, bp.g_depth = g->g_depth;
  bp.d_proj = d_proj, bp.d_mlp = g->d_mlp_params, bp.d_empty_proj = g->d_empty_proj;
  bp.gs_ws = gs_ws, bp.flush_ws = flush_ws;
  bp.tiles = d_proj ? tiles : nullptr;
  bp.tiles_per_img = (int)map_tiles(cfg->H, cfg->W, cfg->feat_shift);
  bp.tile_tw = tile_cols(cfg->H >> cfg->feat_shift, cfg->W >> cfg->feat_shift, cfg->tile_blocks);
  return bp;
}
inline int mc_launch_passes_bc(const BwdParams& bp, const float* rows, const BtsFieldCfg* cfg, int grid, hipStream_t s) {
  int rc = BTS_OK;
  if (bp.d_mlp) rc = launch_dwpe_rows(bp.f, rows, bp.d_mlp, bp.flush_ws, cfg->C, cfg->d_hidden, cfg->n_blocks, cfg->n, grid, s, false);
  if (rc == BTS_OK && (bp.d_proj || bp.d_empty_proj)) rc = launch_scatter_rows(bp, rows, cfg->d_hidden, cfg->n, s);
  return rc;
}

}  // namespace bts
