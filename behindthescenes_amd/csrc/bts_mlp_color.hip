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
#include "bts_mc_field.h"
#include "bts_host.h"

namespace bts {

constexpr int kMcOut = 4;         // lin_out rows: density + three colour channels

struct McParams {
  FwdParams f;
  int R;              // rays per work-group iteration (kMcThreads / K)
  long n_groups;      // ceil(n * Bp / R)
  // backward
  const float* g_rgb;      // (B, 3)
  const float* g_depth;    // (B)
  const float* g_weights;  // (B, K)
  const float* g_alphas;   // (B, K)
  float* u0_ws;            // (B, K, HD) storage order, or null
  float* gs_ws;            // (B, K)
  float* d_mlp;            // packed, four-output layout, or null
};

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
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_t[kMcThreads], s_c[kMcThreads][3], s_T[kMcThreads];
  mc_stage_empty<C, HD>(s_empty, p);
  const int K = p.K, R = mp.R;
  const long B = (long)p.n * p.Bp;
  const long ray0 = (long)blockIdx.x * R;
  const int tid = threadIdx.x;
  const int r_loc = tid / K, k = tid - r_loc * K;
  const long ray = ray0 + r_loc;
  const bool live = r_loc < R && ray < B;
  float z = 0.0f;
  if (live) {
    z = mc_depth(p, ray, k);
    s_z[tid] = z;
    if (p.z_out) p.z_out[ray * K + k] = z;
  }
  __syncthreads();
  float o[kMcOut] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool invalid = false;
  if (live) {
    const int sample = (int)(ray / p.Bp);
    const Cam enc = load_cam_v(p.w2c_enc + sample * 16, p.K_enc + sample * 9);
    const float* rr = p.rays + ray * 8;
    McAct<C, HD, NB> act;
    mc_field<C, HD, NB>(p, enc, sample, rr[0] + z * rr[3], rr[1] + z * rr[4], rr[2] + z * rr[5], s_empty, act, o, invalid);
    float sg = fmaxf(o[0], 0.0f);                              // models_bts.py:317
    if (p.empty_empty && invalid) sg = 0.0f;                   // models_bts.py:323-324
    if (p.sigma_noise) sg = sg + p.sigma_noise[ray * K + k];   // nerf.py:279-280
    const float delta = k < K - 1 ? s_z[tid + 1] - z : 1e10f;  // nerf.py:276-277
    const float t = transmittance(delta, sg);                  // exp(-|delta| relu(sigma)), nerf.py:283
    float alpha = 1.0f - t;
    if (p.hard_cap && k == K - 1) alpha = 1.0f;                // nerf.py:285-286
    s_a[tid] = alpha, s_t[tid] = t;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_c[tid][c] = mc_sigmoid(o[1 + c]);
  }
  __syncthreads();
  // one lane per ray: the transmittance product and the sums, front to back (nerf.py:288-304)
  if (tid < R && ray0 + tid < B) {
    const long rw = ray0 + tid;
    const int base = tid * K;
    float T = 1.0f, wsum = 0.0f, dep = 0.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
    for (int kk = 0; kk < K; ++kk) {
      const float al = s_a[base + kk];
      const float wk = al * T;
      s_T[base + kk] = T;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] + wk * s_c[base + kk][c];
      dep = dep + wk * s_z[base + kk];
      wsum = wsum + wk;
      T = T * ((1.0f - al) + 1e-10f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) p.rgb[rw * 3 + c] = p.white_bkgd ? rgb[c] + (1.0f - wsum) : rgb[c];
    p.depth[rw] = dep;
  }
  __syncthreads();
  if (live) {
    const long i = ray * K + k;
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
  constexpr int D_IN = C + kPeDim;
  constexpr int ASTR = HD + 1, BSTR = HD + 1;   // odd strides: a lane's row writes spread over the banks
  __shared__ float s_empty[HD];
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_t[kMcThreads], s_c[kMcThreads][3], s_go[kMcThreads][kMcOut];
  __shared__ float s_A[kMcThreads * ASTR], s_B[kMcThreads * BSTR];
  mc_stage_empty<C, HD>(s_empty, p);
  const MlpLayout ml{D_IN, HD, NB};
  const cfp w = as_const(p.mlp);
  const int K = p.K, R = mp.R;
  const long B = (long)p.n * p.Bp;
  const int tid = threadIdx.x;
  const int r_loc = tid / K, k = tid - r_loc * K;
  const bool want_w = mp.d_mlp != nullptr;
  McTile<kMcOut, HD> t_out;
  McTile<HD, HD> t_w1, t_w0;
  t_out.zero(), t_w1.zero(), t_w0.zero();
  for (long grp = blockIdx.x; grp < mp.n_groups; grp += gridDim.x) {
    const long ray0 = grp * R;
    const long ray = ray0 + r_loc;
    const bool live = r_loc < R && ray < B;
    __syncthreads();   // the previous iteration's LDS readers are done
    float z = 0.0f;
    if (live) {
      z = p.z_samp[ray * K + k];
      s_z[tid] = z;
    }
    __syncthreads();
    // ---- the sample's field, activations kept in registers
    McAct<C, HD, NB> act;
#pragma unroll
    for (int j = 0; j < HD; ++j) act.h0[j] = 0.0f, act.nn[NB > 0 ? j : 0] = 0.0f, act.h1[NB > 0 ? j : 0] = 0.0f;
    float o[kMcOut] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool invalid = false, sg_pos = false;
    if (live) {
      const int sample = (int)(ray / p.Bp);
      const Cam enc = load_cam_v(p.w2c_enc + sample * 16, p.K_enc + sample * 9);
      const float* rr = p.rays + ray * 8;
      mc_field<C, HD, NB>(p, enc, sample, rr[0] + z * rr[3], rr[1] + z * rr[4], rr[2] + z * rr[5], s_empty, act, o, invalid);
      const long i = ray * K + k;
      const float o0 = p.sigma_raw[i];   // the forward's (the same value: same routine)
      float sg = fmaxf(o0, 0.0f);
      if (p.empty_empty && invalid) sg = 0.0f;
      if (p.sigma_noise) sg = sg + p.sigma_noise[i];
      sg_pos = sg > 0.0f;
      const float delta = k < K - 1 ? s_z[tid + 1] - z : 1e10f;
      const float t = transmittance(delta, sg);
      float alpha = 1.0f - t;
      if (p.hard_cap && k == K - 1) alpha = 1.0f;
      s_a[tid] = alpha;
      s_t[tid] = (p.hard_cap && k == K - 1) || !sg_pos ? 0.0f : fabsf(delta) * t;   // d alpha / d sigma (relu'(0) = 0)
#pragma unroll
      for (int c = 0; c < 3; ++c) s_c[tid][c] = p.rgb_samps ? p.rgb_samps[i * 3 + c] : mc_sigmoid(o[1 + c]);
    }
    __syncthreads();
    // ---- one lane per ray: back to front.  P = sum_{j>k} g_w_j alpha_j prod_{k<i<j} (1 - alpha_i + 1e-10), so that dL/dalpha_k =
    // g_w_k T_k - T_k P + g_alpha_k without a division (the reference's cumprod gradient, nerf.py:288-289)
    if (tid < R && ray0 + tid < B) {
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
      for (int kk = K - 1; kk >= 0; --kk) {
        const long i = rw * K + kk;
        const float al = s_a[base + kk], T = p.trans[i];
        const float wk = al * T;
        float gw = g_dep * s_z[base + kk] + g_bk;
        if (mp.g_weights) gw = gw + mp.g_weights[i];
        float cg[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gw = __builtin_fmaf(g_rgb[c], s_c[base + kk][c], gw), cg[c] = g_rgb[c] * wk;
        float ga = gw * T - T * P;
        if (mp.g_alphas) ga = ga + mp.g_alphas[i];
        P = gw * al + ((1.0f - al) + 1e-10f) * P;
        s_go[base + kk][0] = ga * s_t[base + kk];
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
    if (live) {
      go[0] = s_go[tid][0];
      if (!(o[0] > 0.0f) || (p.empty_empty && invalid)) go[0] = 0.0f;   // relu'(o0), and the empty_empty select
      go[1] = s_go[tid][1], go[2] = s_go[tid][2], go[3] = s_go[tid][3];
    }
    float g1[HD];   // dL/d(last hidden layer)
#pragma unroll
    for (int j = 0; j < HD; ++j) {
      float a = 0.0f;
#pragma unroll
      for (int r = 0; r < kMcOut; ++r) a = __builtin_fmaf(w[ml.w_out() + r * HD + j], go[r], a);
      g1[j] = act.last(j) > 0.0f ? a : 0.0f;
    }
    if (want_w) {   // dW_out += g_o (x) relu(h_last), db_out += g_o
      if (live) {
#pragma unroll
        for (int r = 0; r < kMcOut; ++r) s_A[tid * ASTR + r] = go[r];
#pragma unroll
        for (int j = 0; j < HD; ++j) s_B[tid * BSTR + j] = fmaxf(act.last(j), 0.0f);
      }
      __syncthreads();
      t_out.add(s_A, ASTR, s_B, BSTR, (int)min((long)R, B - ray0) * K);
      __syncthreads();
    }
    float u0[HD];
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
        const int S = (int)min((long)R, B - ray0) * K;
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
    if (live && mp.u0_ws) {
      const long i = ray * K + k;
      float4* row = reinterpret_cast<float4*>(mp.u0_ws + i * HD);
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4)
        row[s4] = make_float4(u0[proj_hidden_of_storage(4 * s4)], u0[proj_hidden_of_storage(4 * s4 + 1)], u0[proj_hidden_of_storage(4 * s4 + 2)],
                              u0[proj_hidden_of_storage(4 * s4 + 3)]);
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
static int mc_status(const char* who) { return launch_check("%s: kernel launch failed (HIP error %ld)", who); }

int mlp_color_render_fwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, hipStream_t s) {
  McParams mp;
  memset(&mp, 0, sizeof(mp));
  mp.f = make_params(cfg, t);
  FwdParams& p = mp.f;
  p.imgs = p.K_r = p.w2c_r = nullptr, p.enc_view = -1;
  p.rays = a->rays, p.z_samp = a->z_samp;
  p.jitter = a->z_samp ? nullptr : a->jitter, p.z_out = a->z_samp ? nullptr : a->z_samp_out, p.lindisp = a->lindisp;
  p.Bp = a->rays_per_sample, p.K = a->K, p.hard_cap = a->hard_alpha_cap, p.white_bkgd = a->white_bkgd;
  p.rgb = a->rgb, p.depth = a->depth, p.weights = a->weights, p.alphas = a->alphas, p.invalid = a->invalid;
  p.rgb_samps = a->rgb_samps, p.sigma_raw = a->sigma_raw, p.trans = a->trans, p.sigma_noise = a->sigma_noise;
  mp.R = kMcThreads / p.K;
  mp.n_groups = ((long)cfg->n * p.Bp + mp.R - 1) / mp.R;
  if (mp.n_groups > 0x7FFFFFFFL) {
    set_error("%s: too many rays in one call (%ld)", "bts_render_fwd_mlp_color", (long)cfg->n * p.Bp);
    return BTS_E_UNSUPPORTED;
  }
  return with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mc_render_kernel<S::C, S::HD, S::NB><<<(int)mp.n_groups, kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_fwd_mlp_color");
  });
}

int mlp_color_field_query_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int P, int only_density, float* rgb,
                               float* invalid, float* sigma, hipStream_t s) {
  FwdParams p = make_params(cfg, t);
  p.imgs = p.K_r = p.w2c_r = nullptr, p.enc_view = -1;
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

static size_t mc_flush_bytes(const BtsFieldCfg* cfg) { return sizeof(float) * kFlushSlots * kFlushRows * (size_t)cfg->d_hidden; }

// the row layout of bts_render_bwd's general path: u0 (B, K, HD), g_s (B, K), pass C's slot copies
size_t mlp_color_bwd_workspace_impl(const BtsFieldCfg* cfg, const BtsRenderArgs* a) {
  const size_t samples = (size_t)cfg->n * (size_t)a->rays_per_sample * (size_t)a->K;
  return align16(samples * ((size_t)cfg->d_hidden + 1) * sizeof(float)) + mc_flush_bytes(cfg);
}

int mlp_color_render_bwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g, void* workspace,
                              hipStream_t s) {
  McParams mp;
  memset(&mp, 0, sizeof(mp));
  mp.f = make_params(cfg, t);
  FwdParams& p = mp.f;
  p.imgs = p.K_r = p.w2c_r = nullptr, p.enc_view = -1;
  p.rays = a->rays, p.z_samp = a->z_samp;
  p.Bp = a->rays_per_sample, p.K = a->K, p.hard_cap = a->hard_alpha_cap, p.white_bkgd = a->white_bkgd;
  p.sigma_raw = a->sigma_raw, p.trans = a->trans, p.sigma_noise = a->sigma_noise, p.rgb_samps = a->rgb_samps;
  p.tiles_per_sample = (a->rays_per_sample + 255) / 256;
  mp.R = kMcThreads / p.K;
  mp.n_groups = ((long)cfg->n * p.Bp + mp.R - 1) / mp.R;
  p.lpr = 64, p.groups = (long)cfg->n * p.Bp;
  if (p.groups > 0x7FF00000L) {
    set_error("%s: too many rays in one call (%ld)", "bts_render_bwd_mlp_color", p.groups);
    return BTS_E_UNSUPPORTED;
  }
  const size_t samples = (size_t)cfg->n * a->rays_per_sample * a->K;
  const bool want_b = g->d_proj_nhwc || g->d_empty_proj, want_c = g->d_mlp_params != nullptr;
  mp.g_rgb = g->g_rgb, mp.g_depth = g->g_depth, mp.g_weights = g->g_weights, mp.g_alphas = g->g_alphas;
  mp.u0_ws = (want_b || want_c) ? static_cast<float*>(workspace) : nullptr;
  mp.gs_ws = static_cast<float*>(workspace) + samples * (size_t)cfg->d_hidden;
  mp.d_mlp = g->d_mlp_params;
  if (!want_b && !want_c) return BTS_OK;
  // persistent grid of at most render_grid's size (the weight-gradient partials are flushed once per work-group).  How many reside per CU
  // is set by pass A's LDS and registers: one at d_hidden 64 (143 KB of LDS), one wave per SIMD at (32, 32, 1)
  const int grid = render_grid(p);
  int rc = with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    const long g_ = mp.n_groups < grid ? mp.n_groups : grid;
    mc_rows_kernel<S::C, S::HD, S::NB><<<(int)g_, kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_bwd_mlp_color");
  });
  if (rc) return rc;
  BwdParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.f = p;
  bp.g_rgb = g->g_rgb, bp.g_depth = g->g_depth;
  bp.d_proj = g->d_proj_nhwc, bp.d_mlp = g->d_mlp_params, bp.d_empty_proj = g->d_empty_proj;
  bp.gs_ws = mp.gs_ws;
  bp.flush_ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + align16(samples * ((size_t)cfg->d_hidden + 1) * sizeof(float)));
  bp.tiles = bp.d_proj ? g->d_proj_tiles : nullptr;
  bp.tiles_per_img = (int)map_tiles(cfg->H, cfg->W, cfg->feat_shift);
  bp.tile_tw = tile_cols(cfg->H >> cfg->feat_shift, cfg->W >> cfg->feat_shift, cfg->tile_blocks);
  if (want_c) rc = launch_dwpe_rows(bp.f, mp.u0_ws, bp.d_mlp, bp.flush_ws, cfg->C, cfg->d_hidden, cfg->n_blocks, cfg->n, grid, s, false);
  if (rc == BTS_OK && want_b) rc = launch_scatter_rows(bp, mp.u0_ws, cfg->d_hidden, cfg->n, s);
  return rc;
}

}  // namespace bts
