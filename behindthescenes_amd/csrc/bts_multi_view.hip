// Merged encoder views (BTSNet.encode(..., combine_ids=...) or several ids_encoder: the reference trainer's `frame_sample_mode: waymo-N`,
// models_bts.py:93-136, 190-210, 237-258): a point is projected into V encoder views, every encoder GROUP contributes the entry
// [bilinear F_v | empty_feature, PE_v] of its first member whose frustum flag is clear (else of its first member), the MLP reads the mean
// of the entries -- a one-member group counted twice (BtsMultiViewField.enc_mult) -- and the colours are sampled from the render groups'
// picked views.  lin_in is linear, so  lin_in(mean) = sum_g c_g (G_v[taps] | empty_proj) + W_pe . (sum_g c_g PE_v) + b  with v = the
// group's pick, c_g = multiplicity / T and G_v the projected map of view v (the projected-feature shortcut).
//
// Kernels, lane = SAMPLE (or point), fp32 throughout.  The MLP and its backward, a sample's alpha, the sums along a ray, the kernels'
// parameters and passes B and C's launches are bts_mc_field.h's, shared with bts_mlp_color.hip; this file holds the merged views' own: the
// picks (mv_field), the render groups' colours (mv_color), the per-view rows (mv_scale_kernel) and the workspace.
//   mv_render_kernel   one work-group = R = 256 / K whole rays: projection into the views, the picks, lin_in, blocks, lin_out, softplus,
//                      the render groups' colour taps; one lane per ray composites front to back from LDS.
//   mv_query_kernel    one lane = one query point (bts_field_query_multi_view).
//   mv_rows_kernel     pass A of the backward: the compositing gradient per ray, g_s = dL/d(lin_out's output) per sample, the MLP backward in
//                      registers; per sample u0 = dL/d(lin_in output) in G's storage order, |g_s| and per view c_v (0: not picked).
//   mv_scale_kernel    view v's rows c_v u0 and its liveness slot (0 exactly where c_v = 0 or the sample is dead).
// Passes B (scatter_kernel<HD, true>) and C (dwpe_rows_kernel) of bts_bwd_rows.hip then run unchanged once per view, with that view's
// camera, map and rows: both are linear in the rows and sum_v c_v = 1, so db_in, dW_pe, dG_v and d_empty_proj come out right.
#include "bts_mc_field.h"

namespace bts {

constexpr int kMvMax = BTS_MV_MAX_VIEWS;        // encoder views, encoder groups, render groups: at most this many each
constexpr int kMvColStride = 3 * kMvMax + 1;    // a sample's colours in LDS (odd: the lanes' rows spread over the banks)

struct MvTables {
  const float* proj[kMvMax];      // per encoder view: G_v (n, H >> fs, W >> fs, HD)
  const float* K_enc[kMvMax];     //                   (n, 3, 3)
  const float* w2c_enc[kMvMax];   //                   (n, 4, 4)
  int V, n_enc, n_ren, pad_;
  int enc_start[kMvMax + 1], enc_member[kMvMax];   // members of encoder group g: enc_member[enc_start[g] .. enc_start[g + 1])
  float enc_coef[kMvMax];                          // multiplicity / T
  int ren_start[kMvMax + 1], ren_member[kMvMax];   // render groups over the cfg's nv render views
};

// f = view 0's field: sizes, switches, MLP, empty feature, the render views' frames and cameras (proj, K_enc, w2c_enc: `t`); g_rgb is
// (B, nv' * 3), gs_ws = |dL/d(lin_out's output)|.  One flat kernel argument: the tables are read through kernarg_view
struct MvParams : McParams {
  MvTables t;
  float* cw_ws;            // backward: (V, B, K) c_v per sample
};
typedef const MvParams __attribute__((address_space(4)))* MvArgs;   // the tables are read from the kernarg segment: wave-uniform s_loads

// the first member of a group whose frustum flag is clear, else its first member (torch.min's tie rule on the CPU: torch_modes._merge_groups)
#define MV_TAKES(first, cur, cand) ((first) || ((cur).invalid && !(cand).invalid))

// Everything between a world point and the pre-softplus density.  cw != null: c_v of this sample is written to cw[v * cw_stride] for the
// picked views (the caller zeroed every view's slot).
template <int C, int HD, int NB>
__device__ __forceinline__ void mv_field(MvArgs q, const FwdParams& p, int sample, float px, float py, float pz, const float* empty_proj,
                                         McAct<C, HD, NB>& a, float& o0, bool& inv_f, float* cw, long cw_stride) {
  const cfp w = as_const(p.mlp);
  const long plane = (long)(p.H >> p.fs) * (p.W >> p.fs);
  float enc_in[kPeDim];
#pragma unroll
  for (int k = 0; k < kPeDim; ++k) enc_in[k] = 0.0f;
#pragma unroll
  for (int j = 0; j < HD; ++j) a.h0[j] = 0.0f;
  inv_f = false;
  const int n_enc = q->t.n_enc;
#pragma unroll 1
  for (int g = 0; g < n_enc; ++g) {
    const int m0 = q->t.enc_start[g], m1 = q->t.enc_start[g + 1];
    Proj ch = {};
    const float* Gc = nullptr;
    int cv = 0;
#pragma unroll 1
    for (int m = m0; m < m1; ++m) {
      const int v = q->t.enc_member[m];
      const Cam cam = load_cam_v(q->t.w2c_enc[v] + sample * 16, q->t.K_enc[v] + sample * 9);
      const Proj pr = p.code_mode == 1 ? project<true>(cam, px, py, pz) : project<false>(cam, px, py, pz);
      if (MV_TAKES(m == m0, ch, pr)) ch = pr, Gc = q->t.proj[v], cv = v;
    }
    const float c = q->t.enc_coef[g];
    inv_f = inv_f | ch.invalid;                       // invalid_features = any of the entries' flags (models_bts.py:210)
    if (cw) cw[cv * cw_stride] = c;
    float v3[3], e[kPeDim];
    v3[0] = ch.x, v3[1] = ch.y;
    v3[2] = depth_code(ch, p.code_mode == 1, p.inv_z != 0, p.inv_dmax, p.inv_range, p.d_min, p.range);
    mc_encode(e, v3, p.freq_factor);
#pragma unroll
    for (int k = 0; k < kPeDim; ++k) enc_in[k] = __builtin_fmaf(c, e[k], enc_in[k]);
    if (p.learn_empty && ch.invalid) {
#pragma unroll
      for (int j = 0; j < HD; ++j) a.h0[j] = __builtin_fmaf(c, empty_proj[j], a.h0[j]);
    } else {
      const Taps tp = make_taps(ch.x, ch.y, p.H, p.W, p.fs);
      mc_bilinear<HD, false>(a.h0, Gc + (long)sample * plane * HD, tp, c);
    }
  }
  float o[1];
  mc_mlp<C, HD, NB, 1>(w, enc_in, a, o);
  o0 = o[0];
}

// render group g's colour and frustum flag (models_bts.py:237-258: the same pick, over the render views)
__device__ __forceinline__ void mv_color(MvArgs q, const FwdParams& p, int g, int sample, float px, float py, float pz, float (&col)[3], bool& inv) {
  const int m0 = q->t.ren_start[g], m1 = q->t.ren_start[g + 1];
  Proj ch = {};
  const float4* img = nullptr;
#pragma unroll 1
  for (int m = m0; m < m1; ++m) {
    const long sv = (long)sample * p.nv + q->t.ren_member[m];
    const Cam cam = load_cam_v(p.w2c_r + sv * 16, p.K_r + sv * 9);
    const Proj pr = project<false>(cam, px, py, pz);
    if (MV_TAKES(m == m0, ch, pr)) ch = pr, img = reinterpret_cast<const float4*>(p.imgs) + sv * p.H * p.W;
  }
  inv = ch.invalid;
  const Taps tc = make_taps(ch.x, ch.y, p.H, p.W);
  const float4 a = img[tc.o00], b = img[tc.o01], cc = img[tc.o10], d = img[tc.o11];
  col[0] = ((a.x * tc.w00 + b.x * tc.w01) + cc.x * tc.w10) + d.x * tc.w11;
  col[1] = ((a.y * tc.w00 + b.y * tc.w01) + cc.y * tc.w10) + d.y * tc.w11;
  col[2] = ((a.z * tc.w00 + b.z * tc.w01) + cc.z * tc.w10) + d.z * tc.w11;
}

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mv_render_kernel(const MvParams mp) {
  const FwdParams& p = mp.f;
  const MvArgs q = kernarg_view<MvParams>();
  __shared__ float s_empty[HD];
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_w[kMcThreads], s_T[kMcThreads], s_ws[kMcThreads];
  __shared__ float s_c[kMcThreads * kMvColStride];
  mc_stage_empty<C, HD>(s_empty, p);
  const int K = p.K, nvp = mp.t.n_ren, nv3 = 3 * nvp;
  const long ray0 = (long)blockIdx.x * mp.R;
  const int tid = threadIdx.x;
  const McLane ln = mc_lane(mp, ray0, s_z, [&](long ray, int k) { return mc_depth(p, ray, k); });
  const long i = ln.ray * K + ln.k;
  __syncthreads();
  float o0 = 0.0f;
  if (ln.live) {
    const int sample = (int)(ln.ray / p.Bp);
    const float* rr = p.rays + ln.ray * 8;
    const float z = ln.z;
    const float px = rr[0] + z * rr[3], py = rr[1] + z * rr[4], pz = rr[2] + z * rr[5];
    McAct<C, HD, NB> act;
    bool inv_f;
    mv_field<C, HD, NB>(q, p, sample, px, py, pz, s_empty, act, o0, inv_f, nullptr, 0);
    // softplus: models_bts.py:313; the empty_empty select on the merged flag
    s_a[tid] = mc_alpha(p, s_z, ln.k, i, z, softplus(o0), p.empty_empty && inv_f).alpha;
#pragma unroll 1
    for (int g = 0; g < nvp; ++g) {
      float col[3];
      bool inv_c;
      mv_color(q, p, g, sample, px, py, pz, col, inv_c);
#pragma unroll
      for (int c = 0; c < 3; ++c) s_c[tid * kMvColStride + 3 * g + c] = col[c];
      if (p.invalid) p.invalid[i * nvp + g] = (inv_c | inv_f) ? 1.0f : 0.0f;   // models_bts.py:333
      if (p.rgb_samps) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.rgb_samps[(i * nvp + g) * 3 + c] = col[c];
      }
    }
  }
  __syncthreads();
  // one lane per ray: the transmittance product, the weights, depth and the weight sum
  if (mc_ray_lane(mp, ray0)) {
    const int base = tid * K;
    const McRaySums sums = mc_scan(s_a, s_z, s_T, base, K, [&](int kk, float wk) { s_w[base + kk] = wk; });
    s_ws[tid] = sums.wsum;
    p.depth[ray0 + tid] = sums.depth;
  }
  __syncthreads();
  // one lane per (ray, view, channel): rgb = sum_k w_k c_k
  const int rays_here = mc_rays_here(mp, ray0);
  for (int idx = tid; idx < rays_here * nv3; idx += kMcThreads) {
    const int r = idx / nv3, j = idx - r * nv3;
    const int base = r * K;
    float acc = 0.0f;
    for (int kk = 0; kk < K; ++kk) acc = acc + s_w[base + kk] * s_c[(base + kk) * kMvColStride + j];
    p.rgb[(ray0 + r) * nv3 + j] = p.white_bkgd ? acc + (1.0f - s_ws[r]) : acc;
  }
  if (ln.live) {
    if (p.weights) p.weights[i] = s_w[tid];
    if (p.alphas) p.alphas[i] = s_a[tid];
    if (p.trans) p.trans[i] = s_T[tid];
    if (p.sigma_raw) p.sigma_raw[i] = o0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// field query
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mv_query_kernel(const MvParams mp) {
  const FwdParams& p = mp.f;
  const MvArgs q = kernarg_view<MvParams>();
  __shared__ float s_empty[HD];
  mc_stage_empty<C, HD>(s_empty, p);
  __syncthreads();
  const long P = p.Bp;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)p.n * P) return;
  const int sample = (int)(idx / P);
  const float* x = p.xyz + idx * 3;
  const float px = x[0], py = x[1], pz = x[2];
  McAct<C, HD, NB> act;
  float o0;
  bool inv_f;
  mv_field<C, HD, NB>(q, p, sample, px, py, pz, s_empty, act, o0, inv_f, nullptr, 0);
  float sg = softplus(o0);
  if (p.empty_empty && inv_f) sg = 0.0f;
  p.q_sigma[idx] = sg;
  const int nvp = mp.t.n_ren;
#pragma unroll 1
  for (int g = 0; g < nvp; ++g) {
    float col[3];
    bool inv_c;
    mv_color(q, p, g, sample, px, py, pz, col, inv_c);
    if (p.invalid) p.invalid[idx * nvp + g] = (inv_c | inv_f) ? 1.0f : 0.0f;
    if (p.rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.rgb[(idx * nvp + g) * 3 + c] = col[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward, pass A
// ---------------------------------------------------------------------------------------------------------------
template <int C, int HD, int NB>
__global__ __launch_bounds__(kMcThreads) void mv_rows_kernel(const MvParams mp) {
  const FwdParams& p = mp.f;
  const MvArgs q = kernarg_view<MvParams>();
  constexpr int ASTR = HD + 1, BSTR = HD + 1;   // mc_mlp_bwd's rows
  __shared__ float s_empty[HD];
  __shared__ float s_z[kMcThreads], s_a[kMcThreads], s_t[kMcThreads], s_cd[kMcThreads], s_go[kMcThreads];
  __shared__ float s_A[kMcThreads * ASTR], s_B[kMcThreads * BSTR];
  mc_stage_empty<C, HD>(s_empty, p);
  const MlpLayout ml{C + kPeDim, HD, NB};
  const cfp w = as_const(p.mlp);
  const int K = p.K, nvp = mp.t.n_ren, nv3 = 3 * nvp, V = mp.t.V;
  const long samples = (long)p.n * p.Bp * K;
  const int tid = threadIdx.x;
  const bool want_w = mp.d_mlp != nullptr;
  McTile<1, HD> t_out;
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
    float dsig = 0.0f;   // d sigma / d o0
    if (ln.live) {
      const int sample = (int)(ln.ray / p.Bp);
      const float* rr = p.rays + ln.ray * 8;
      const float z = ln.z;
      const float px = rr[0] + z * rr[3], py = rr[1] + z * rr[4], pz = rr[2] + z * rr[5];
      for (int v = 0; v < V; ++v) mp.cw_ws[v * samples + i] = 0.0f;
      float o_now;
      bool inv_f;
      mv_field<C, HD, NB>(q, p, sample, px, py, pz, s_empty, act, o_now, inv_f, mp.cw_ws + i, samples);
      const float o0 = p.sigma_raw[i];   // the forward's (the same value: same routine)
      const bool empty = p.empty_empty && inv_f;
      dsig = empty ? 0.0f : sigmoidf(o0);
      const McAlpha al = mc_alpha(p, s_z, ln.k, i, z, softplus(o0), empty);
      s_a[tid] = al.alpha;
      s_t[tid] = mc_dalpha_dsigma(p, ln.k, al);
      // g_rgb . colours of this sample (the forward's colours when the caller kept them, else the taps again)
      float cd = 0.0f;
      if (mp.g_rgb) {
        const float* gr = mp.g_rgb + ln.ray * nv3;
        if (p.rgb_samps) {
          for (int j = 0; j < nv3; ++j) cd = __builtin_fmaf(gr[j], p.rgb_samps[i * nv3 + j], cd);
        } else {
#pragma unroll 1
          for (int g = 0; g < nvp; ++g) {
            float col[3];
            bool inv_c;
            mv_color(q, p, g, sample, px, py, pz, col, inv_c);
#pragma unroll
            for (int c = 0; c < 3; ++c) cd = __builtin_fmaf(gr[3 * g + c], col[c], cd);
          }
        }
      }
      s_cd[tid] = cd;
    }
    __syncthreads();
    // ---- one lane per ray: back to front
    if (mc_ray_lane(mp, ray0)) {
      const long rw = ray0 + tid;
      const int base = tid * K;
      float g_bk = 0.0f;
      if (mp.g_rgb && p.white_bkgd)                            // rgb += 1 - sum(weights): d/dw_k = -sum(g_rgb)
        for (int j = 0; j < nv3; ++j) g_bk -= mp.g_rgb[rw * nv3 + j];
      const float g_dep = mp.g_depth ? mp.g_depth[rw] : 0.0f;
      float P = 0.0f;
      for (int kk = K - 1; kk >= 0; --kk) {
        const long ik = rw * K + kk;
        float gw = g_dep * s_z[base + kk] + g_bk;
        if (mp.g_weights) gw = gw + mp.g_weights[ik];
        gw = gw + s_cd[base + kk];
        s_go[base + kk] = mc_suffix_step(mp, ik, gw, s_a[base + kk], p.trans[ik], P) * s_t[base + kk];
      }
    }
    __syncthreads();
    // ---- the MLP backward of this lane's sample
    float go[1] = {0.0f};
    if (ln.live) go[0] = s_go[tid] * dsig;   // softplus' = sigmoid, and the empty_empty select
    float u0[HD];
    mc_mlp_bwd<C, HD, NB, 1>(w, act, go, ln.live, want_w, mc_rays_here(mp, ray0) * K, s_A, s_B, t_out, t_w1, t_w0, u0);
    if (ln.live) {
      mc_store_row<HD>(mp.u0_ws + i * HD, u0);
      mp.gs_ws[i] = fabsf(go[0]);
    }
  }
  if (want_w) {
    t_out.flush(mp.d_mlp, ml.w_out(), ml.b_out());
    if constexpr (NB > 0) {
      t_w1.flush(mp.d_mlp, ml.blk_w1(0), ml.blk_b1(0));
      t_w0.flush(mp.d_mlp, ml.blk_w0(0), ml.blk_b0(0));
    }
  }
}

// rows_v = c_v u0 and view v's liveness slot: c_v where the sample is live (|g_s| != 0), else 0
__global__ __launch_bounds__(256) void mv_scale_kernel(const float* __restrict__ u0, const float* __restrict__ gs, const float* __restrict__ cw,
                                                      float* __restrict__ rows, float* __restrict__ gs_v, long samples, int hd4) {
  const long total = samples * hd4;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long i = e / hd4;
    const float c = cw[i];
    const float4 u = reinterpret_cast<const float4*>(u0)[e];
    reinterpret_cast<float4*>(rows)[e] = make_float4(c * u.x, c * u.y, c * u.z, c * u.w);
    if (e - i * hd4 == 0) gs_v[i] = gs[i] != 0.0f ? c : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the kernels' parameters of a CHECKED field (bts_api.hip: check_multi_view)
static MvParams mv_params(const BtsMultiViewField* mv) {
  MvParams mp;
  memset(&mp, 0, sizeof(mp));
  mp.f = make_params(&mv->cfg[0], &mv->view[0]);
  mp.f.enc_view = -1;
  MvTables& t = mp.t;
  t.V = mv->V, t.n_enc = mv->n_enc_groups, t.n_ren = mv->n_ren_groups;
  for (int v = 0; v < mv->V; ++v) t.proj[v] = mv->view[v].proj_nhwc, t.K_enc[v] = mv->view[v].K_enc, t.w2c_enc[v] = mv->view[v].w2c_enc;
  int T = 0;
  for (int g = 0; g < t.n_enc; ++g) T += mv->enc_mult[g];
  for (int g = 0; g <= t.n_enc; ++g) t.enc_start[g] = mv->enc_group_start[g];
  for (int g = 0; g <= t.n_ren; ++g) t.ren_start[g] = mv->ren_group_start[g];
  for (int g = 0; g < t.n_enc; ++g) t.enc_coef[g] = (float)mv->enc_mult[g] / (float)T;
  for (int m = 0; m < t.enc_start[t.n_enc]; ++m) t.enc_member[m] = mv->enc_member[m];
  for (int m = 0; m < t.ren_start[t.n_ren]; ++m) t.ren_member[m] = mv->ren_member[m];
  return mp;
}

int multi_view_render_fwd_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a, hipStream_t s) {
  const BtsFieldCfg* cfg = &mv->cfg[0];
  MvParams mp = mv_params(mv);
  if (int rc = mc_render_params(mp, cfg, a, false, "bts_render_fwd_multi_view")) return rc;
  return with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mv_render_kernel<S::C, S::HD, S::NB><<<(int)mp.n_groups, kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_fwd_multi_view");
  });
}

int multi_view_field_query_impl(const BtsMultiViewField* mv, const float* xyz, int P, float* rgb, float* invalid, float* sigma, hipStream_t s) {
  const BtsFieldCfg* cfg = &mv->cfg[0];
  MvParams mp = mv_params(mv);
  FwdParams& p = mp.f;
  p.xyz = xyz, p.Bp = P, p.K = 1;
  p.rgb = rgb, p.invalid = invalid, p.q_sigma = sigma;
  const long pts = (long)cfg->n * P;
  const long blocks = (pts + kMcThreads - 1) / kMcThreads;
  if (blocks > 0x7FFFFFFFL) {
    set_error("%s: too many points in one call (%ld)", "bts_field_query_multi_view", pts);
    return BTS_E_UNSUPPORTED;
  }
  return with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mv_query_kernel<S::C, S::HD, S::NB><<<(int)blocks, kMcThreads, 0, s>>>(mp);
    return mc_status("bts_field_query_multi_view");
  });
}

// u0 (B, K, HD) | one view's rows (B, K, HD) | |g_s| (B, K) | one view's liveness slots (B, K) | c_v (V, B, K) | pass C's slot copies
struct MvWs {
  float *u0, *rows, *gs, *gs_v, *cw, *flush;
};
static MvWs mv_ws_layout(Carver& w, const BtsMultiViewField* mv, const BtsRenderArgs* a) {
  const BtsFieldCfg* cfg = &mv->cfg[0];
  const size_t samples = (size_t)cfg->n * (size_t)a->rays_per_sample * (size_t)a->K;
  MvWs ws;
  ws.u0 = w.take<float>(samples * (size_t)cfg->d_hidden);
  ws.rows = w.take<float>(samples * (size_t)cfg->d_hidden);
  ws.gs = w.take<float>(samples);
  ws.gs_v = w.take<float>(samples);
  ws.cw = w.take<float>(samples * (size_t)mv->V);
  ws.flush = w.take<float>((size_t)kFlushSlots * kFlushRows * (size_t)cfg->d_hidden);
  return ws;
}

size_t multi_view_bwd_workspace_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a) {
  Carver w(nullptr);
  (void)mv_ws_layout(w, mv, a);
  return w.bytes();
}

int multi_view_render_bwd_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a, const BtsRenderGrads* g, float* const* d_proj_views,
                               unsigned char* const* d_proj_tiles_views, void* workspace, hipStream_t s) {
  const BtsFieldCfg* cfg = &mv->cfg[0];
  MvParams mp = mv_params(mv);
  if (int rc = mc_render_params(mp, cfg, a, true, "bts_render_bwd_multi_view")) return rc;
  bool want = g->d_mlp_params || g->d_empty_proj;
  for (int v = 0; v < mv->V; ++v) want = want || (d_proj_views && d_proj_views[v]);
  if (!want) return BTS_OK;
  Carver carve(workspace);
  const MvWs ws = mv_ws_layout(carve, mv, a);
  const long samples = (long)cfg->n * a->rays_per_sample * a->K;
  mp.g_rgb = g->g_rgb, mp.g_depth = g->g_depth, mp.g_weights = g->g_weights, mp.g_alphas = g->g_alphas;
  mp.u0_ws = ws.u0, mp.gs_ws = ws.gs, mp.cw_ws = ws.cw, mp.d_mlp = g->d_mlp_params;
  const int grid = render_grid(mp.f);
  int rc = with_shape(cfg->C, cfg->d_hidden, cfg->n_blocks, [&](auto sh) {
    using S = decltype(sh);
    mv_rows_kernel<S::C, S::HD, S::NB><<<mc_rows_grid(mp, grid), kMcThreads, 0, s>>>(mp);
    return mc_status("bts_render_bwd_multi_view");
  });
  const int hd4 = cfg->d_hidden / 4;
  const long scale_blocks = (samples * hd4 + 255) / 256;
  for (int v = 0; v < mv->V && rc == BTS_OK; ++v) {
    bool grouped = false;
    for (int m = 0; m < mv->enc_group_start[mv->n_enc_groups]; ++m) grouped = grouped || mv->enc_member[m] == v;
    if (!grouped) continue;   // c_v = 0 everywhere
    mv_scale_kernel<<<(int)(scale_blocks < 4096 ? scale_blocks : 4096), 256, 0, s>>>(ws.u0, ws.gs, ws.cw + (long)v * samples, ws.rows, ws.gs_v, samples, hd4);
    rc = mc_status("bts_render_bwd_multi_view");
    if (rc) break;
    BwdParams bp = mc_pass_params(mp.f, cfg, g, d_proj_views ? d_proj_views[v] : nullptr, d_proj_tiles_views ? d_proj_tiles_views[v] : nullptr,
                                  ws.gs_v, ws.flush);
    bp.f.proj = mv->view[v].proj_nhwc, bp.f.K_enc = mv->view[v].K_enc, bp.f.w2c_enc = mv->view[v].w2c_enc;
    rc = mc_launch_passes_bc(bp, ws.rows, cfg, grid, s);
  }
  return rc;
}

}  // namespace bts
