// What the lane = SAMPLE fp32 kernels of bts_mlp_color.hip and bts_multi_view.hip share: the MLP behind lin_in's feature columns with its
// activations in registers (mc_mlp), its backward with the per-work-group weight-gradient contraction (McTile, mc_mlp_bwd), the projected
// empty feature and the sample depths.  Weights are read through the constant address space (wave-uniform s_loads).  NOUT = lin_out's rows:
// 4 for MLP-predicted colour (density + three channels), 1 for the density MLP.
#pragma once
#include "bts_bwd.h"

namespace bts {

constexpr int kMcThreads = 256;   // samples of one work-group iteration (whole rays: K <= 256)

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
// the work-group's tiles.  Every lane of the work-group calls this (it synchronises).  (mc_rows_kernel keeps these steps written out in its
// own body: as a call its instruction stream came out differently scheduled, and that kernel's stream is held to its previous revision's.)
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

}  // namespace bts
