// bts_loss_reg.hip -- the optional REGULARISERS of ReconstructionLoss (models/bts/model/loss.py:192-245, 261-281): alpha_reg (reduction
// ray | slice), surfaceness, ray entropy and the depth term that lambda_depth_reg and lambda_depth_smoothness both name, forward and
// gradient with respect to this scale's alphas (B, K) and depth (B).  include/bts_render.h lists the reference's quirks next to
// bts_loss_regularisers.  The invalid-ray rule is bts_loss_device.h's ray_invalid over this file's parameter struct.  Everything is
// memory-bound (alphas is read once, twice in slice mode with gradients); launches on one stream, a kernel boundary is the only
// hand-over between work-groups:
//   keep     thread = ray: the keep flag (policies other than none)
//   rays     a wave takes 64 / K' rays at once, K' = the power of two at or above K (K <= 64: segmented butterflies inside K' lanes;
//            K > 64: one ray, a lane holds up to four of its samples): per ray A = sum_{k < K-1} a_k, sum_k p_k, S = sum_k (a_k + 1e-5) and
//            H = -sum d ln d / log2 K -> a workspace row; unless the alpha gate waits for a row sum (slice) the gradient row in the same pass
//   pixels   thread = ray: the per-ray terms times keep, the slice rows' sums, terms and gates (the thread of a row's first pixel adds
//            the row in order), the depth differences -- a pixel owns the edges to its right and lower neighbour inside the patch -- and
//            g_depth, which gathers the left and upper ones; per work-group partials
//   final    one work-group: the partials in index order, in fp64, rounded once -> terms[5] and reg = sum_t c_t term_t
//   rays<grad> slice mode with gradients only: alphas once more, the row's gate from the workspace
// No float atomics: every sum is a butterfly, then a fixed-order sum of per-work-group partials; reruns are bit-identical.  Every
// element of g_alphas / g_depth is written exactly once.  Plain fp32 with expf / logf (no fast intrinsics).
#include <hip/hip_runtime.h>

#include <cmath>

#include "bts_host.h"
#include "bts_loss_device.h"

namespace bts {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPerLane = 4;        // K <= 256 samples over 64 lanes
constexpr int kPartials = 5;          // alpha, surfaceness, entropy, squared depth differences along y, along x

struct RegParams {
  const float* alphas;          // (B, Ka)
  const float* depth;           // (B) or NULL
  // the invalid-ray inputs of scale 0 (ray_invalid reads nv, K, policy and these)
  const float* weights;
  const float* invalid;
  const float* invalid_wsum;
  const float* invalid_any;
  const float* rgb_samps;
  float* terms;                 // (5)
  float* reg;                   // (1)
  float* g_alphas;              // (B, Ka) or NULL
  float* g_depth;               // (B) or NULL
  int nv, K, policy;            // K: the samples of `invalid` / `weights`
  int Ka, seg_log2;             // samples of `alphas`; a ray's lanes = 1 << seg_log2
  int ph, pw;
  int on_alpha, on_surf, on_ent, on_depth, slice;
  float c_alpha, c_surf, c_ent, c_depth;
  float cap, log2K;
  long B, n_rows, n_blocks;     // rays, patch rows, work-groups of the pixel pass
  float n_dy, n_dx;             // pairs along y and x inside the patches
  // workspace
  unsigned char* keep;          // (B): 0 = invalid ray
  float4* stats;                // (B): A, sum p, H, S
  unsigned char* row_gate;      // (n_rows): the slice rows' clamp gates
  float* blk;                   // (5, n_blocks)
  unsigned* blk_inv;            // (n_blocks)
};

__global__ __launch_bounds__(kThreads) void reg_keep_kernel(const RegParams p) {
  const long ray = blockIdx.x * (long)kThreads + threadIdx.x;
  if (ray >= p.B) return;
  p.keep[ray] = ray_invalid<false, true>(p, ray) ? 0 : 1;
}

// sum over the 1 << seg_log2 lanes of a ray; every lane of the segment gets it
__device__ __forceinline__ float seg_sum(float v, int seg_log2) {
  for (int off = (1 << seg_log2) >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// d p / d a of p = -log(exp(-|a|) + exp(-|1 - a|)), torch's: sign(0) = 0 for both absolute values
__device__ __forceinline__ float surf_grad(float a) {
  const float e1 = expf(-fabsf(a)), e2 = expf(-fabsf(1.0f - a));
  return (sign0(a) * e1 - sign0(1.0f - a) * e2) / (e1 + e2);
}

// kGrad = false: the per-ray sums -> stats, and the gradient row unless the slice gate is still unknown.  kGrad = true: the gradient
// row alone (slice mode), the same sums formed again from the same loads in the same order
template <bool kGrad>
__global__ __launch_bounds__(kThreads) void reg_rays_kernel(const RegParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = 1 << p.seg_log2, sl = lane & (seg - 1);
  const long ray = ((long)blockIdx.x * kWaves + wave) * (64 >> p.seg_log2) + (lane >> p.seg_log2);
  const bool act = ray < p.B;
  const int K = p.Ka;
  const float* row = p.alphas + (act ? ray : 0) * K;
  float a[kMaxPerLane];
  float A = 0.0f, P = 0.0f, S = 0.0f;
#pragma unroll
  for (int i = 0; i < kMaxPerLane; ++i) {
    const int k = sl + i * 64;
    a[i] = 0.0f;
    if (act && k < K) {
      a[i] = row[k];
      S += a[i] + 1e-5f;
      if (k < K - 1) A += a[i];
      if (p.on_surf) P += -logf(expf(-fabsf(a[i])) + expf(-fabsf(1.0f - a[i])));
    }
  }
  A = seg_sum(A, p.seg_log2), S = seg_sum(S, p.seg_log2);
  if (p.on_surf) P = seg_sum(P, p.seg_log2);
  float Ht = 0.0f;      // -sum d ln d, the logarithm natural
  if (p.on_ent) {
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i) {
      const int k = sl + i * 64;
      if (act && k < K) {
        const float d = (a[i] + 1e-5f) / S;
        Ht -= d * logf(d);
      }
    }
    Ht = seg_sum(Ht, p.seg_log2);
  }
  if (!kGrad && act && sl == 0) p.stats[ray] = make_float4(A, P, Ht / p.log2K, S);
  if (!p.g_alphas || (!kGrad && p.on_alpha && p.slice) || !act) return;
  const float keep = (p.policy == 0 || p.keep[ray]) ? 1.0f : 0.0f;
  const float nB = (float)p.B;
  float ga = 0.0f;
  if (p.on_alpha) {
    // torch's clamp_min passes the gradient at an exact tie
    const bool gate = p.slice ? p.row_gate[ray / p.pw] != 0 : (A * keep - p.cap * keep >= 0.0f);
    ga = gate ? p.c_alpha / nB * keep : 0.0f;
  }
  const float gs = p.c_surf / nB / (float)K * keep;
  const float ge = p.c_ent / nB * keep;
  float* g = p.g_alphas + ray * K;
#pragma unroll
  for (int i = 0; i < kMaxPerLane; ++i) {
    const int k = sl + i * 64;
    if (k < K) {
      float v = k < K - 1 ? ga : 0.0f;
      if (p.on_surf) v += gs * surf_grad(a[i]);
      if (p.on_ent) v += ge * (-(logf((a[i] + 1e-5f) / S) + Ht) / (S * p.log2K));
      g[k] = v;
    }
  }
}

// the work-group's sum: butterfly per wave, then the four waves in order; thread 0 uses it.  s_red: 4 words
__device__ __forceinline__ float group_sum(float v, float* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(kThreads) void reg_pixels_kernel(const RegParams p) {
  __shared__ float s_red[kWaves];
  const long ray = blockIdx.x * (long)kThreads + threadIdx.x;
  float v[kPartials] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float inv = 0.0f;
  if (ray < p.B) {
    const int pw = p.pw, ph = p.ph;
    const long row = ray / pw;
    const int x = (int)(ray - row * pw), y = (int)(row % ph);
    const float keep = (p.policy == 0 || p.keep[ray]) ? 1.0f : 0.0f;
    inv = 1.0f - keep;
    if (p.on_alpha || p.on_surf || p.on_ent) {
      const float4 st = p.stats[ray];
      if (p.on_alpha && !p.slice) v[0] = fmaxf(st.x * keep - p.cap * keep, 0.0f);
      if (p.on_surf) v[1] = st.y / (float)p.Ka * keep;
      if (p.on_ent) v[2] = st.z * keep;
    }
    if (p.on_alpha && p.slice && x == 0) {     // the row's first pixel adds the row, x ascending
      float sa = 0.0f, sc = 0.0f;
      for (int j = 0; j < pw; ++j) {
        const float kj = (p.policy == 0 || p.keep[ray + j]) ? 1.0f : 0.0f;
        sa += p.stats[ray + j].x * kj;
        sc += p.cap * kj;
      }
      const float t = sa - sc;
      v[0] = fmaxf(t, 0.0f) / (float)pw;
      p.row_gate[row] = t >= 0.0f ? 1 : 0;
    }
    if (p.on_depth) {
      const float d = p.depth[ray];
      const bool has_r = x + 1 < pw, has_b = y + 1 < ph;
      const float ex = has_r ? p.depth[ray + 1] - d : 0.0f, ey = has_b ? p.depth[ray + pw] - d : 0.0f;
      v[3] = ey * ey, v[4] = ex * ex;
      if (p.g_depth) {
        // this pixel's own edges and the edges its left / upper neighbour owns
        float gy = -ey, gx = -ex;
        if (y > 0) gy += d - p.depth[ray - pw];
        if (x > 0) gx += d - p.depth[ray - 1];
        p.g_depth[ray] = p.c_depth * (2.0f * gy / p.n_dy + 2.0f * gx / p.n_dx);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kPartials; ++t) {
    const float s = group_sum(v[t], s_red);
    if (threadIdx.x == 0) p.blk[t * p.n_blocks + blockIdx.x] = s;
  }
  const float si = group_sum(inv, s_red);      // at most 256: exact
  if (threadIdx.x == 0) p.blk_inv[blockIdx.x] = (unsigned)si;
}

// one work-group: thread t takes partials t, t + 256, ... in order, then the waves' butterflies, then the four waves in order; fp64
// throughout, every term rounded to fp32 once
__global__ __launch_bounds__(kThreads) void reg_final_kernel(const RegParams p) {
  __shared__ double s_d[kPartials + 1][kWaves];
  double acc[kPartials + 1];
#pragma unroll
  for (int t = 0; t <= kPartials; ++t) acc[t] = 0.0;
  for (long i = threadIdx.x; i < p.n_blocks; i += kThreads) {
#pragma unroll
    for (int t = 0; t < kPartials; ++t) acc[t] += (double)p.blk[t * p.n_blocks + i];
    acc[kPartials] += (double)p.blk_inv[i];
  }
#pragma unroll
  for (int t = 0; t <= kPartials; ++t) {
    for (int off = 32; off >= 1; off >>= 1) acc[t] += __shfl_xor(acc[t], off, 64);
    if ((threadIdx.x & 63) == 0) s_d[t][threadIdx.x >> 6] = acc[t];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[kPartials + 1];
#pragma unroll
    for (int t = 0; t <= kPartials; ++t) tot[t] = ((s_d[t][0] + s_d[t][1]) + s_d[t][2]) + s_d[t][3];
    const float t_alpha = p.on_alpha ? (float)(tot[0] / (double)(p.slice ? p.n_rows : p.B)) : 0.0f;
    const float t_surf = p.on_surf ? (float)(tot[1] / (double)p.B) : 0.0f;
    const float t_ent = p.on_ent ? (float)(tot[2] / (double)p.B) : 0.0f;
    const float t_depth = p.on_depth ? (float)(tot[3] / (double)p.n_dy) + (float)(tot[4] / (double)p.n_dx) : 0.0f;
    p.terms[0] = t_alpha, p.terms[1] = t_surf, p.terms[2] = t_ent, p.terms[3] = t_depth, p.terms[4] = (float)tot[kPartials];
    p.reg[0] = ((p.c_alpha * t_alpha + p.c_surf * t_surf) + p.c_ent * t_ent) + p.c_depth * t_depth;
  }
}

// THE layout of bts_loss_regularisers' workspace: keep flags, the per-ray sums, the slice rows' gates, five partials and the invalid
// rays per work-group of the pixel pass
inline void reg_layout(Carver& w, RegParams& p, size_t B, size_t n_rows) {
  const size_t n_blocks = (B + kThreads - 1) / kThreads;
  p.keep = w.take<unsigned char>(B);
  p.stats = w.take<float4>(B);
  p.row_gate = w.take<unsigned char>(n_rows);
  p.blk = w.take<float>(kPartials * n_blocks);
  p.blk_inv = w.take<unsigned>(n_blocks);
}

}  // namespace

size_t loss_reg_bytes(long B, int n_patches, int ph, int pw, int K) {
  if (B <= 0 || n_patches <= 0 || ph <= 0 || pw <= 0 || K <= 0 || (long)n_patches * ph * pw != B) return 0;
  Carver count(nullptr);
  RegParams p;
  reg_layout(count, p, (size_t)B, (size_t)n_patches * ph);
  return count.bytes();
}

int loss_reg_impl(const BtsLossRegArgs* a, void* workspace, hipStream_t s) {
  RegParams p;
  p.alphas = a->alphas, p.depth = a->depth, p.weights = a->weights, p.invalid = a->invalid, p.invalid_wsum = a->invalid_wsum;
  p.invalid_any = a->invalid_any, p.rgb_samps = a->rgb_samps;
  p.terms = a->terms, p.reg = a->reg, p.g_alphas = a->g_alphas, p.g_depth = a->g_depth;
  p.nv = a->nv, p.K = a->K_invalid, p.policy = a->invalid_policy, p.Ka = a->K, p.ph = a->patch_h, p.pw = a->patch_w;
  p.seg_log2 = 1;
  while ((1 << p.seg_log2) < p.Ka && p.seg_log2 < 6) ++p.seg_log2;
  p.on_alpha = a->coef_alpha_reg > 0.0f, p.on_surf = a->coef_surfaceness > 0.0f, p.on_ent = a->coef_entropy > 0.0f;
  p.on_depth = a->coef_depth > 0.0f, p.slice = a->alpha_reg_slice ? 1 : 0;
  p.c_alpha = p.on_alpha ? a->coef_alpha_reg : 0.0f, p.c_surf = p.on_surf ? a->coef_surfaceness : 0.0f;
  p.c_ent = p.on_ent ? a->coef_entropy : 0.0f, p.c_depth = p.on_depth ? a->coef_depth : 0.0f;
  p.cap = (float)((double)p.Ka * (double)a->alpha_reg_fraction);
  p.log2K = (float)log2((double)p.Ka);
  p.B = (long)a->B, p.n_rows = (long)a->n_patches * p.ph;
  p.n_blocks = (p.B + kThreads - 1) / kThreads;
  p.n_dy = (float)((long)a->n_patches * (p.ph - 1) * p.pw), p.n_dx = (float)((long)a->n_patches * p.ph * (p.pw - 1));
  Carver carve(workspace);
  reg_layout(carve, p, (size_t)p.B, (size_t)p.n_rows);
  const bool rays = p.on_alpha || p.on_surf || p.on_ent;
  if (!rays) p.g_alphas = nullptr;
  if (!p.on_depth) p.g_depth = nullptr;
  const unsigned grid_px = (unsigned)p.n_blocks;
  const long per_group = (long)kWaves * (64 >> p.seg_log2);
  const unsigned grid_rays = (unsigned)((p.B + per_group - 1) / per_group);
  if (p.policy) reg_keep_kernel<<<grid_px, kThreads, 0, s>>>(p);
  if (rays) reg_rays_kernel<false><<<grid_rays, kThreads, 0, s>>>(p);
  reg_pixels_kernel<<<grid_px, kThreads, 0, s>>>(p);
  reg_final_kernel<<<1, kThreads, 0, s>>>(p);
  if (p.g_alphas && p.on_alpha && p.slice) reg_rays_kernel<true><<<grid_rays, kThreads, 0, s>>>(p);
  return launch_check("%s: loss regulariser kernel launch failed (%ld)");
}

}  // namespace bts
