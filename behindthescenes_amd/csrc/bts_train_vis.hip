// bts_train_vis.hip -- the panels of the trainer's `visualize` (models/bts/trainer.py:430-506) for the first T <= 6 rendered frames of
// batch element 0: input, reconstruction, colour-mapped inverse depth per scale, the depth profile of three image rows, ray entropy,
// alpha sum, reconstruction error and the invalid share -- float32, channel-planar, exactly the tensors the reference hands to make_grid.
// include/bts_render.h lists the reference's quirks next to bts_train_vis.  Two launches on one stream, a kernel boundary is the only
// hand-over:
//   rays     a work-group takes kVisChunk pixels of ONE image row; a wave takes 64 / K' pixels at once, K' = the power of two at or
//            above K (K <= 64: segmented butterflies inside K' lanes; K > 64: one pixel, a lane holds up to four of its samples -- the
//            layout of bts_loss_reg.hip's reg_rays_kernel).  Per pixel S = sum_k (a_k + 1e-5), then p = (a + 1e-5) / S and sum p ln p;
//            the pixel's K * nv invalid values in the same sweep.  The pixel's sums wait in LDS until the chunk is done; the output
//            phase (thread = pixel) does the divisions behind them and writes whole rows: colour index, table look-up, three planes.
//            On the profile rows the work-group's maximum of the raw alphas (and "a NaN was seen") goes to a partial slot of its own.
//            The lane widths, the samples per lane and the view-count rung are template parameters (VALU-issue bound: see there)
//   panels   work-groups [0, pix_blocks): thread = pixel -- input, reconstruction, error and the S depths.  The others: one 64 x 64
//            tile (x, k) of a profile row.  Each folds ALL partials into the one maximum (a maximum does not depend on the order),
//            reads alphas contiguous in k, divides, keeps the value in a 64 x 65 LDS tile (65: neither side bank-conflicts on 64
//            banks) and writes contiguous in x, looking the table up on the way out.  (The tile holds the value, not its index: the
//            optional field output needs the value, and the index is two compares behind it.)
// No atomics of any kind: every sum is a butterfly or a fixed loop, the maximum is order-free; reruns are bit-identical.  alphas and
// invalid are const: the reference's in-place `alphas += 1e-5` on the caller's dict is NOT reproduced.  Plain fp32 with correctly
// rounded division (__fdiv_rn) and logf, no contraction: the fields are compared with torch's within rounding of the sums' order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bts_host.h"

namespace bts {

namespace {

constexpr int kVisThreads = 256;
constexpr int kVisWaves = kVisThreads / 64;
constexpr int kVisMaxPerLane = 4;       // K <= 256 samples over 64 lanes
constexpr int kVisChunk = 128;          // pixels of a row per work-group of the ray pass: one sweep of 4 waves at K = 2
constexpr int kVisTile = 64;            // the profile's transpose tile
constexpr int kVisMaxDim = 8192;        // h, w: the ray pass's grid has T * h rows

struct VisParams {
  const float* imgs[BTS_TRAIN_VIS_MAX_FRAMES];
  const float* rgb;
  const float* depth[BTS_MAX_SCALES];
  const float* alphas;
  const float* invalid;
  const double* lut;
  const float* z_near_far;      // (2) or NULL: z_near / z_far below
  float *input_im, *recon_im, *recon_depth, *depth_profile, *ray_entropy, *alpha_sum, *recon_mse, *invalids;
  float *f_depth, *f_profile, *f_entropy, *f_alpha_sum, *f_mse, *f_invalid;
  float* partials;              // (3 T, n_chunks, 2): maximum, NaN flag
  int T, h, w, K, nv, S, N;
  int seg_log2, n_chunks;       // a pixel's lanes = 1 << seg_log2; work-groups per row of the ray pass
  int rows[3];                  // h / 4, h / 2, 3 h / 4
  int pix_blocks, k_tiles, x_tiles;
  float z_near, z_far, log2K;
};

// matplotlib's Colormap.__call__ on a float32 array -- the twin of bts_frames.hip's cmap_index (restated: moved to a shared header it
// would have to leave every kernel of that file its instruction stream)
__device__ __forceinline__ int vis_cmap_index(float x, int N) {
  const float t = x * (float)N;
  if (t != t) return N + 2;
  if (t == (float)N) return N - 1;
  if (t < 0.0f) return N;
  if (t >= (float)N) return N + 1;
  return (int)t;
}

// the table row of x, each double rounded once to fp32, into the three planes of a channel-planar image (plane = pixels per channel)
__device__ __forceinline__ void vis_put(float* __restrict__ out, size_t plane, float x, int N, const double* __restrict__ lut) {
  const int k = vis_cmap_index(x, N);
  out[0] = (float)lut[3 * k], out[plane] = (float)lut[3 * k + 1], out[2 * plane] = (float)lut[3 * k + 2];
}

// torch's clamp(0, 1): a NaN stays a NaN
__device__ __forceinline__ float vis_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// sum over the 1 << kSegLog2 lanes of a pixel; every lane of the segment gets it (bts_loss_reg.hip's seg_sum with its width compiled in)
template <int kSegLog2>
__device__ __forceinline__ float vis_seg_sum(float v) {
#pragma unroll
  for (int off = (1 << kSegLog2) >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// kSegLog2: a pixel's lanes = 1 << kSegLog2; kPerLane: samples a lane holds (1: K <= 1 << kSegLog2; 4: K up to 256 on 64 lanes);
// kNvMax: the rung of with_nvmax at or above nv.  With run-time widths the pass was bound by VALU issue, not by HBM (README, "Training
// visualisation panels"): the widths are compiled in so that the butterflies unroll with their lane addresses hoisted, and everything
// a PIXEL needs once -- the four divisions behind the sums -- happens in the chunk's output phase, one lane per pixel, not in the sweep
template <int kSegLog2, int kPerLane, int kNvMax>
__global__ __launch_bounds__(kVisThreads) void train_vis_rays_kernel(const VisParams p) {
  __shared__ float s_val[2 + kNvMax][kVisChunk];     // per pixel: sum p ln p, S, and per view the sum of invalid over K
  __shared__ float s_hi[kVisWaves], s_bad[kVisWaves];
  constexpr int kSeg = 1 << kSegLog2, kPpw = 64 >> kSegLog2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sl = lane & (kSeg - 1);
  const int f = blockIdx.y / p.h, y = blockIdx.y - f * p.h;
  const int x0 = blockIdx.x * kVisChunk;
  const size_t row = ((size_t)f * p.h + y) * p.w;
  const int K = p.K, nv = p.nv;
  float hi = __int_as_float(0xFF800000), bad = 0.0f;
  for (int it = 0; it < kVisChunk / (kVisWaves * kPpw); ++it) {
    const int px = (it * kVisWaves + wave) * kPpw + (lane >> kSegLog2);
    const bool act = x0 + px < p.w;
    const size_t pix = row + (act ? x0 + px : 0);
    const float* __restrict__ al = p.alphas + pix * K;
    const float* __restrict__ iv = p.invalid + pix * K * nv;
    float a[kPerLane], m[kNvMax];
#pragma unroll
    for (int j = 0; j < kNvMax; ++j) m[j] = 0.0f;
    float S = 0.0f;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int k = sl + i * 64;
      a[i] = 0.0f;
      if (act && k < K) {
        const float v = al[k];
        hi = fmaxf(hi, v);                 // the profile's maximum: raw, unclamped, without the 1e-5
        if (v != v) bad = 1.0f;
        a[i] = v + 1e-5f;
        S += a[i];
#pragma unroll
        for (int j = 0; j < kNvMax; ++j)
          if (j < nv) m[j] += iv[k * nv + j];
      }
    }
    S = vis_seg_sum<kSegLog2>(S);
    float Ht = 0.0f;                       // sum p ln p, the logarithm natural
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int k = sl + i * 64;
      if (act && k < K) {
        const float d = __fdiv_rn(a[i], S);
        Ht += d * logf(d);
      }
    }
    Ht = vis_seg_sum<kSegLog2>(Ht);
#pragma unroll
    for (int j = 0; j < kNvMax; ++j)
      if (j < nv) m[j] = vis_seg_sum<kSegLog2>(m[j]);
    if (act && sl == 0) {
      s_val[0][px] = Ht, s_val[1][px] = S;
#pragma unroll
      for (int j = 0; j < kNvMax; ++j) s_val[2 + j][px] = m[j];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hi = fmaxf(hi, __shfl_xor(hi, o, 64)), bad = fmaxf(bad, __shfl_xor(bad, o, 64));
  if (lane == 0) s_hi[wave] = hi, s_bad[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kVisWaves; ++w) hi = fmaxf(hi, s_hi[w]), bad = fmaxf(bad, s_bad[w]);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (p.rows[j] == y) {
        float* o = p.partials + ((size_t)(f * 3 + j) * p.n_chunks + blockIdx.x) * 2;
        o[0] = hi, o[1] = bad;
      }
  }
  // the chunk's three rows of scalars leave as rows: thread = pixel, the two halves of the work-group share the three panels
  const int px = threadIdx.x & (kVisChunk - 1), x = x0 + px;
  if (x >= p.w) return;
  const size_t plane = (size_t)p.h * p.w, at = (size_t)y * p.w + x;
  for (int q = threadIdx.x / kVisChunk; q < 3; q += kVisThreads / kVisChunk) {
    float v;
    if (q == 0) {
      v = __fdiv_rn(-s_val[0][px], p.log2K);
    } else if (q == 1) {
      v = __fdiv_rn(s_val[1][px], (float)K);
    } else {                               // mean over K per view, then the mean of the views
      v = 0.0f;
#pragma unroll
      for (int j = 0; j < kNvMax; ++j)
        if (j < nv) v += __fdiv_rn(s_val[2 + j][px], (float)K);
      v = __fdiv_rn(v, (float)nv);
    }
    float* panel = q == 0 ? p.ray_entropy : (q == 1 ? p.alpha_sum : p.invalids);
    float* field = q == 0 ? p.f_entropy : (q == 1 ? p.f_alpha_sum : p.f_invalid);
    vis_put(panel + (size_t)f * 3 * plane + at, plane, v, p.N, p.lut);
    if (field) field[(size_t)f * plane + at] = v;
  }
}

__global__ __launch_bounds__(kVisThreads) void train_vis_panels_kernel(const VisParams p) {
  __shared__ float s_tile[kVisTile][kVisTile + 1];
  __shared__ float s_hi[kVisWaves], s_bad[kVisWaves];
  const size_t plane = (size_t)p.h * p.w;
  if ((int)blockIdx.x < p.pix_blocks) {
    const int per = p.pix_blocks / p.T, f = blockIdx.x / per;
    const size_t i = (size_t)(blockIdx.x - f * per) * kVisThreads + threadIdx.x;
    if (i >= plane) return;
    const float* __restrict__ im = p.imgs[f];
    const float* __restrict__ rg = p.rgb + ((size_t)f * plane + i) * p.nv * 3;
    float in[3], rc[3], e[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      in[c] = im[c * plane + i] * 0.5f + 0.5f;
      float s = 0.0f;
      for (int j = 0; j < p.nv; ++j) s += rg[j * 3 + c];
      rc[c] = __fdiv_rn(s, (float)p.nv);
      const float d = in[c] - rc[c];
      e[c] = __fdiv_rn(d * d, 2.0f);
      p.input_im[((size_t)f * 3 + c) * plane + i] = in[c];
      p.recon_im[((size_t)f * 3 + c) * plane + i] = rc[c];
    }
    const float mse = vis_clamp01(__fdiv_rn((e[0] + e[1]) + e[2], 3.0f));
    vis_put(p.recon_mse + (size_t)f * 3 * plane + i, plane, mse, p.N, p.lut);
    if (p.f_mse) p.f_mse[(size_t)f * plane + i] = mse;
    // ((1 / d - 1 / z_far) / (1 / z_near - 1 / z_far)).clamp(0, 1), every step fp32 as on the reference's float32 tensors
    const float z_near = p.z_near_far ? p.z_near_far[0] : p.z_near, z_far = p.z_near_far ? p.z_near_far[1] : p.z_far;
    const float inv_far = __fdiv_rn(1.0f, z_far), den = __fdiv_rn(1.0f, z_near) - inv_far;
    for (int s = 0; s < p.S; ++s) {
      const float t = vis_clamp01(__fdiv_rn(__fdiv_rn(1.0f, p.depth[s][(size_t)f * plane + i]) - inv_far, den));
      vis_put(p.recon_depth + ((size_t)s * p.T + f) * 3 * plane + i, plane, t, p.N, p.lut);
      if (p.f_depth) p.f_depth[((size_t)s * p.T + f) * plane + i] = t;
    }
    return;
  }
  int b = blockIdx.x - p.pix_blocks;
  const int xt = b % p.x_tiles;
  b /= p.x_tiles;
  const int kt = b % p.k_tiles, r = b / p.k_tiles;        // r = 3 frame + row, in [0, 3 T)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ONE maximum over all 3 T rows; a NaN anywhere makes it NaN (torch's max())
  float hi = __int_as_float(0xFF800000), bad = 0.0f;
  for (int i = threadIdx.x; i < 3 * p.T * p.n_chunks; i += kVisThreads) hi = fmaxf(hi, p.partials[2 * i]), bad = fmaxf(bad, p.partials[2 * i + 1]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hi = fmaxf(hi, __shfl_xor(hi, o, 64)), bad = fmaxf(bad, __shfl_xor(bad, o, 64));
  if (lane == 0) s_hi[wave] = hi, s_bad[wave] = bad;
  __syncthreads();
  hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])), bad = fmaxf(fmaxf(s_bad[0], s_bad[1]), fmaxf(s_bad[2], s_bad[3]));
  const float mx = bad != 0.0f ? __int_as_float(0x7FC00000) : hi;
  const int f = r / 3, y = p.rows[r - 3 * f];
  const float* __restrict__ src = p.alphas + ((size_t)f * p.h + y) * p.w * p.K;
  const int k_in = kt * kVisTile + lane, x_out = xt * kVisTile + lane;
  for (int xi = wave; xi < kVisTile; xi += kVisWaves) {       // reads contiguous in k
    const int x = xt * kVisTile + xi;
    if (x < p.w && k_in < p.K) {
      const float a = src[(size_t)x * p.K + k_in];
      s_tile[xi][lane] = __fdiv_rn(a < 0.0f ? 0.0f : a, mx);  // clamp_min(0) keeps a NaN; 0 / 0 = NaN, the bad colour
    }
  }
  __syncthreads();
  for (int ki = wave; ki < kVisTile; ki += kVisWaves) {       // writes contiguous in x
    const int k = kt * kVisTile + ki;
    if (k < p.K && x_out < p.w) {
      const float v = s_tile[lane][ki];
      const size_t kw = (size_t)p.K * p.w;
      vis_put(p.depth_profile + (size_t)r * 3 * kw + (size_t)k * p.w + x_out, kw, v, p.N, p.lut);
      if (p.f_profile) p.f_profile[(size_t)r * kw + (size_t)k * p.w + x_out] = v;
    }
  }
}

int vis_chunks(int w) { return (w + kVisChunk - 1) / kVisChunk; }

}  // namespace

bool train_vis_sizes_ok(int h, int w) { return h > 0 && w > 0 && h <= kVisMaxDim && w <= kVisMaxDim; }

static float* train_vis_layout(Carver& c, int T, int w) { return c.take<float>((size_t)3 * T * vis_chunks(w) * 2); }

size_t train_vis_bytes(int T, int w) {
  Carver count(nullptr);
  (void)train_vis_layout(count, T, w);
  return count.bytes();
}

int train_vis_launch(const BtsTrainVis* a, hipStream_t s) {
  VisParams p;
  for (int i = 0; i < BTS_TRAIN_VIS_MAX_FRAMES; ++i) p.imgs[i] = a->imgs[i < a->T ? i : 0];
  for (int i = 0; i < BTS_MAX_SCALES; ++i) p.depth[i] = a->depth[i < a->S ? i : 0];
  p.rgb = a->rgb, p.alphas = a->alphas, p.invalid = a->invalid, p.lut = a->lut, p.z_near_far = a->z_near_far;
  p.input_im = a->input_im, p.recon_im = a->recon_im, p.recon_depth = a->recon_depth, p.depth_profile = a->depth_profile;
  p.ray_entropy = a->ray_entropy, p.alpha_sum = a->alpha_sum, p.recon_mse = a->recon_mse, p.invalids = a->invalids;
  p.f_depth = a->f_depth, p.f_profile = a->f_profile, p.f_entropy = a->f_entropy, p.f_alpha_sum = a->f_alpha_sum, p.f_mse = a->f_mse;
  p.f_invalid = a->f_invalid;
  Carver carve(a->workspace);
  p.partials = train_vis_layout(carve, a->T, a->w);
  p.T = a->T, p.h = a->h, p.w = a->w, p.K = a->K, p.nv = a->nv, p.S = a->S, p.N = a->lut_N;
  p.seg_log2 = 1;
  while ((1 << p.seg_log2) < a->K && p.seg_log2 < 6) ++p.seg_log2;
  p.n_chunks = vis_chunks(a->w);
  p.rows[0] = a->h / 4, p.rows[1] = a->h / 2, p.rows[2] = 3 * a->h / 4;
  const long hw = (long)a->h * a->w;
  p.pix_blocks = a->T * (int)((hw + kVisThreads - 1) / kVisThreads);
  p.k_tiles = (a->K + kVisTile - 1) / kVisTile, p.x_tiles = (a->w + kVisTile - 1) / kVisTile;
  p.z_near = a->z_near, p.z_far = a->z_far, p.log2K = (float)std::log2((double)a->K);
  const dim3 grid(p.n_chunks, a->T * a->h);
  const int rc = with_nvmax(a->nv, [&](auto nvmax) {
    constexpr int NV = decltype(nvmax)::value;
    if (a->K > 64) train_vis_rays_kernel<6, kVisMaxPerLane, NV><<<grid, kVisThreads, 0, s>>>(p);
    else if (p.seg_log2 == 6) train_vis_rays_kernel<6, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    else if (p.seg_log2 == 5) train_vis_rays_kernel<5, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    else if (p.seg_log2 == 4) train_vis_rays_kernel<4, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    else if (p.seg_log2 == 3) train_vis_rays_kernel<3, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    else if (p.seg_log2 == 2) train_vis_rays_kernel<2, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    else train_vis_rays_kernel<1, 1, NV><<<grid, kVisThreads, 0, s>>>(p);
    return launch_code();
  });
  if (rc) return rc;
  train_vis_panels_kernel<<<p.pix_blocks + 3 * a->T * p.k_tiles * p.x_tiles, kVisThreads, 0, s>>>(p);
  return launch_code();
}

}  // namespace bts
