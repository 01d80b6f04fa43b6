// bts_loss_pixel_c.hip -- the l1 / l2 criteria of ReconstructionLoss (models/bts/model/loss.py:43-293) for a RUN-TIME channel count
// C (1 <= C <= 27): the colour targets of image_processor {type: patch} have 27 channels.  bts_loss_pixel.hip's rules, a kernel set of
// its own (those kernels keep their device code): thread = ray,
//   e[ray, ch] = min_v crit(rgb[ray, v, ch] - gt[ray, ch]) * keep,   rgb term = sum e / (B C),
// keep from bts_loss_device.h's ray_invalid under the policies none / strict / weight_guided (per-sample weights + invalid, or the
// renderer's per-ray reductions); the gradient follows torch's amin (tied views share it EQUALLY), sign(0) = 0 for l1, 2 d for l2, its
// normaliser scale_rgb / (B C) is known up front.  Two launches: the rays (per work-group the sum of e and the invalid rays), then one
// work-group that adds the partials in index order.  No atomics: a rerun is bit-identical.  Not here (bts_pixel_loss has them for three
// channels): median thresholding, weight_guided_diverse, the automasking bound, edge-aware smoothness.
#include <hip/hip_runtime.h>

#include "bts_host.h"
#include "bts_loss_device.h"

namespace bts {

namespace {

constexpr int kThreads = 256;

struct PixelCParams {
  const float *rgb, *rgb_gt;                               // (B, nv, C), (B, C)
  const float *weights, *invalid, *invalid_wsum, *invalid_any;
  float *out, *g_rgb, *g_depth;                            // (4); (B, nv, C) or null; (B) or null: zeros (no term reads the depth)
  int nv, K, policy, crit, C;
  float s_rgb;
  long B, n_blocks;
  float* blk_sum;                                          // (n_blocks)
  unsigned* blk_inv;                                       // (n_blocks) invalid rays
};

__device__ __forceinline__ float crit_c(int crit, float d) { return crit == 1 ? fabsf(d) : d * d; }

__global__ __launch_bounds__(kThreads) void pixel_c_err_kernel(const PixelCParams p) {
  __shared__ float s_f[4];
  __shared__ unsigned s_u[4];
  const long ray = blockIdx.x * (long)kThreads + threadIdx.x;
  float esum = 0.0f;
  unsigned inv = 0u;
  if (ray < p.B) {
    const bool bad = ray_invalid<false, false>(p, ray);
    const float keep = bad ? 0.0f : 1.0f;
    inv = bad ? 1u : 0u;
    const int nv = p.nv, C = p.C;
    const float* x = p.rgb + ray * nv * C;
    float* g = p.g_rgb ? p.g_rgb + ray * nv * C : nullptr;
    const float norm = p.s_rgb / (float)(C * p.B);
    for (int ch = 0; ch < C; ++ch) {
      const float y = p.rgb_gt[ray * C + ch];
      float emin = 0.0f;
      for (int v = 0; v < nv; ++v) {
        const float val = crit_c(p.crit, x[v * C + ch] - y);
        emin = v == 0 ? val : fminf(emin, val);
      }
      esum += emin * keep;
      if (g) {
        float ties = 0.0f;
        for (int v = 0; v < nv; ++v) ties += crit_c(p.crit, x[v * C + ch] - y) == emin ? 1.0f : 0.0f;
        const float coef = keep != 0.0f ? norm / ties : 0.0f;
        for (int v = 0; v < nv; ++v) {
          const float d = x[v * C + ch] - y;
          const float dc = p.crit == 1 ? sign0(d) : 2.0f * d;
          g[v * C + ch] = crit_c(p.crit, d) == emin ? coef * dc : 0.0f;
        }
      }
    }
    if (p.g_depth) p.g_depth[ray] = 0.0f;
  }
  // the work-group's sums: butterfly per wave, then the four waves in order
  esum = wave_sum(esum), inv = wave_sum(inv);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = esum, s_u[threadIdx.x >> 6] = inv;
  __syncthreads();
  if (threadIdx.x == 0) {
    p.blk_sum[blockIdx.x] = ((s_f[0] + s_f[1]) + s_f[2]) + s_f[3];
    p.blk_inv[blockIdx.x] = ((s_u[0] + s_u[1]) + s_u[2]) + s_u[3];
  }
}

// one work-group: thread t takes partials t, t + 256, ... in order, then the waves' butterflies, then the four waves in order
__global__ __launch_bounds__(kThreads) void pixel_c_final_kernel(const PixelCParams p) {
  __shared__ float s_f[4];
  __shared__ unsigned long long s_c[4];
  float sum = 0.0f;
  unsigned long long inv = 0ull;
  for (long i = threadIdx.x; i < p.n_blocks; i += kThreads) sum += p.blk_sum[i], inv += p.blk_inv[i];
  sum = wave_sum(sum);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) inv += __shfl_xor(inv, off, 64);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = sum, s_c[threadIdx.x >> 6] = inv;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float count = (float)((unsigned long long)p.C * (unsigned long long)p.B);
    p.out[0] = (((s_f[0] + s_f[1]) + s_f[2]) + s_f[3]) / count;
    p.out[1] = 0.0f;
    p.out[2] = (float)(s_c[0] + s_c[1] + s_c[2] + s_c[3]);
    p.out[3] = count;
  }
}

inline void pixel_c_layout(Carver& w, PixelCParams& p, size_t n_blocks) {
  p.blk_sum = w.take<float>(n_blocks);
  p.blk_inv = w.take<unsigned>(n_blocks);
}

}  // namespace

size_t pixel_loss_channels_bytes(long B) {
  if (B <= 0) return 0;
  Carver count(nullptr);
  PixelCParams p;
  pixel_c_layout(count, p, (size_t)((B + kThreads - 1) / kThreads));
  return count.bytes();
}

int pixel_loss_channels_impl(const BtsPixelLossArgs* a, int channels, void* workspace, hipStream_t s) {
  PixelCParams p;
  p.rgb = a->rgb, p.rgb_gt = a->rgb_gt, p.weights = a->weights, p.invalid = a->invalid, p.invalid_wsum = a->invalid_wsum;
  p.invalid_any = a->invalid_any, p.out = a->out, p.g_rgb = a->g_rgb, p.g_depth = a->g_depth;
  p.nv = a->nv, p.K = a->K, p.policy = a->invalid_policy, p.crit = a->criterion, p.C = channels, p.s_rgb = a->scale_rgb;
  p.B = (long)a->B, p.n_blocks = (p.B + kThreads - 1) / kThreads;
  Carver carve(workspace);
  pixel_c_layout(carve, p, (size_t)p.n_blocks);
  pixel_c_err_kernel<<<(unsigned)p.n_blocks, kThreads, 0, s>>>(p);
  pixel_c_final_kernel<<<1, kThreads, 0, s>>>(p);
  return launch_check("%s: pixel loss kernel launch failed (%ld)");
}

}  // namespace bts
