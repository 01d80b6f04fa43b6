// bts_loss_pixel.hip -- the PER-PIXEL criteria of ReconstructionLoss (models/bts/model/loss.py:43-293): criterion l1 / l2, with or
// without median thresholding, under any of the four invalid-ray policies (none, strict, weight_guided, weight_guided_diverse), plus the
// edge-aware smoothness term of bts_loss_tiled.hip (its header has the scheme: the un-normalised edges, the patch's mean inverse depth
// m; the arithmetic both files call is bts_loss_device.h's: inv_depth, edge_term, edge_u_own, depth_grad with the closed-interval clamp
// gradient, sign(0) = 0).  Everything is memory-bound,
// a few bytes per ray and pass: thread = ray, rows read as they lie.  Launches on one stream (a kernel boundary is the only hand-over
// between work-groups):
//   err          keep flag per ray (bts_loss_device.h's ray_invalid, with the diverse policy and its diverse_flag),
//                e[ray, c] = min_v crit(rgb[ray, v, c] - gt[ray, c]) * keep -> workspace; per work-group the sum of e and the
//                invalid rays; with median the histogram of bits 31..21 of e's bit pattern (e >= 0: pattern order = value order);
//                without median the gradient, whose normaliser 1 / (3 B) is known up front
//   hist<1>, <2> median only: bits 20..10 of the e that share the wanted 11 bits, then bits 9..0 of those that share 22 -- the exact radix
//                selection bts_depth_metrics.hip runs (bts_loss_device.h: select_bin), per batch sample, rank (N - 1) / 2 = torch's LOWER median
//   kept         median only: thr[sample] from the last histogram; per work-group the sum and the number of e <= thr (ties all kept)
//   edges, patch smoothness in bts_loss_tiled.hip's geometry and order of sums: per ray the un-normalised edges and u_p, per 16 x 16 tile
//                their sums; per patch m, S and S / m -- bit for bit that kernel's
//   final        one work-group: the partials in index order -> out[4] = [rgb term, sum of the smoothness term, invalid rays, count],
//                the kept count as an integer and the gradient's normaliser
//   grad         median only: d rgb term / d rgb with 1 / count
//   gdepth       g_depth
// No float atomics: every sum is a fixed-order sum of partials (integer atomics build the histograms), reruns are bit-identical.
// The gradient follows torch's amin: tied views share it EQUALLY; sign(0) = 0 for l1, 2 d for l2; no gradient flows through thr.
// An e that is NaN or inf is outside the contract (nothing faults; the selection orders the pattern).
#include <hip/hip_runtime.h>

#include "bts_host.h"
#include "bts_loss_device.h"

namespace bts {

namespace {

constexpr int kThreads = 256;      // (the median selection's work-groups of bts_loss_device.h are this size)

struct PixelParams {
  const float* rgb;
  const float* depth;
  const float* weights;
  const float* invalid;
  const float* invalid_wsum;
  const float* invalid_any;
  const float* rgb_samps;
  const float* rgb_gt;
  float* out;                   // (4)
  float* thresholds;            // (n) or NULL
  long long* kept;              // (1) or NULL
  float* g_rgb;
  float* g_depth;
  int n, ph, pw, nv, K, policy, crit, median, has_eas;
  float s_rgb, s_eas;
  long B, Bs;                   // rays, rays per batch sample
  int blocks_per_sample;        // work-groups of 256 rays per sample
  long n_blocks;
  int area, tiles_x, tiles;     // 16 x 16 tiles per patch row, per patch (bts_loss_tiled.hip's)
  long n_patches, n_tiles;
  // workspace
  float* e;                     // (B, 3)
  unsigned char* keep;          // (B): 0 = invalid ray
  unsigned* hist;               // (n, 3, 2048)
  unsigned* state;              // (n, 8)
  float* thr;                   // (n)
  float* blk_sum;               // (n_blocks)
  unsigned* blk_cnt;            // (n_blocks) kept values
  unsigned* blk_inv;            // (n_blocks) invalid rays
  float* u;                     // (B)
  float2* tile_parts;           // (n_tiles): sum of un-normalised edges, sum of d
  float4* patch_stats;          // (n_patches): m, S, S / m, 0
  float* fin;                   // [0] = s_rgb / count
};
// ... with the automasking bound (loss.py:157-158): e[ray, c] = min(min_v crit, thresh[ray]) * keep -- the ray's ONE bound against each of
// its three channels, before the keep factor and before the median ranking; the gradient of torch's binary min (full below the bound,
// none above, HALF on a tie) multiplies the channel's share.  A type of its own: the kernels without the bound keep their arguments
// and their code
struct PixelParamsThr : PixelParams {
  const float* thresh;          // (B)
};

__device__ __forceinline__ float crit_of(int crit, float d) { return crit == 1 ? fabsf(d) : d * d; }

// d (norm * sum of the kept e) / d rgb of one ray: per channel the views that attain the minimum share the gradient equally (amin)
template <class P>
__device__ __forceinline__ void write_grad(const P& p, long ray, float keep, float thr, float norm) {
  constexpr bool kThr = std::is_same<P, PixelParamsThr>::value;
  const int nv = p.nv;
  const float* x = p.rgb + ray * nv * 3;
  float* g = p.g_rgb + ray * nv * 3;
  const float y[3] = {p.rgb_gt[ray * 3], p.rgb_gt[ray * 3 + 1], p.rgb_gt[ray * 3 + 2]};
  float emin[3] = {0.0f, 0.0f, 0.0f};
  for (int v = 0; v < nv; ++v)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float val = crit_of(p.crit, x[v * 3 + c] - y[c]);
      emin[c] = v == 0 ? val : fminf(emin[c], val);
    }
  float ties[3] = {0.0f, 0.0f, 0.0f};
  for (int v = 0; v < nv; ++v)
#pragma unroll
    for (int c = 0; c < 3; ++c) ties[c] += crit_of(p.crit, x[v * 3 + c] - y[c]) == emin[c] ? 1.0f : 0.0f;
  float coef[3];
  if constexpr (kThr) {
    const float t = p.thresh[ray];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float f = min_grad_factor(emin[c], t);
      coef[c] = (keep != 0.0f && fminf(emin[c], t) * keep <= thr) ? norm / ties[c] * f : 0.0f;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) coef[c] = (keep != 0.0f && emin[c] * keep <= thr) ? norm / ties[c] : 0.0f;
  }
  for (int v = 0; v < nv; ++v)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = x[v * 3 + c] - y[c];
      const float dc = p.crit == 1 ? sign0(d) : 2.0f * d;
      g[v * 3 + c] = crit_of(p.crit, d) == emin[c] ? coef[c] * dc : 0.0f;
    }
}

// the work-group's sum: butterfly per wave, then the four waves in order; every thread gets it.  s_red: 4 words
__device__ __forceinline__ float block_sum(float v, float* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

template <class P>
__global__ __launch_bounds__(kThreads) void pixel_err_kernel(const P p) {
  constexpr bool kThr = std::is_same<P, PixelParamsThr>::value;
  __shared__ unsigned s_hist[kSelBins];
  __shared__ float s_f[4];
  __shared__ unsigned s_u[4];
  if (p.median) {
    for (int i = threadIdx.x; i < kSelBins; i += kThreads) s_hist[i] = 0u;
    __syncthreads();
  }
  const RayPos r = ray_pos(p);
  float esum = 0.0f;
  unsigned inv = 0u;
  if (r.act) {
    const long ray = r.ray;
    const bool bad = ray_invalid<false, true>(p, ray);
    const float keep = bad ? 0.0f : 1.0f;
    p.keep[ray] = bad ? 0 : 1;
    inv = bad ? 1u : 0u;
    const int nv = p.nv;
    const float* x = p.rgb + ray * nv * 3;
    const float y[3] = {p.rgb_gt[ray * 3], p.rgb_gt[ray * 3 + 1], p.rgb_gt[ray * 3 + 2]};
    float emin[3] = {0.0f, 0.0f, 0.0f};
    for (int v = 0; v < nv; ++v)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float val = crit_of(p.crit, x[v * 3 + c] - y[c]);
        emin[c] = v == 0 ? val : fminf(emin[c], val);
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float e = emin[c];
      if constexpr (kThr) e = fminf(e, p.thresh[ray]);
      e = e * keep;
      p.e[ray * 3 + c] = e;
      esum += e;
      if (p.median) atomicAdd(&s_hist[__float_as_uint(e) >> 21], 1u);
    }
    if (!p.median && p.g_rgb) write_grad(p, ray, keep, __uint_as_float(0x7F800000u), p.s_rgb / (float)(3 * p.B));
  }
  const float bs = block_sum(esum, s_f);
  const unsigned bi = block_sum(inv, s_u);
  if (threadIdx.x == 0) p.blk_sum[blockIdx.x] = bs, p.blk_cnt[blockIdx.x] = 0u, p.blk_inv[blockIdx.x] = bi;
  if (p.median) flush_hist(s_hist, p.hist + (size_t)r.sample * kSelHistSample);     // (block_sum's barriers are behind the atomics)
}

// radix passes 1 and 2 of a sample's median (bts_loss_device.h: select_hist_pass, three channels per ray)
template <int PASS>
__global__ __launch_bounds__(kThreads) void pixel_hist_kernel(const PixelParams p) {
  __shared__ unsigned s_hist[kSelBins];
  __shared__ unsigned s_scan[kThreads];
  __shared__ unsigned s_sel[2];
  const RayPos r = ray_pos(p);
  flush_hist(s_hist, select_hist_pass<PASS, 3>(p, r, s_hist, s_scan, s_sel) + PASS * kSelBins);
}

// thr[sample] (bts_loss_device.h: select_threshold); the kept set e <= thr of this work-group's rays.  The note-down stays written out here
// and in loss_med_kept: as a function (p and r by reference or by value, the sample alone handed over) 47 lines of both kernels move.
// So do the sums: this one's block_sum hands every thread the sum, that one adds the four waves in thread 0 -- other instructions
__global__ __launch_bounds__(kThreads) void pixel_kept_kernel(const PixelParams p) {
  __shared__ unsigned s_scan[kThreads];
  __shared__ unsigned s_sel[2];
  __shared__ float s_f[4];
  __shared__ unsigned s_u[4];
  const RayPos r = ray_pos(p);
  const float thr = select_threshold(p, r, s_scan, s_sel);
  if (blockIdx.x == (unsigned)r.sample * p.blocks_per_sample && threadIdx.x == 0) {
    p.thr[r.sample] = thr;
    if (p.thresholds) p.thresholds[r.sample] = thr;
  }
  float sum = 0.0f;
  unsigned cnt = 0u;
  if (r.act) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e = p.e[r.ray * 3 + c];
      if (e <= thr) sum += e, cnt += 1u;
    }
  }
  const float bs = block_sum(sum, s_f);
  const unsigned bc = block_sum(cnt, s_u);
  if (threadIdx.x == 0) p.blk_sum[blockIdx.x] = bs, p.blk_cnt[blockIdx.x] = bc;
}

// smoothness (loss.py:21-40, masked as in :252-254) on the un-normalised inverse depth: bts_loss_tiled.hip's pass 1 per pixel, the
// neighbours read from memory.  The GEOMETRY is that kernel's too -- a work-group per 16 x 16 tile, thread = pixel, butterfly per wave,
// the four waves in order, then (pixel_patch_kernel) its pass 2 -- so that m, S, the per-patch term and g_depth are the tiled kernel's bit
// for bit (tests/test_gpu_loss_pixel.py).  The edges' sum and u_p's own part are bts_loss_device.h's; the weights and the left / upper
// neighbours' part stay written out: behind a function their loads come in another order and the kernel's instructions change
__global__ __launch_bounds__(kThreads) void pixel_edges_kernel(const PixelParams p) {
  __shared__ float s_red[4][2];
  const int tid = threadIdx.x;
  const long patch = blockIdx.x / p.tiles;
  const int r = (int)(blockIdx.x - patch * p.tiles);
  const int ty = r / p.tiles_x;
  const int py = ty * kTile + (tid >> 4), px = (r - ty * p.tiles_x) * kTile + (tid & 15);
  float eas = 0.0f, d = 0.0f;
  if (py < p.ph && px < p.pw) {
    const int pw = p.pw, ph = p.ph;
    const long ray = patch * p.area + (long)py * pw + px;
    const float keep = (p.policy == 0 || p.keep[ray]) ? 1.0f : 0.0f;
    d = inv_depth(p.depth[ray]);
    const float* y = p.rgb_gt + ray * 3;
    const bool has_r = px + 1 < pw, has_b = py + 1 < ph;
    float wx = 0.0f, wy = 0.0f, ex = 0.0f, ey = 0.0f;
    if (has_r) {
      float idx = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) idx += fabsf(y[c] - y[3 + c]);
      wx = expf(-(idx / 3.0f));
      ex = d - inv_depth(p.depth[ray + 1]);
    }
    if (has_b) {
      float idy = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) idy += fabsf(y[c] - y[3 * pw + c]);
      wy = expf(-(idy / 3.0f));
      ey = d - inv_depth(p.depth[ray + pw]);
    }
    eas = edge_term(ex, ey, wx, wy, keep);
    if (p.g_depth) {
      // u_p: this pixel's own edges and the edges its left / upper neighbour owns
      float u = edge_u_own(ex, ey, wx, wy, keep);
      if (px > 0) {
        float il = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) il += fabsf(y[c - 3] - y[c]);
        const float kl = (p.policy == 0 || p.keep[ray - 1]) ? 1.0f : 0.0f;
        u -= sign0(inv_depth(p.depth[ray - 1]) - d) * expf(-(il / 3.0f)) * kl;
      }
      if (py > 0) {
        float iu = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) iu += fabsf(y[c - 3 * pw] - y[c]);
        const float ku = (p.policy == 0 || p.keep[ray - pw]) ? 1.0f : 0.0f;
        u -= sign0(inv_depth(p.depth[ray - pw]) - d) * expf(-(iu / 3.0f)) * ku;
      }
      p.u[ray] = u;
    }
  }
  const float r0 = wave_sum(eas), r1 = wave_sum(d);
  if ((tid & 63) == 0) s_red[tid >> 6][0] = r0, s_red[tid >> 6][1] = r1;
  __syncthreads();
  if (tid == 0)
    p.tile_parts[blockIdx.x] = make_float2(((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0],
                                           ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1]);
}

// one wave per patch: lane l takes tiles l, l + 64, ... in order, then the butterfly (bts_loss_tiled.hip's pass 2, written out in both:
// as a shared function the loop is laid out on its own before it is inlined, which moves both kernels' instruction streams)
__global__ __launch_bounds__(64) void pixel_patch_kernel(const PixelParams p) {
  const int lane = threadIdx.x;
  for (long patch = blockIdx.x; patch < p.n_patches; patch += gridDim.x) {
    const float2* cp = p.tile_parts + patch * p.tiles;
    float a0 = 0.0f, a1 = 0.0f;
    for (int t = lane; t < p.tiles; t += 64) {
      const float2 q = cp[t];
      a0 += q.x, a1 += q.y;
    }
    a0 = wave_sum(a0), a1 = wave_sum(a1);
    if (lane == 0) {
      const float m = a1 / (float)p.area;
      p.patch_stats[patch] = make_float4(m, a0, a0 / m, 0.0f);
    }
  }
}

// one work-group: thread t takes partials t, t + 256, ... in order, then the waves' butterflies, then the four waves in order.  Written
// out here and in loss_med_final: this one reads the smoothness term and the invalid count from patch_stats / blk_inv, that one from parts
__global__ __launch_bounds__(kThreads) void pixel_final_kernel(const PixelParams p) {
  __shared__ float s_f[4];
  __shared__ double s_d[4];
  __shared__ unsigned long long s_c[2][4];
  float sum = 0.0f;
  double eas = 0.0;      // the per-patch terms are added in fp64 and rounded once: the fp32 number nearest to their sum
  unsigned long long cnt = 0ull, inv = 0ull;
  for (long i = threadIdx.x; i < p.n_blocks; i += kThreads) sum += p.blk_sum[i], cnt += p.blk_cnt[i], inv += p.blk_inv[i];
  if (p.has_eas)
    for (long i = threadIdx.x; i < p.n_patches; i += kThreads) eas += p.patch_stats[i].z;
  sum = block_sum(sum, s_f);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64), inv += __shfl_xor(inv, off, 64), eas += __shfl_xor(eas, off, 64);
  if ((threadIdx.x & 63) == 0) s_c[0][threadIdx.x >> 6] = cnt, s_c[1][threadIdx.x >> 6] = inv, s_d[threadIdx.x >> 6] = eas;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long count = p.median ? s_c[0][0] + s_c[0][1] + s_c[0][2] + s_c[0][3] : 3ull * (unsigned long long)p.B;
    const unsigned long long bad = s_c[1][0] + s_c[1][1] + s_c[1][2] + s_c[1][3];
    p.out[0] = sum / (float)count;
    p.out[1] = (float)(((s_d[0] + s_d[1]) + s_d[2]) + s_d[3]);
    p.out[2] = (float)bad;
    p.out[3] = (float)count;
    if (p.kept) p.kept[0] = (long long)count;
    p.fin[0] = p.s_rgb / (float)count;
  }
}

template <class P>
__global__ __launch_bounds__(kThreads) void pixel_grad_kernel(const P p) {
  const RayPos r = ray_pos(p);
  if (r.act) write_grad(p, r.ray, p.keep[r.ray] ? 1.0f : 0.0f, p.thr[r.sample], p.fin[0]);
}

__global__ __launch_bounds__(kThreads) void pixel_gdepth_kernel(const PixelParams p) {
  const long ray = blockIdx.x * (long)kThreads + threadIdx.x;
  if (ray >= p.B) return;
  float g = 0.0f;
  if (p.has_eas) {
    const float u = p.u[ray];
    const float4 st = p.patch_stats[ray / p.area];      // m, S = sum_p u_p d_p = the un-normalised edge sum
    const float dep = p.depth[ray];
    g = depth_grad(u, st.x, st.y, p.area, dep, p.s_eas);
  }
  p.g_depth[ray] = g;
}

__global__ __launch_bounds__(kThreads) void diverse_flags_kernel(const float* __restrict__ rgb_samps, const float* __restrict__ weights,
                                                                 const float* __restrict__ invalid, long B, int K, int nv,
                                                                 float* __restrict__ flags) {
  const long i = blockIdx.x * (long)kThreads + threadIdx.x;
  if (i >= B * nv) return;
  const long ray = i / nv;
  flags[i] = diverse_flag(rgb_samps, weights, invalid, ray, (int)(i - ray * nv), nv, K) ? 1.0f : 0.0f;
}

struct Geom {
  long Bs, n_blocks, n_patches, n_tiles;
  int blocks_per_sample, area, tiles_x, tiles;
};
inline Geom geom_of(long B, int n, int ph, int pw) {
  Geom g;
  g.Bs = B / n;
  g.blocks_per_sample = (int)((g.Bs + kThreads - 1) / kThreads);
  g.n_blocks = (long)n * g.blocks_per_sample;
  g.area = ph * pw;
  g.n_patches = B / g.area;
  g.tiles_x = (pw + kTile - 1) / kTile;
  g.tiles = ((ph + kTile - 1) / kTile) * g.tiles_x;
  g.n_tiles = g.n_patches * g.tiles;
  return g;
}

// THE layout of bts_pixel_loss's workspace: e, keep flags, histograms, selection state, thresholds, three partials per work-group, u,
// tile partials, patch statistics, the final words
inline void pixel_layout(Carver& w, PixelParams& p, size_t B, size_t n, const Geom& g) {
  p.e = w.take<float>(B * 3);
  p.keep = w.take<unsigned char>(B);
  p.hist = w.take<unsigned>(n * kSelHistSample);
  p.state = w.take<unsigned>(n * kSelStateSample);
  p.thr = w.take<float>(n);
  p.blk_sum = w.take<float>((size_t)g.n_blocks);
  p.blk_cnt = w.take<unsigned>((size_t)g.n_blocks);
  p.blk_inv = w.take<unsigned>((size_t)g.n_blocks);
  p.u = w.take<float>(B);
  p.tile_parts = w.take<float2>((size_t)g.n_tiles);
  p.patch_stats = w.take<float4>((size_t)g.n_patches);
  p.fin = w.take<float>(4);
}

}  // namespace

size_t pixel_loss_bytes(long B, int n, int ph, int pw) {
  if (B <= 0 || n <= 0 || ph <= 0 || pw <= 0 || (long)ph * pw > B) return 0;
  Carver count(nullptr);
  PixelParams p;
  pixel_layout(count, p, (size_t)B, (size_t)n, geom_of(B, n, ph, pw));
  return count.bytes();
}

int pixel_loss_impl(const BtsPixelLossArgs* a, void* workspace, hipStream_t s, const float* thresh) {
  PixelParamsThr pt;
  pt.thresh = thresh;
  PixelParams& p = pt;
  p.rgb = a->rgb, p.depth = a->depth, p.weights = a->weights, p.invalid = a->invalid, p.invalid_wsum = a->invalid_wsum;
  p.invalid_any = a->invalid_any, p.rgb_samps = a->rgb_samps, p.rgb_gt = a->rgb_gt;
  p.out = a->out, p.thresholds = a->thresholds, p.kept = (long long*)a->kept, p.g_rgb = a->g_rgb, p.g_depth = a->g_depth;
  p.n = a->n, p.ph = a->patch_h, p.pw = a->patch_w, p.nv = a->nv, p.K = a->K, p.policy = a->invalid_policy, p.crit = a->criterion;
  p.median = a->median_thresholding ? 1 : 0, p.has_eas = a->edge_aware_smoothness ? 1 : 0;
  p.s_rgb = a->scale_rgb, p.s_eas = a->scale_eas;
  p.B = (long)a->B;
  const Geom g = geom_of(p.B, p.n, p.ph, p.pw);
  p.Bs = g.Bs, p.blocks_per_sample = g.blocks_per_sample, p.n_blocks = g.n_blocks, p.area = g.area, p.tiles_x = g.tiles_x, p.tiles = g.tiles;
  p.n_patches = g.n_patches, p.n_tiles = g.n_tiles;
  Carver carve(workspace);
  pixel_layout(carve, p, (size_t)p.B, (size_t)p.n, g);
  const unsigned grid = (unsigned)g.n_blocks;
  if (p.median && hipMemsetAsync(p.hist, 0, (size_t)p.n * kSelHistSample * sizeof(unsigned), s) != hipSuccess) {
    set_error("%s: clearing the histograms failed", "bts_pixel_loss");
    return BTS_E_LAUNCH;
  }
  if (thresh)
    pixel_err_kernel<PixelParamsThr><<<grid, kThreads, 0, s>>>(pt);
  else
    pixel_err_kernel<PixelParams><<<grid, kThreads, 0, s>>>(p);
  if (p.median) {
    pixel_hist_kernel<1><<<grid, kThreads, 0, s>>>(p);
    pixel_hist_kernel<2><<<grid, kThreads, 0, s>>>(p);
    pixel_kept_kernel<<<grid, kThreads, 0, s>>>(p);
  }
  if (p.has_eas) {
    pixel_edges_kernel<<<(unsigned)g.n_tiles, kThreads, 0, s>>>(p);
    pixel_patch_kernel<<<(unsigned)(g.n_patches < 65536 ? g.n_patches : 65536), 64, 0, s>>>(p);
  }
  pixel_final_kernel<<<1, kThreads, 0, s>>>(p);
  if (p.median && p.g_rgb) {
    if (thresh)
      pixel_grad_kernel<PixelParamsThr><<<grid, kThreads, 0, s>>>(pt);
    else
      pixel_grad_kernel<PixelParams><<<grid, kThreads, 0, s>>>(p);
  }
  if (p.g_depth) pixel_gdepth_kernel<<<(unsigned)((p.B + kThreads - 1) / kThreads), kThreads, 0, s>>>(p);
  return launch_check("%s: pixel loss kernel launch failed (%ld)");
}

int diverse_flags_launch(const float* rgb_samps, const float* weights, const float* invalid, long B, int K, int nv, float* flags,
                         hipStream_t s) {
  diverse_flags_kernel<<<(unsigned)((B * nv + kThreads - 1) / kThreads), kThreads, 0, s>>>(rgb_samps, weights, invalid, B, K, nv, flags);
  return launch_check("%s: diverse flags kernel launch failed (%ld)");
}

}  // namespace bts
