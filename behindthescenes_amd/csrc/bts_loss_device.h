// bts_loss_device.h -- the rules the loss kernels share, each written ONCE: bts_loss.hip (one wave per patch of at most 64 pixels),
// bts_loss_tiled.hip (16 x 16 tiles of patches of any size), bts_loss_pixel.hip (per-pixel criteria), bts_automask.hip (the error map)
// and, for the rank selection, bts_depth_metrics.hip include it.  "Bit for bit the other kernel's result" means: both call the function
// below.  Device code only, every function inlined into its kernel (select_bin: left to the compiler, as before).  The evaluation
// kernels' shared rules are bts_eval_device.h's; its lane-0 __shfl_down sums are NOT the wave_sum below (every lane holds that one).
//   - wave sums, sign(0) = 0, the gradient factor of torch's binary min
//   - the invalid-ray rule (loss.py:100-118) for every policy, over the kernel's parameter struct
//   - the 3 x 3 Gaussian window of SSIM (layers.py:92-101), the per-channel SSIM term and its three backward coefficients
//   - edge-aware smoothness (loss.py:21-40): the inverse clamped depth, a pixel's own edges and their part of u_p, the depth gradient
//   - the rank selection in a histogram of 2 048 bins
//   - the median of a plane per batch sample on top of it: the workspace constants, the (sample, 256 rays) position, the radix passes,
//     the threshold (bts_loss_pixel.hip and bts_loss_tiled.hip's median variant; bts_depth_metrics.hip selects two keys at once)
// What is NOT here although two files write it: a rule stays in its kernel where calling it from this header changes that kernel's
// instructions (every kernel of the five files is the instruction stream it was before the header existed, tools/asm_compare.py).  The
// compiler simplifies a function on its own before it inlines it, so a function with a loop, or one whose arguments are loaded in another
// order than the inline text read them, gives other block orders and register numbers.  Those sites carry a comment that says so.
#pragma once
#include <hip/hip_runtime.h>

namespace bts {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float sign0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// d min(e, t) / d e as torch.min(a, b) forms it: full below the bound, none above, HALF on a tie
__device__ __forceinline__ float min_grad_factor(float e, float t) { return e < t ? 1.0f : (e > t ? 0.0f : 0.5f); }

// ---- invalid rays
// weight_guided_diverse per (ray, view), loss.py:109-118: (sum_k invalid w > .9) | (mean_c std_k(rgb_samps) < .01); the unbiased std
// (K - 1) in fp32, the mean first, then the squared deviations, k ascending; K == 1: 0 / 0 = NaN and the comparison is false
__device__ __forceinline__ bool diverse_flag(const float* __restrict__ rgb_samps, const float* __restrict__ weights,
                                             const float* __restrict__ invalid, long ray, int v, int nv, int K) {
  float s = 0.0f;
  for (int k = 0; k < K; ++k) s += invalid[(ray * K + k) * nv + v] * weights[ray * K + k];
  float sd = 0.0f;
  const long stride = (long)nv * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* x = rgb_samps + (ray * K * nv + v) * 3 + c;
    float m = 0.0f;
    for (int k = 0; k < K; ++k) m += x[k * stride];
    m = m / (float)K;
    float q = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float d = x[k * stride] - m;
      q += d * d;
    }
    sd += sqrtf(q / (float)(K - 1));
  }
  return (s > 0.9f) || (sd / 3.0f < 0.01f);
}

// invalid ray?  (loss.py:100-118)  Policy 0 none, 1 strict (any sample, every view), 2 weight_guided (sum_k w_k invalid_k > .9, every
// view), 3 weight_guided_diverse (every view's diverse flag).  invalid_wsum / invalid_any: the renderer's epilogue already reduced over
// the samples.  P: the kernel's parameter struct.  kVec4: P has `vec4` -- with one view the rows of K floats are read as 16-byte loads,
// the sums in the same order.  kDiverse: P has `rgb_samps` and knows policy 3.
template <bool kVec4, bool kDiverse, class P>
__device__ __forceinline__ bool ray_invalid(const P& p, long ray) {
  if (p.policy == 0) return false;
  const int nv = p.nv, K = p.K;
  if constexpr (kVec4) {
    if (p.vec4 && !(p.policy == 2 ? p.invalid_wsum : p.invalid_any)) {
      const float4* i4 = reinterpret_cast<const float4*>(p.invalid + ray * K);
      if (p.policy == 2) {
        const float4* w4 = reinterpret_cast<const float4*>(p.weights + ray * K);
        float s = 0.0f;
        for (int k = 0; k < K / 4; ++k) {
          const float4 i = i4[k], w = w4[k];
          s += i.x * w.x, s += i.y * w.y, s += i.z * w.z, s += i.w * w.w;
        }
        return s > 0.9f;
      }
      bool any_k = false;
      for (int k = 0; k < K / 4; ++k) {
        const float4 i = i4[k];
        any_k = any_k || (i.x > 0.5f) || (i.y > 0.5f) || (i.z > 0.5f) || (i.w > 0.5f);
      }
      return any_k;
    }
  }
  bool all_v = true;
  for (int v = 0; v < nv; ++v) {
    if constexpr (kDiverse) {
      if (p.policy == 3) {
        all_v = all_v && diverse_flag(p.rgb_samps, p.weights, p.invalid, ray, v, nv, K);
        continue;
      }
    }
    if (p.policy == 2 && p.invalid_wsum) {
      all_v = all_v && (p.invalid_wsum[ray * nv + v] > 0.9f);
    } else if (p.policy == 1 && p.invalid_any) {
      all_v = all_v && (p.invalid_any[ray * nv + v] > 0.5f);
    } else if (p.policy == 2) {
      float s = 0.0f;
      for (int k = 0; k < K; ++k) s += p.invalid[(ray * K + k) * nv + v] * p.weights[ray * K + k];
      all_v = all_v && (s > 0.9f);
    } else {
      bool any_k = false;
      for (int k = 0; k < K; ++k) any_k = any_k || (p.invalid[(ray * K + k) * nv + v] > 0.5f);
      all_v = all_v && any_k;
    }
  }
  return all_v;
}

// ---- SSIM
constexpr float kGa = 0.0947f, kGb = 0.1183f, kGc = 0.1478f;   // layers.py:92-101 window: corner, edge, centre
constexpr float kSsimC1 = 0.01f * 0.01f, kSsimC2 = 0.03f * 0.03f;

// Gaussian-weighted sum of the 3x3 neighbourhood of `centre` in a zero-bordered plane of row length `ld`, row-major order of additions
__device__ __forceinline__ float gauss9(const float* pl, int centre, int ld) {
  const float* r0 = pl + centre - ld;
  const float* r1 = pl + centre;
  const float* r2 = pl + centre + ld;
  float s = kGa * r0[-1];
  s += kGb * r0[0], s += kGa * r0[1];
  s += kGb * r1[-1], s += kGc * r1[0], s += kGb * r1[1];
  s += kGa * r2[-1], s += kGb * r2[0], s += kGa * r2[1];
  return s;
}

// one channel's SSIM term clamp(1 - n / d, 0, 1) / 2 from the windowed sums mu = G * x, gxx = G * x^2, gxy = G * xy (and y's)
__device__ __forceinline__ float ssim_term(float mu_x, float gxx, float gxy, float mu_y, float gyy) {
  const float mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
  const float sx = gxx - mxx, sy = gyy - myy, sxy = gxy - mxy;
  const float nn = (2.0f * mxy + kSsimC1) * (2.0f * sxy + kSsimC2);
  const float dd = (mxx + myy + kSsimC1) * (sx + sy + kSsimC2);
  return fminf(fmaxf(1.0f - nn / dd, 0.0f), 1.0f) / 2.0f;
}

// what a pixel with upstream gradient `up` (d loss / d e of this pixel) hands its neighbours: the coefficients of d mu_x, d G*x^2 and
// d G*xy of one channel.  All zero where the clamp is active
struct SsimCoef {
  float k_mu, k_xx, k_xy;
};
__device__ __forceinline__ SsimCoef ssim_coef(float mu_x, float gxx, float gxy, float mu_y, float gyy, float up) {
  SsimCoef k = {0.0f, 0.0f, 0.0f};
  const float mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
  const float sx = gxx - mxx, sy = gyy - myy, sxy = gxy - mxy;
  const float A1 = 2.0f * mxy + kSsimC1, A2 = 2.0f * sxy + kSsimC2, B1 = mxx + myy + kSsimC1, B2 = sx + sy + kSsimC2;
  const float nn = A1 * A2, dd = B1 * B2;
  const float t = 1.0f - nn / dd;
  if (t >= 0.0f && t <= 1.0f) {   // torch.clamp passes the gradient on the closed interval
    // d(ssim) = -1/2 d(n/d);  d(n/d) = dn/d - n dd/d^2
    const float gs = up * (0.85f / 3.0f) * (-0.5f);
    const float dn_mu = 2.0f * mu_y * (A2 - A1), dn_xy = 2.0f * A1;
    const float dd_mu = 2.0f * mu_x * (B2 - B1), dd_xx = B1;
    const float inv_d = 1.0f / dd, n_d2 = nn * inv_d * inv_d;
    k.k_mu = gs * (dn_mu * inv_d - n_d2 * dd_mu);
    k.k_xy = gs * (dn_xy * inv_d);
    k.k_xx = gs * (-n_d2 * dd_xx);
  }
  return k;
}

// ---- edge-aware smoothness
constexpr int kTile = 16;   // tile side of the smoothness partial sums (the tiled kernel's tiles; the pixel kernels keep its geometry)

// d = 1 / clamp(depth, 1e-3, 80)
__device__ __forceinline__ float inv_depth(float depth) { return 1.0f / fminf(fmaxf(depth, 1e-3f), 80.0f); }

// A pixel owns the edges to its right and lower neighbour: ex = d_p - d_right, ey = d_p - d_below with weights wx, wy = exp(-mean_c |dy_c|)
// of the ground-truth colours (0 where there is no neighbour).  Its term of the un-normalised sum, and what those two edges add to
// u_p = d (sum of edges) / d d_p; the edges its left / upper neighbour q owns take sign0(d_q - d_p) w keep_q from u_p
__device__ __forceinline__ float edge_term(float ex, float ey, float wx, float wy, float keep) { return (fabsf(ex) * wx + fabsf(ey) * wy) * keep; }
__device__ __forceinline__ float edge_u_own(float ex, float ey, float wx, float wy, float keep) {
  return sign0(ex) * wx * keep + sign0(ey) * wy * keep;
}

// d loss / d depth_j of the smoothness term: dn_p = d_p / m, m = mean d over the patch's `area` pixels, so d E / d d_j =
// u_j / m - S / (m^2 N) with S = sum_p u_p d_p (= the un-normalised edge sum: E is homogeneous of degree 1), times d d / d depth, which
// torch.clamp passes on the closed interval, times the upstream factor s_eas.  (N: the callers' integer type of `area`, converted here.
// Where the conversion and the callers' loads of u, the patch statistics and the depth stand decides the kernels' register numbering)
template <class N>
__device__ __forceinline__ float depth_grad(float u, float m, float S, N area, float depth, float s_eas) {
  const float dcl = fminf(fmaxf(depth, 1e-3f), 80.0f);
  const float gd = u / m - S / (m * m * (float)area);
  return ((depth >= 1e-3f && depth <= 80.0f) ? -gd / (dcl * dcl) : 0.0f) * s_eas;
}

// ---- rank selection
// The bin of `hist` (2 048 bins) that holds the element of rank `rank` (0-based; median != 0: rank = (total - 1) / 2 of the histogram's
// own total = torch's LOWER median) and the rank inside that bin.  Every lane takes eight consecutive bins, the work-group scans the 256
// sums.  out: bin, rank inside, and with kTotal the total; bin = rank = 0 when rank >= total.  All 256 lanes of the work-group call
// this; s_scan holds 256 words.
template <bool kTotal>
__device__ void select_bin(const unsigned* __restrict__ hist, int median, unsigned rank, unsigned* s_scan, unsigned* out) {
  constexpr int kLanes = 256;
  const int t = threadIdx.x;
  const uint4 lo = reinterpret_cast<const uint4*>(hist)[t * 2], hi = reinterpret_cast<const uint4*>(hist)[t * 2 + 1];
  const unsigned h[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  unsigned local = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) local += h[k];
  s_scan[t] = local;
  __syncthreads();
  for (int o = 1; o < kLanes; o <<= 1) {
    const unsigned v = t >= o ? s_scan[t - o] : 0u;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const unsigned total = s_scan[kLanes - 1], incl = s_scan[t], excl = incl - local;
  if (median) rank = total ? (total - 1) / 2 : 0u;
  if (t == 0) {
    if constexpr (kTotal) out[2] = total;
    if (rank >= total) out[0] = 0u, out[1] = 0u;
  }
  if (rank >= excl && rank < incl) {   // one lane, when rank < total
    unsigned r = rank - excl, rem = 0u;
    int bin = -1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (bin < 0) {
        if (r < h[k]) bin = k, rem = r;
        else r -= h[k];
      }
    }
    out[0] = (unsigned)(t * 8 + bin), out[1] = rem;
  }
  __syncthreads();
}

// ---- the median of a plane e of CHANNELS values per ray, per batch sample (loss.py:163-167): three radix passes over select_bin, run by
// work-groups of 256 rays that never straddle two samples.  bts_loss_pixel.hip (three channels per ray) and the median variant of
// bts_loss_tiled.hip (one) launch them; P, the kernel's parameter struct, has e, hist (n, 3, 2 048), state (n, 8), thr (n), thresholds,
// Bs (rays per sample) and blocks_per_sample.  THE protocol between the launches: a sample's first work-group notes the selected prefix
// and the rank inside it in state[0, 1] after pass 0's histogram and in state[4, 5] after pass 1's; the NEXT launch reads them.
// Two pieces of the passes stay in the kernels, because inside a function here they move a kernel's instructions (each kernel is the
// stream it was, tools/asm_compare.py): the flush behind select_hist_pass -- bts_loss_pixel.hip's is flush_hist on a pointer,
// bts_loss_tiled.hip's two are loops written out, one of them indexing from the sample's base -- and the note-down of thr behind
// select_threshold.  Both sites say what was tried.
constexpr int kSelBins = 2048;
constexpr int kSelHistSample = 3 * kSelBins;      // three radix passes per batch sample
constexpr int kSelStateSample = 8;

// which sample and which ray a thread of the (sample, 256 rays) work-groups takes
struct RayPos {
  int sample;
  long ray;
  bool act;
};
template <class P>
__device__ __forceinline__ RayPos ray_pos(const P& p) {
  RayPos r;
  r.sample = (int)(blockIdx.x / p.blocks_per_sample);
  const long in_sample = (long)(blockIdx.x - (unsigned)r.sample * p.blocks_per_sample) * 256 + threadIdx.x;
  r.act = in_sample < p.Bs;
  r.ray = (long)r.sample * p.Bs + (r.act ? in_sample : 0);
  return r;
}

// the work-group's non-zero bins into the sample's histogram (bts_loss_pixel.hip's three flushes)
__device__ __forceinline__ void flush_hist(const unsigned* s_hist, unsigned* dst) {
  for (int i = threadIdx.x; i < kSelBins; i += 256) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(&dst[i], c);
  }
}

// radix passes 1 and 2 up to the flush: bits 20..10 of the e that share the wanted 11 bits, then bits 9..0 of those that share 22, counted
// in s_hist.  -> the sample's three histograms; the caller adds s_hist's non-zero bins to the one at PASS * kSelBins.  r: ray_pos(p), taken
// in the kernel (taken in here, loss_med_hist's loads are scheduled in another order).  s_hist: kSelBins words, s_scan: 256, s_sel: 2 --
// the calling kernel's LDS
template <int PASS, int CHANNELS, class P>
__device__ __forceinline__ unsigned* select_hist_pass(const P& p, const RayPos& r, unsigned* s_hist, unsigned* s_scan, unsigned* s_sel) {
  unsigned* hist_s = p.hist + (size_t)r.sample * kSelHistSample;
  unsigned* state_s = p.state + (size_t)r.sample * kSelStateSample;
  for (int i = threadIdx.x; i < kSelBins; i += 256) s_hist[i] = 0u;
  unsigned want;
  if (PASS == 1) {
    select_bin<false>(hist_s, 1, 0u, s_scan, s_sel);
    want = s_sel[0];
    if (blockIdx.x == (unsigned)r.sample * p.blocks_per_sample && threadIdx.x == 0) state_s[0] = want, state_s[1] = s_sel[1];
  } else {
    select_bin<false>(hist_s + kSelBins, 0, state_s[1], s_scan, s_sel);
    want = (state_s[0] << 11) | s_sel[0];
    if (blockIdx.x == (unsigned)r.sample * p.blocks_per_sample && threadIdx.x == 0) state_s[4] = want, state_s[5] = s_sel[1];
  }
  __syncthreads();
  if (r.act) {
#pragma unroll
    for (int c = 0; c < CHANNELS; ++c) {
      const unsigned key = __float_as_uint(p.e[r.ray * CHANNELS + c]);
      if (PASS == 1) {
        if ((key >> 21) == want) atomicAdd(&s_hist[(key >> 10) & 2047u], 1u);
      } else {
        if ((key >> 10) == want) atomicAdd(&s_hist[key & 1023u], 1u);
      }
    }
  }
  __syncthreads();
  return hist_s;
}

// thr[sample] = the value whose pattern is the 22-bit prefix and the last histogram's bin; the sample's first work-group notes it down
template <class P>
__device__ __forceinline__ float select_threshold(const P& p, const RayPos& r, unsigned* s_scan, unsigned* s_sel) {
  const unsigned* state_s = p.state + (size_t)r.sample * kSelStateSample;
  select_bin<false>(p.hist + (size_t)r.sample * kSelHistSample + 2 * kSelBins, 0, state_s[5], s_scan, s_sel);
  return __uint_as_float((state_s[4] << 10) | s_sel[0]);
}

}  // namespace bts
