// bts_loss_tiled.hip -- the photometric loss of bts_loss.hip for patches of ANY size (the trainer's default 16 x 16 patch, sample_mode
// "image", the validation loss on whole 192 x 640 frames): a patch is cut into 16 x 16 tiles, one work-group of 256 threads per tile,
// thread = pixel.  The arithmetic per pixel is that of bts_loss.hip, through the functions both call (bts_loss_device.h: the SSIM term
// and its backward coefficients with the closed-interval clamp gradient, sign(0) = 0, the depth gradient; bts_loss.hip's header has the
// formulas); what is new is that 3x3 neighbourhoods cross tile borders and that the smoothness term needs the PATCH's mean inverse
// depth.  Up to four launches on one stream (a kernel boundary is the only hand-over between work-groups; no float atomics, every sum
// is a fixed-order sum of partials, reruns are bit-identical):
//   keep, per ray      the invalid-ray policy once per ray (thread = ray; bts_loss_device.h's ray_invalid with 16-byte loads of the
//                      weights / invalid rows when nv = 1 and K is a multiple of 4: the validation frame) -> one byte per ray; not
//                      launched with policy none
//   pass 1, per tile   stages ground truth, that keep flag and d = 1 / clamp(depth) of the 18 x 18 halo in LDS, then one view's colours at a
//                      time; per pixel: e_v for every view, v*, the rgb term; with gradients the three SSIM backward coefficients
//                      per channel of v* (workspace, nine planes) and v* itself (-1: no gradient leaves this pixel); the
//                      UN-normalised smoothness edges |d_p - d_q| w keep and u_p = d (sum of edges) / d d_p up to the factor 1 / m.
//                      Per tile: [sum rgb term, sum un-normalised edges, sum d, invalid rays] -> workspace.
//   pass 2, per patch  adds the tile partials (one wave: lane l takes tiles l, l + 64, ... in order, then the butterfly), m = mean d,
//                      parts[patch] = [rgb, edges / m, invalid, 0].  |dn_p - dn_q| = |d_p - d_q| / m, so no pre-pass for m is needed,
//                      and since the smoothness sum E is homogeneous of degree 1 in dn, sum_p u_p d_p = m E = the un-normalised sum.
//   pass 3, per tile   only with gradients: g_rgb[p, v, c] gathers the coefficients of the nine neighbours whose v* is v (staged with
//                      their halo in LDS); g_depth[p] = s_eas * (u_p / m - S / (m^2 N)) * d clamp / d depth.
// One difference from the wave kernel in the last bit: it takes sign(dn_p - dn_q), this file sign(d_p - d_q) -- equal unless two
// different d round to the same dn, where the reference sits on the kink of |.| anyway.
// LDS: pass 1 8 planes of 324 floats + 16 partials = 10 432 bytes; pass 3 10 planes of 324 = 12 960 bytes.  Four waves share the
// planes, so every hand-over is a real __syncthreads() (the wave kernel's wave-scope fence is not enough here).
//
// MEDIAN THRESHOLDING (loss.py:163-167) for l1+ssim, bts_photometric_loss_median: the same passes over a third parameter struct
// (TiledParamsMed), joined to the exact radix selection of bts_loss_pixel.hip (bts_loss_device.h: select_bin).  Every pixel's error must
// exist before any pixel's gradient can be written and the normaliser 1 / count is only known on the device, so:
//   pass 1 (median)    as above with a UNIT upstream gradient (times the automasking factor when a bound is given: a run-time NULL);
//                      e = min(e_min, t) * keep -> workspace (B); bits 31..21 of e's pattern -> the batch sample's histogram (in LDS,
//                      flushed with integer atomics; a tile lies in one patch, a patch in one sample)
//   hist<1>, <2>, kept ray-wise over that plane: bits 20..10, bits 9..0, then thr[sample] (rank (N - 1) / 2: torch's LOWER median) and per
//                      work-group the sum and the number of e <= thr (ties all kept)
//   pass 2             unchanged: parts[patch] = [sum of e BEFORE thresholding, edges / m, invalid rays, 0]
//   final              one work-group, partials in index order: out[4] = [sum of kept e / count, sum of the smoothness term, invalid
//                      rays, count], the count as int64, fin[0] = s_rgb / count
//   pass 3 (median)    a neighbour q with e[q] > thr[sample] is staged with v* = -1 (it hands nothing on, whether or not the receiving
//                      pixel is kept); the gathered sum, the centre's L1 term included, is multiplied by fin[0] -- the coefficients are
//                      linear in the upstream gradient, so scaling after the gather is exact up to one rounding
// LDS of the median pass 1: the 10 432 bytes above + 8 192 of histogram; pass 3 as above.
#include <hip/hip_runtime.h>

#include "bts_host.h"
#include "bts_loss_device.h"

namespace bts {

namespace {

// (kTile = 16, bts_loss_device.h: interior pixels per tile side -- 256 threads, thread = pixel)
constexpr int kLd = kTile + 2;         // row length of a plane with its one-pixel halo
constexpr int kHalo = kLd * kLd;       // 324

struct TiledParams {
  const float* rgb;
  const float* depth;
  const float* weights;
  const float* invalid;
  const float* invalid_wsum;
  const float* invalid_any;
  const float* rgb_gt;
  float* parts;
  float* g_rgb;
  float* g_depth;
  int n_patches, ph, pw, nv, K, policy;
  float s_rgb, s_eas;
  int has_eas;
  int tiles_x, tiles;      // tiles per patch row, tiles per patch
  long B;                  // rays
  // workspace
  float4* tile_parts;      // (n_patches * tiles): sum rgb term, sum un-normalised edges, sum d, invalid rays
  float4* patch_stats;     // (n_patches): m, un-normalised edge sum, 0, 0
  int* vstar;              // (B)
  float* coef;             // (9, B): plane c * 3 + {mu, xx, xy}
  float* u;                // (B)
  unsigned char* keep;     // (B): 0 = invalid ray
  int vec4;                // weights / invalid rows can be read as float4 (nv == 1, K % 4 == 0, 16-byte aligned bases)
};
// ... with the automasking bound (bts_loss.hip: LossParamsThr): pass 1 bounds e and scales the pixel's upstream gradient by the factor
// of torch's binary min (1, 0 or -- on a tie -- .5), which therefore sits in the coefficients BEFORE the neighbours gather them in pass 3;
// the factor itself goes to the workspace for pass 3's L1 term.  A type of its own: the kernels without the bound keep their arguments
// and their code
struct TiledParamsThr : TiledParams {
  const float* thresh;     // (B)
  float* fthr;             // workspace (B): d min(e, thresh) / d e
};

// ... with median thresholding (loss.py:163-167; the header has the pipeline).  `thresh` may be NULL here (no automasking bound): a
// run-time branch of this variant only.  A third type: the two above keep their arguments and their code
struct TiledParamsMed : TiledParamsThr {
  float* out;              // (4)
  float* thresholds;       // (n) or NULL
  long long* kept;         // (1) or NULL
  int n, pps;              // batch samples, patches per sample
  long Bs;                 // rays per sample
  int blocks_per_sample;   // work-groups of 256 rays per sample (hist / kept kernels)
  long n_blocks;
  // workspace
  float* e;                // (B): min(e_min, t) * keep
  unsigned* hist;          // (n, 3, 2048)
  unsigned* state;         // (n, 8): [0, 1] prefix and rank after the first histogram, [4, 5] after the second
  float* thr;              // (n)
  float* blk_sum;          // (n_blocks) sum of the kept e
  unsigned* blk_cnt;       // (n_blocks) kept pixels
  float* fin;              // [0] = s_rgb / count
};
// the tile's histogram of the median pass 1: LDS of the kernels that call this, and of no other
__device__ __forceinline__ unsigned* med_hist() {
  __shared__ unsigned s_hist[kSelBins];
  return s_hist;
}

// gauss9 (bts_loss_device.h) of the product of two planes, in its order of additions
__device__ __forceinline__ float gauss9_prod(const float* pa, const float* pb, int ctr) {
  const float* a0 = pa + ctr - kLd;
  const float* a1 = pa + ctr;
  const float* a2 = pa + ctr + kLd;
  const float* b0 = pb + ctr - kLd;
  const float* b1 = pb + ctr;
  const float* b2 = pb + ctr + kLd;
  float s = kGa * (a0[-1] * b0[-1]);
  s += kGb * (a0[0] * b0[0]), s += kGa * (a0[1] * b0[1]);
  s += kGb * (a1[-1] * b1[-1]), s += kGc * (a1[0] * b1[0]), s += kGb * (a1[1] * b1[1]);
  s += kGa * (a2[-1] * b2[-1]), s += kGb * (a2[0] * b2[0]), s += kGa * (a2[1] * b2[1]);
  return s;
}
// ... of a plane of which only the neighbours flagged in `m` (bit 3 * row + column) count
__device__ __forceinline__ float gauss9_masked(const float* pl, int ctr, unsigned m) {
  const float* r0 = pl + ctr - kLd;
  const float* r1 = pl + ctr;
  const float* r2 = pl + ctr + kLd;
  float s = kGa * ((m & 1u) ? r0[-1] : 0.0f);
  s += kGb * ((m & 2u) ? r0[0] : 0.0f), s += kGa * ((m & 4u) ? r0[1] : 0.0f);
  s += kGb * ((m & 8u) ? r1[-1] : 0.0f), s += kGc * ((m & 16u) ? r1[0] : 0.0f), s += kGb * ((m & 32u) ? r1[1] : 0.0f);
  s += kGa * ((m & 64u) ? r2[-1] : 0.0f), s += kGb * ((m & 128u) ? r2[0] : 0.0f), s += kGa * ((m & 256u) ? r2[1] : 0.0f);
  return s;
}

// which tile of which patch a work-group takes (1-D grid over n_patches x tiles; beyond kMaxGrid work-groups each takes several)
constexpr long kMaxGrid = 1L << 20;
struct TilePos {
  int patch, y0, x0;
  long base;     // first ray of the patch
};
__device__ __forceinline__ TilePos tile_pos(const TiledParams& p, long blk) {
  TilePos t;
  t.patch = (int)(blk / p.tiles);
  const int r = (int)(blk - (long)t.patch * p.tiles);
  const int ty = r / p.tiles_x;
  t.y0 = ty * kTile, t.x0 = (r - ty * p.tiles_x) * kTile;
  t.base = (long)t.patch * ((long)p.ph * p.pw);
  return t;
}

__global__ __launch_bounds__(256) void loss_tiled_keep(const TiledParams p) {
  for (long ray = blockIdx.x * 256L + threadIdx.x; ray < p.B; ray += gridDim.x * 256L) p.keep[ray] = ray_invalid<true, false>(p, ray) ? 0 : 1;
}

template <class P>
__global__ __launch_bounds__(256) void loss_tiled_pass1(const P p, const long n_tiles) {
  constexpr bool kThr = std::is_same<P, TiledParamsThr>::value;
  constexpr bool kMed = std::is_same<P, TiledParamsMed>::value;
  __shared__ float sY[3][kHalo], sX[3][kHalo], sD[kHalo], sK[kHalo];
  __shared__ float sRed[4][4];
  const int tid = threadIdx.x;
  for (long blk = blockIdx.x; blk < n_tiles; blk += gridDim.x) {
  if (blk != blockIdx.x) __syncthreads();      // the previous tile's readers are done with the planes and sRed
  const TilePos tp = tile_pos(p, blk);
  const int ph = p.ph, pw = p.pw, nv = p.nv;
  if constexpr (kMed)      // (the barriers below stand between this, the atomics and the flush)
    for (int i = tid; i < kSelBins; i += 256) med_hist()[i] = 0u;

  // ---- halo: ground truth, keep flag, d = 1 / clamp(depth); zero outside the patch (the SSIM window's zero padding)
  for (int i = tid; i < kHalo; i += 256) {
    const int hy = i / kLd, hx = i - hy * kLd;
    const int py = tp.y0 + hy - 1, px = tp.x0 + hx - 1;
    float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, d = 0.0f, k = 0.0f;
    if (py >= 0 && py < ph && px >= 0 && px < pw) {
      const long ray = tp.base + (long)py * pw + px;
      y0 = p.rgb_gt[ray * 3], y1 = p.rgb_gt[ray * 3 + 1], y2 = p.rgb_gt[ray * 3 + 2];
      k = (p.policy == 0 || p.keep[ray]) ? 1.0f : 0.0f;
      if (p.has_eas) d = inv_depth(p.depth[ray]);
    }
    sY[0][i] = y0, sY[1][i] = y1, sY[2][i] = y2, sD[i] = d, sK[i] = k;
  }
  __syncthreads();

  const int ly = tid >> 4, lx = tid & 15;
  const int py = tp.y0 + ly, px = tp.x0 + lx;
  const bool act = py < ph && px < pw;
  const int ctr = (ly + 1) * kLd + lx + 1;
  const long ray = tp.base + (act ? (long)py * pw + px : 0);
  const float keep = act ? sK[ctr] : 0.0f;

  float y[3], mu_y[3], gyy[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    y[c] = sY[c][ctr];
    mu_y[c] = gauss9(sY[c], ctr, kLd);
    gyy[c] = gauss9_prod(sY[c], sY[c], ctr);
  }

  // ---- e_v, the minimum over the views (loss.py:152-153); the statistics of v* stay in registers for the coefficients
  float e_min = 0.0f;
  int v_star = 0;
  float b_x[3], b_mu[3], b_gxx[3], b_gxy[3];
  for (int v = 0; v < nv; ++v) {
    __syncthreads();      // the previous view's readers are done with sX
    for (int i = tid; i < kHalo; i += 256) {
      const int hy = i / kLd, hx = i - hy * kLd;
      const int qy = tp.y0 + hy - 1, qx = tp.x0 + hx - 1;
      float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
      if (qy >= 0 && qy < ph && qx >= 0 && qx < pw) {
        const float* src = p.rgb + ((tp.base + (long)qy * pw + qx) * nv + v) * 3;
        x0 = src[0], x1 = src[1], x2 = src[2];
      }
      sX[0][i] = x0, sX[1][i] = x1, sX[2][i] = x2;
    }
    __syncthreads();
    float ss = 0.0f, l1 = 0.0f;
    float x[3], mu[3], gxx[3], gxy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[c] = sX[c][ctr];
      mu[c] = gauss9(sX[c], ctr, kLd);
      gxx[c] = gauss9_prod(sX[c], sX[c], ctr);
      gxy[c] = gauss9_prod(sX[c], sY[c], ctr);
      ss += ssim_term(mu[c], gxx[c], gxy[c], mu_y[c], gyy[c]);
      l1 += fabsf(x[c] - y[c]);
    }
    const float e = 0.85f * (ss / 3.0f) + 0.15f * (l1 / 3.0f);
    if (v == 0 || e < e_min) {
      e_min = e, v_star = v;
#pragma unroll
      for (int c = 0; c < 3; ++c) b_x[c] = x[c], b_mu[c] = mu[c], b_gxx[c] = gxx[c], b_gxy[c] = gxy[c];
    }
  }
  float up = keep * p.s_rgb;             // d loss / d e_{v*}(this pixel)
  if constexpr (kMed) {
    // a UNIT upstream gradient: the normaliser s_rgb / count is pass 3's, once the count is known
    float f = 1.0f;
    if (p.thresh) {
      const float t = act ? p.thresh[ray] : 0.0f;
      f = min_grad_factor(e_min, t);
      e_min = fminf(e_min, t);
    }
    up = keep * f;
    if (act) {
      if (p.g_rgb) p.fthr[ray] = f;
      const float e = e_min * keep;        // >= 0: the order of the bit patterns is the order of the values
      p.e[ray] = e;
      atomicAdd(&med_hist()[__float_as_uint(e) >> 21], 1u);
    }
  } else if constexpr (kThr) {
    const float t = act ? p.thresh[ray] : 0.0f;
    const float f = min_grad_factor(e_min, t);
    up = up * f;
    e_min = fminf(e_min, t);
    if (p.g_rgb && act) p.fthr[ray] = f;
  }
  const float L = e_min * keep;

  // ---- the SSIM backward coefficients of v* (gathered by the neighbours in pass 3)
  if (p.g_rgb && act) {
    const bool live = up != 0.0f;
    p.vstar[ray] = live ? v_star : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const SsimCoef k = live ? ssim_coef(b_mu[c], b_gxx[c], b_gxy[c], mu_y[c], gyy[c], up) : SsimCoef{0.0f, 0.0f, 0.0f};
      p.coef[(long)(c * 3 + 0) * p.B + ray] = k.k_mu;
      p.coef[(long)(c * 3 + 1) * p.B + ray] = k.k_xx;
      p.coef[(long)(c * 3 + 2) * p.B + ray] = k.k_xy;
    }
  }

  // ---- edge-aware smoothness (loss.py:21-40, masked as in :262-266) on the un-normalised inverse depth
  float eas = 0.0f, d = 0.0f;
  if (p.has_eas && act) {
    d = sD[ctr];
    const bool has_r = px + 1 < pw, has_b = py + 1 < ph;
    float idx = 0.0f, idy = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      idx += fabsf(y[c] - sY[c][ctr + 1]);
      idy += fabsf(y[c] - sY[c][ctr + kLd]);
    }
    const float wx = has_r ? expf(-(idx / 3.0f)) : 0.0f, wy = has_b ? expf(-(idy / 3.0f)) : 0.0f;
    const float ex = d - sD[ctr + 1], ey = d - sD[ctr + kLd];
    eas = edge_term(ex, ey, wx, wy, keep);
    if (p.g_depth) {
      // u_p: this pixel's own edges and the edges its left / upper neighbour owns (those, like the weights above, are also
      // pixel_edges_kernel's; written out in both: behind a function the neighbours' loads come in another order)
      float u = edge_u_own(ex, ey, wx, wy, keep);
      if (px > 0) {
        float il = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) il += fabsf(sY[c][ctr - 1] - y[c]);
        u -= sign0(sD[ctr - 1] - d) * expf(-(il / 3.0f)) * sK[ctr - 1];
      }
      if (py > 0) {
        float iu = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) iu += fabsf(sY[c][ctr - kLd] - y[c]);
        u -= sign0(sD[ctr - kLd] - d) * expf(-(iu / 3.0f)) * sK[ctr - kLd];
      }
      p.u[ray] = u;
    }
  }

  // ---- the tile's partial sums: butterfly per wave, then the four waves in order
  const float r0 = wave_sum(L), r1 = wave_sum(eas), r2 = wave_sum(d), r3 = wave_sum((act && keep == 0.0f) ? 1.0f : 0.0f);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) sRed[wave][0] = r0, sRed[wave][1] = r1, sRed[wave][2] = r2, sRed[wave][3] = r3;
  __syncthreads();
  if (tid == 0) {
    float4 o;
    o.x = ((sRed[0][0] + sRed[1][0]) + sRed[2][0]) + sRed[3][0];
    o.y = ((sRed[0][1] + sRed[1][1]) + sRed[2][1]) + sRed[3][1];
    o.z = ((sRed[0][2] + sRed[1][2]) + sRed[2][2]) + sRed[3][2];
    o.w = ((sRed[0][3] + sRed[1][3]) + sRed[2][3]) + sRed[3][3];
    p.tile_parts[blk] = o;
  }
  if constexpr (kMed) {      // the tile's non-zero bins into its sample's first histogram (the barrier above is behind the atomics);
                             // written out: as bts_loss_device.h's flush_hist, forced inline or not, 25 lines of this kernel's tail move
    unsigned* dst = p.hist + (size_t)(tp.patch / p.pps) * kSelHistSample;
    for (int i = tid; i < kSelBins; i += 256) {
      const unsigned c = med_hist()[i];
      if (c) atomicAdd(&dst[i], c);
    }
  }
  }
}

// one wave per patch (the reduction is also pixel_patch_kernel's, bts_loss_pixel.hip: written out in both, see there)
__global__ __launch_bounds__(64) void loss_tiled_pass2(const TiledParams p) {
  const int lane = threadIdx.x;
  for (long patch = blockIdx.x; patch < p.n_patches; patch += gridDim.x) {
  const float4* tp = p.tile_parts + patch * p.tiles;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (int t = lane; t < p.tiles; t += 64) {
    const float4 q = tp[t];
    a0 += q.x, a1 += q.y, a2 += q.z, a3 += q.w;
  }
  a0 = wave_sum(a0), a1 = wave_sum(a1), a2 = wave_sum(a2), a3 = wave_sum(a3);
  if (lane == 0) {
    const float area = (float)((long)p.ph * p.pw);
    const float m = a2 / area;
    p.parts[patch * 4L + 0] = a0;
    p.parts[patch * 4L + 1] = p.has_eas ? a1 / m : 0.0f;
    p.parts[patch * 4L + 2] = a3;
    p.parts[patch * 4L + 3] = 0.0f;
    p.patch_stats[patch] = make_float4(m, a1, 0.0f, 0.0f);
  }
  }
}

template <class P>
__global__ __launch_bounds__(256) void loss_tiled_pass3(const P p, const long n_tiles) {
  constexpr bool kThr = std::is_same<P, TiledParamsThr>::value;
  constexpr bool kMed = std::is_same<P, TiledParamsMed>::value;
  __shared__ float sC[9][kHalo];
  __shared__ int sV[kHalo];
  const int tid = threadIdx.x;
  for (long blk = blockIdx.x; blk < n_tiles; blk += gridDim.x) {
  if (blk != blockIdx.x) __syncthreads();      // the previous tile's readers are done with the planes
  const TilePos tp = tile_pos(p, blk);
  const int ph = p.ph, pw = p.pw, nv = p.nv;
  float thr_s = 0.0f, fin = 0.0f;              // median: the sample's threshold, s_rgb / count
  if constexpr (kMed) {
    if (p.g_rgb) thr_s = p.thr[tp.patch / p.pps], fin = p.fin[0];
  }
  if (p.g_rgb) {
    for (int i = tid; i < kHalo; i += 256) {
      const int hy = i / kLd, hx = i - hy * kLd;
      const int qy = tp.y0 + hy - 1, qx = tp.x0 + hx - 1;
      int vs = -1;
      float k[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (qy >= 0 && qy < ph && qx >= 0 && qx < pw) {
        const long q = tp.base + (long)qy * pw + qx;
        vs = p.vstar[q];
        if constexpr (kMed) {
          if (p.e[q] > thr_s) vs = -1;        // a dropped pixel hands nothing on (its kept neighbours still hand to it)
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) k[j] = p.coef[(long)j * p.B + q];
      }
      sV[i] = vs;
#pragma unroll
      for (int j = 0; j < 9; ++j) sC[j][i] = k[j];
    }
  }
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  const int py = tp.y0 + ly, px = tp.x0 + lx;
  if (py >= ph || px >= pw) continue;    // (the next barrier is the loop's, which every thread reaches)
  const int ctr = (ly + 1) * kLd + lx + 1;
  const long ray = tp.base + (long)py * pw + px;

  if (p.g_rgb) {
    int vq[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) vq[r * 3 + c] = sV[ctr + (r - 1) * kLd + (c - 1)];
    const float y[3] = {p.rgb_gt[ray * 3], p.rgb_gt[ray * 3 + 1], p.rgb_gt[ray * 3 + 2]};
    float up_c = p.s_rgb;                 // the centre's upstream gradient when it is kept
    if constexpr (kMed)
      up_c = p.fthr[ray];                 // (unit upstream gradient in pass 1: `fin` scales the sum below)
    else if constexpr (kThr)
      up_c = up_c * p.fthr[ray];
    for (int v = 0; v < nv; ++v) {
      unsigned m = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) m |= (vq[j] == v) ? (1u << j) : 0u;
      const float* src = p.rgb + (ray * nv + v) * 3;
      float* dst = p.g_rgb + (ray * nv + v) * 3;
      if (m == 0) {                       // no neighbour chose this view
        dst[0] = 0.0f, dst[1] = 0.0f, dst[2] = 0.0f;
        continue;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = src[c];
        const float t_mu = gauss9_masked(sC[c * 3 + 0], ctr, m), t_xx = gauss9_masked(sC[c * 3 + 1], ctr, m),
                    t_xy = gauss9_masked(sC[c * 3 + 2], ctr, m);
        // the L1 term's gradient: a centre with v* >= 0 is kept, so its upstream gradient is s_rgb
        const float g_l1 = (m & 16u) ? up_c * (0.15f / 3.0f) * sign0(x - y[c]) : 0.0f;
        const float g = t_mu + 2.0f * x * t_xx + y[c] * t_xy + g_l1;
        if constexpr (kMed)
          dst[c] = g * fin;
        else
          dst[c] = g;
      }
    }
  }
  if (p.g_depth) {
    float g = 0.0f;
    if (p.has_eas) {
      const float u = p.u[ray];
      const float4 st = p.patch_stats[tp.patch];      // m, S = sum_p u_p d_p = the un-normalised edge sum
      const float dep = p.depth[ray];
      g = depth_grad(u, st.x, st.y, (long)ph * pw, dep, p.s_eas);
    }
    p.g_depth[ray] = g;
  }
  }
}

// ---- median thresholding: the ray-wise kernels over the one-channel plane e (B).  The selection is bts_loss_pixel.hip's, three channels
// per ray there and one here: both call bts_loss_device.h (ray_pos, select_hist_pass, select_threshold).  The flush stays written out:
// this kernel addresses the bins from the sample's base (a 64-bit vector address), flush_hist on `hist_s + PASS * kSelBins` from a scalar
// one (35 lines fewer), and flush_hist with the index handed over moves the loop's tail (26 lines)
template <int PASS>
__global__ __launch_bounds__(256) void loss_med_hist(const TiledParamsMed p) {
  __shared__ unsigned s_scan[256];
  __shared__ unsigned s_sel[2];
  unsigned* s_hist = med_hist();
  const RayPos r = ray_pos(p);
  unsigned* hist_s = select_hist_pass<PASS, 1>(p, r, s_hist, s_scan, s_sel);
  for (int i = threadIdx.x; i < kSelBins; i += 256) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(&hist_s[PASS * kSelBins + i], c);
  }
}

// thr[sample]; the kept set e <= thr of this work-group's rays: its sum (butterfly per wave, then the four waves in order) and its size.
// The note-down and the sums stay written out here and in pixel_kept_kernel (see there): thread 0 adds the four waves here, block_sum
// hands every thread the sum there
__global__ __launch_bounds__(256) void loss_med_kept(const TiledParamsMed p) {
  __shared__ unsigned s_scan[256];
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
    const float e = p.e[r.ray];
    if (e <= thr) sum = e, cnt = 1u;
  }
  sum = wave_sum(sum), cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = sum, s_u[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    p.blk_sum[blockIdx.x] = ((s_f[0] + s_f[1]) + s_f[2]) + s_f[3];
    p.blk_cnt[blockIdx.x] = ((s_u[0] + s_u[1]) + s_u[2]) + s_u[3];
  }
}

// one work-group: thread t takes partials t, t + 256, ... in order, then the waves' butterflies, then the four waves in order.  The
// smoothness term: pass 2's per-patch terms added in fp64 and rounded once (the fp32 number nearest to their sum); the invalid rays:
// pass 2's per-patch counts (whole numbers below 2^24) added as integers.  Written out here and in pixel_final_kernel: this one reads the
// smoothness term and the invalid count from parts, that one from patch_stats / blk_inv
__global__ __launch_bounds__(256) void loss_med_final(const TiledParamsMed p) {
  __shared__ float s_f[4];
  __shared__ double s_d[4];
  __shared__ unsigned long long s_c[2][4];
  float sum = 0.0f;
  double eas = 0.0;
  unsigned long long cnt = 0ull, inv = 0ull;
  for (long i = threadIdx.x; i < p.n_blocks; i += 256) sum += p.blk_sum[i], cnt += p.blk_cnt[i];
  for (long i = threadIdx.x; i < p.n_patches; i += 256) eas += p.parts[i * 4 + 1], inv += (unsigned long long)p.parts[i * 4 + 2];
  sum = wave_sum(sum);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64), inv += __shfl_xor(inv, off, 64), eas += __shfl_xor(eas, off, 64);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    s_f[w] = sum, s_c[0][w] = cnt, s_c[1][w] = inv, s_d[w] = eas;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long count = s_c[0][0] + s_c[0][1] + s_c[0][2] + s_c[0][3];
    const unsigned long long bad = s_c[1][0] + s_c[1][1] + s_c[1][2] + s_c[1][3];
    p.out[0] = (((s_f[0] + s_f[1]) + s_f[2]) + s_f[3]) / (float)count;
    p.out[1] = (float)(((s_d[0] + s_d[1]) + s_d[2]) + s_d[3]);
    p.out[2] = (float)bad;
    p.out[3] = (float)count;
    if (p.kept) p.kept[0] = (long long)count;
    p.fin[0] = p.s_rgb / (float)count;
  }
}

inline long tiles_of(int ph, int pw) { return (long)((ph + kTile - 1) / kTile) * ((pw + kTile - 1) / kTile); }

// THE layout of bts_photometric_loss_tiled's workspace: tile partials, patch statistics, v*, nine coefficient planes, u, keep flags and,
// with the automasking bound, its gradient factors
inline void tiled_layout(Carver& w, TiledParamsThr& p, size_t n_patches, size_t n_tiles, size_t B, bool with_thresh) {
  p.tile_parts = w.take<float4>(n_tiles);
  p.patch_stats = w.take<float4>(n_patches);
  p.vstar = w.take<int>(B);
  p.coef = w.take<float>(B * 9);
  p.u = w.take<float>(B);
  p.keep = w.take<unsigned char>(B);
  p.fthr = with_thresh ? w.take<float>(B) : nullptr;
}

// THE layout of bts_photometric_loss_median's workspace: the tiled layout with the gradient factors, then e, the histograms, the
// selection state, the thresholds, two partials per work-group of 256 rays, the final words
inline void median_layout(Carver& w, TiledParamsMed& p, size_t n_patches, size_t n_tiles, size_t B, size_t n, size_t n_blocks) {
  tiled_layout(w, p, n_patches, n_tiles, B, true);
  p.e = w.take<float>(B);
  p.hist = w.take<unsigned>(n * kSelHistSample);
  p.state = w.take<unsigned>(n * kSelStateSample);
  p.thr = w.take<float>(n);
  p.blk_sum = w.take<float>(n_blocks);
  p.blk_cnt = w.take<unsigned>(n_blocks);
  p.fin = w.take<float>(4);
}
inline size_t median_blocks_per_sample(size_t n_patches, size_t n, int ph, int pw) { return (n_patches / n * (size_t)ph * (size_t)pw + 255) / 256; }

}  // namespace

size_t loss_median_bytes(int n_patches, int ph, int pw, int nv, int n) {
  if (n_patches <= 0 || ph <= 0 || pw <= 0 || nv <= 0 || n <= 0 || n_patches % n != 0) return 0;
  Carver count(nullptr);
  TiledParamsMed p;
  median_layout(count, p, (size_t)n_patches, (size_t)n_patches * (size_t)tiles_of(ph, pw), (size_t)n_patches * (size_t)ph * (size_t)pw, (size_t)n,
                (size_t)n * median_blocks_per_sample((size_t)n_patches, (size_t)n, ph, pw));
  return count.bytes();
}

int photometric_loss_median_impl(const BtsLossArgs* a, int n, const float* thresh, float* out, float* thresholds, int64_t* kept, void* workspace,
                                 hipStream_t s) {
  TiledParamsMed p;
  p.rgb = a->rgb, p.depth = a->depth, p.weights = a->weights, p.invalid = a->invalid, p.rgb_gt = a->rgb_gt;
  p.invalid_wsum = a->invalid_wsum, p.invalid_any = a->invalid_any;
  p.parts = a->parts, p.g_rgb = a->g_rgb, p.g_depth = a->g_depth;
  p.n_patches = a->n_patches, p.ph = a->patch_h, p.pw = a->patch_w, p.nv = a->nv, p.K = a->K, p.policy = a->invalid_policy;
  p.s_rgb = a->scale_rgb, p.s_eas = a->scale_eas, p.has_eas = a->edge_aware_smoothness;
  p.tiles_x = (p.pw + kTile - 1) / kTile;
  p.tiles = (int)tiles_of(p.ph, p.pw);
  p.B = (long)p.n_patches * p.ph * p.pw;
  p.thresh = thresh;
  p.out = out, p.thresholds = thresholds, p.kept = (long long*)kept;
  p.n = n, p.pps = p.n_patches / n, p.Bs = p.B / n;
  p.blocks_per_sample = (int)median_blocks_per_sample((size_t)p.n_patches, (size_t)n, p.ph, p.pw);
  p.n_blocks = (long)n * p.blocks_per_sample;
  const size_t nt = (size_t)p.n_patches * (size_t)p.tiles;
  Carver carve(workspace);
  median_layout(carve, p, (size_t)p.n_patches, nt, (size_t)p.B, (size_t)n, (size_t)p.n_blocks);
  const TiledParams& base = p;
  p.vec4 = p.nv == 1 && p.K > 0 && (p.K & 3) == 0 && ((uintptr_t)p.invalid & 15) == 0 && ((uintptr_t)p.weights & 15) == 0;
  const unsigned grid = (unsigned)((long)nt < kMaxGrid ? (long)nt : kMaxGrid);
  const unsigned grid2 = (unsigned)(p.n_patches < kMaxGrid ? (long)p.n_patches : kMaxGrid);
  const unsigned gridr = (unsigned)p.n_blocks;
  if (hipMemsetAsync(p.hist, 0, (size_t)n * kSelHistSample * sizeof(unsigned), s) != hipSuccess) {
    set_error("%s: clearing the histograms failed", "bts_photometric_loss_median");
    return BTS_E_LAUNCH;
  }
  if (p.policy != 0) {
    const long kb = (p.B + 255) / 256;
    loss_tiled_keep<<<(unsigned)(kb < kMaxGrid ? kb : kMaxGrid), 256, 0, s>>>(base);
  }
  loss_tiled_pass1<TiledParamsMed><<<grid, 256, 0, s>>>(p, (long)nt);
  loss_med_hist<1><<<gridr, 256, 0, s>>>(p);
  loss_med_hist<2><<<gridr, 256, 0, s>>>(p);
  loss_med_kept<<<gridr, 256, 0, s>>>(p);
  loss_tiled_pass2<<<grid2, 64, 0, s>>>(base);
  loss_med_final<<<1, 256, 0, s>>>(p);
  if (p.g_rgb || p.g_depth) loss_tiled_pass3<TiledParamsMed><<<grid, 256, 0, s>>>(p, (long)nt);
  return launch_check("%s: median loss kernel launch failed (%ld)");
}

size_t loss_tiled_bytes(int n_patches, int ph, int pw, int nv, bool with_thresh) {
  if (n_patches < 0 || ph <= 0 || pw <= 0 || nv <= 0) return 0;
  Carver count(nullptr);
  TiledParamsThr p;
  tiled_layout(count, p, (size_t)n_patches, (size_t)n_patches * (size_t)tiles_of(ph, pw), (size_t)n_patches * (size_t)ph * (size_t)pw, with_thresh);
  return count.bytes();
}

int photometric_loss_tiled_impl(const BtsLossArgs* a, void* workspace, hipStream_t s, const float* thresh) {
  if (a->n_patches == 0) return BTS_OK;
  TiledParamsThr p;
  p.rgb = a->rgb, p.depth = a->depth, p.weights = a->weights, p.invalid = a->invalid, p.rgb_gt = a->rgb_gt;
  p.invalid_wsum = a->invalid_wsum, p.invalid_any = a->invalid_any;
  p.parts = a->parts, p.g_rgb = a->g_rgb, p.g_depth = a->g_depth;
  p.n_patches = a->n_patches, p.ph = a->patch_h, p.pw = a->patch_w, p.nv = a->nv, p.K = a->K, p.policy = a->invalid_policy;
  p.s_rgb = a->scale_rgb, p.s_eas = a->scale_eas, p.has_eas = a->edge_aware_smoothness;
  p.tiles_x = (p.pw + kTile - 1) / kTile;
  p.tiles = (int)tiles_of(p.ph, p.pw);
  p.B = (long)p.n_patches * p.ph * p.pw;
  const size_t nt = (size_t)p.n_patches * (size_t)p.tiles;
  Carver carve(workspace);
  tiled_layout(carve, p, (size_t)p.n_patches, nt, (size_t)p.B, thresh != nullptr);
  p.thresh = thresh;
  const TiledParams& base = p;
  p.vec4 = p.nv == 1 && p.K > 0 && (p.K & 3) == 0 && ((uintptr_t)p.invalid & 15) == 0 && ((uintptr_t)p.weights & 15) == 0;
  const unsigned grid = (unsigned)((long)nt < kMaxGrid ? (long)nt : kMaxGrid);
  const unsigned grid2 = (unsigned)(p.n_patches < kMaxGrid ? (long)p.n_patches : kMaxGrid);
  if (p.policy != 0) {
    const long kb = (p.B + 255) / 256;
    loss_tiled_keep<<<(unsigned)(kb < kMaxGrid ? kb : kMaxGrid), 256, 0, s>>>(base);
  }
  if (thresh)
    loss_tiled_pass1<TiledParamsThr><<<grid, 256, 0, s>>>(p, (long)nt);
  else
    loss_tiled_pass1<TiledParams><<<grid, 256, 0, s>>>(base, (long)nt);
  loss_tiled_pass2<<<grid2, 64, 0, s>>>(base);
  if (p.g_rgb || p.g_depth) {
    if (thresh)
      loss_tiled_pass3<TiledParamsThr><<<grid, 256, 0, s>>>(p, (long)nt);
    else
      loss_tiled_pass3<TiledParams><<<grid, 256, 0, s>>>(base, (long)nt);
  }
  return launch_check("%s: tiled loss kernel launch failed (%ld)");
}

}  // namespace bts
