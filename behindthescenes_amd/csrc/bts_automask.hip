// bts_automask.hip -- the error map of use_automasking (trainer.py:201-206): for every frame f of a batch element the mean, over the L
// loss frames j, of compute_errors_l1ssim(.5 frame f, .5 frame ids_loss[j]) on WHOLE frames, and the reference's torch.cat of that map
// as a fourth plane behind the frame's three colour planes.  The reference spends about twenty torch ops on (n v L, 3, H + 2, W + 2)
// tensors on it; here one launch reads every input plane and writes every output plane once.
//   err[n, f, p] = (1 / L) sum_j ( .85 mean_c ssim(x_f, y_j)[c, p] + .15 mean_c |x_f - y_j|[c, p] ),  x = scale * frame
// with the SSIM of bts_loss.hip (bts_loss_device.h: the 3 x 3 Gaussian window and ssim_term = clamp(1 - n / d, 0, 1) / 2 with c1 = 1e-4,
// c2 = 9e-4; ZERO padding at the frame border), plain fp32; the windowed sums are this file's own: they weigh one operand first and
// accumulate with fused multiply-adds (weigh9 / dot9).
// One work-group of 256 threads per (batch element, 8 x 32 tile), thread = pixel (a wave takes two rows of 32 consecutive floats: whole
// 128-byte lines).  The L partner tiles are staged once, scaled, with their one-pixel halo in LDS; every thread forms mu_y and G * y^2 of
// its pixel for the L x 3 (partner, channel) pairs once and keeps them in registers.  Then the work-group walks the v frames of its
// element: stages the frame's tile (raw: the copy into images4 is bit-exact), forms mu_x and G * x^2 per channel once for all partners,
// G * xy per partner.  LDS: (3 L + 3) planes of 340 floats = 36 720 bytes at L = 8.  No atomics, no cross-group hand-over: reruns are
// bit-identical.
#include <hip/hip_runtime.h>

#include "bts_host.h"
#include "bts_loss_device.h"

namespace bts {

namespace {

constexpr int kTileH = 8, kTileW = 32;          // interior pixels of a tile (256 threads, thread = pixel)
constexpr int kLd = kTileW + 2;                 // row length of a plane with its one-pixel halo
constexpr int kHalo = (kTileH + 2) * kLd;       // 340
constexpr int kStage = (kHalo + 255) / 256;     // halo texels a thread stages per plane

struct AutomaskParams {
  const float* images;   // (n, v, 3, H, W)
  float* errors;         // (n, v, H, W) or null
  float* images4;        // (n, v, 4, H, W) or null
  int n, v, H, W, L;
  int tiles_x, tiles;    // tiles per row of tiles, tiles per frame
  float scale;
  int ids[BTS_MAX_VIEWS];
};

// the 3 x 3 neighbourhood of `ctr` in a zero-bordered plane, row-major, times `scale`
__device__ __forceinline__ void load9(const float* pl, int ctr, float scale, float* q) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[r * 3 + c] = scale * pl[ctr + (r - 1) * kLd + (c - 1)];
}
// The window (bts_loss_device.h: kGa, kGb, kGc) applied once: qw[k] = G[k] * q[k].  Every windowed sum of this kernel is then a row-major sum of qw (the mean) or a chain of
// nine fused multiply-adds of qw with a second neighbourhood (G * q^2, G * qp): a third of the instructions of weighting every product
// on its own, and one rounding per term instead of two
__device__ __forceinline__ void weigh9(const float* q, float* qw) {
  qw[0] = kGa * q[0], qw[1] = kGb * q[1], qw[2] = kGa * q[2];
  qw[3] = kGb * q[3], qw[4] = kGc * q[4], qw[5] = kGb * q[5];
  qw[6] = kGa * q[6], qw[7] = kGb * q[7], qw[8] = kGa * q[8];
}
__device__ __forceinline__ float sum9(const float* qw) {
  float s = qw[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) s += qw[k];
  return s;
}
__device__ __forceinline__ float dot9(const float* qw, const float* p) {
  float s = qw[0] * p[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) s = fmaf(qw[k], p[k], s);
  return s;
}

template <int LMAX>
__global__ __launch_bounds__(256) void automask_kernel(const AutomaskParams p) {
  __shared__ float sY[LMAX][3][kHalo];
  __shared__ float sX[3][kHalo];
  const int tid = threadIdx.x;
  const int H = p.H, W = p.W, L = p.L, v = p.v;
  const long HW = (long)H * W;
  const int s = blockIdx.x / p.tiles;
  const int r = blockIdx.x - s * p.tiles;
  const int ty = r / p.tiles_x;
  const int y0 = ty * kTileH, x0 = (r - ty * p.tiles_x) * kTileW;
  const float* frames = p.images + (long)s * v * 3 * HW;    // this element's frames

  // the halo texels this thread stages for every plane: LDS index and offset inside a plane (-1: outside the frame, the zero padding)
  int s_idx[kStage];
  long s_off[kStage];
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    const int i = tid + k * 256;
    const int hy = i / kLd, hx = i - hy * kLd;
    const int py = y0 + hy - 1, px = x0 + hx - 1;
    s_idx[k] = i < kHalo ? i : -1;
    s_off[k] = (py >= 0 && py < H && px >= 0 && px < W) ? (long)py * W + px : -1;
  }

  // ---- the L partner tiles, scaled
  for (int j = 0; j < L; ++j) {
    const float* src = frames + (long)p.ids[j] * 3 * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < kStage; ++k)
        if (s_idx[k] >= 0) sY[j][c][s_idx[k]] = s_off[k] >= 0 ? p.scale * src[c * HW + s_off[k]] : 0.0f;
  }
  __syncthreads();

  const int ly = tid >> 5, lx = tid & 31;
  const int py = y0 + ly, px = x0 + lx;
  const bool act = py < H && px < W;
  const int ctr = (ly + 1) * kLd + lx + 1;
  const long pix = (long)py * W + px;

  float yc[LMAX][3], mu_y[LMAX][3], gyy[LMAX][3];
#pragma unroll
  for (int j = 0; j < LMAX; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      yc[j][c] = mu_y[j][c] = gyy[j][c] = 0.0f;
      if (j < L) {
        float q[9], qw[9];
        load9(sY[j][c], ctr, 1.0f, q);
        weigh9(q, qw);
        yc[j][c] = q[4], mu_y[j][c] = sum9(qw), gyy[j][c] = dot9(qw, q);
      }
    }

  for (int f = 0; f < v; ++f) {
    if (f) __syncthreads();      // the previous frame's readers are done with sX
    const float* src = frames + (long)f * 3 * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < kStage; ++k)
        if (s_idx[k] >= 0) sX[c][s_idx[k]] = s_off[k] >= 0 ? src[c * HW + s_off[k]] : 0.0f;
    __syncthreads();

    float ss[LMAX], l1[LMAX], raw[3];
#pragma unroll
    for (int j = 0; j < LMAX; ++j) ss[j] = l1[j] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      raw[c] = sX[c][ctr];
      float x[9], xw[9];
      load9(sX[c], ctr, p.scale, x);
      weigh9(x, xw);
      const float mu_x = sum9(xw), gxx = dot9(xw, x);
#pragma unroll
      for (int j = 0; j < LMAX; ++j) {
        if (j < L) {
          float y[9];
          load9(sY[j][c], ctr, 1.0f, y);
          const float gxy = dot9(xw, y);
          ss[j] += ssim_term(mu_x, gxx, gxy, mu_y[j][c], gyy[j][c]);
          l1[j] += fabsf(x[4] - yc[j][c]);
        }
      }
    }
    float err = 0.0f;
#pragma unroll
    for (int j = 0; j < LMAX; ++j)
      if (j < L) err += 0.85f * (ss[j] / 3.0f) + 0.15f * (l1[j] / 3.0f);
    err = err / (float)L;
    if (act) {
      const long fr = (long)s * v + f;
      if (p.errors) p.errors[fr * HW + pix] = err;
      if (p.images4) {
        float* dst = p.images4 + fr * 4 * HW + pix;
        dst[0] = raw[0], dst[HW] = raw[1], dst[2 * HW] = raw[2], dst[3 * HW] = err;
      }
    }
  }
}

}  // namespace

// tiles of bts_automask_errors' grid (one work-group each); the entry point bounds it by 2^31 - 1
long automask_tiles(int n, int H, int W) { return (long)n * ((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW); }

int automask_errors_launch(const float* images, int n, int v, int H, int W, const int* ids_loss, int L, float scale, float* errors,
                           float* images4, hipStream_t s) {
  AutomaskParams p;
  p.images = images, p.errors = errors, p.images4 = images4;
  p.n = n, p.v = v, p.H = H, p.W = W, p.L = L, p.scale = scale;
  p.tiles_x = (W + kTileW - 1) / kTileW;
  p.tiles = ((H + kTileH - 1) / kTileH) * p.tiles_x;
  for (int j = 0; j < BTS_MAX_VIEWS; ++j) p.ids[j] = j < L ? ids_loss[j] : 0;
  const unsigned grid = (unsigned)automask_tiles(n, H, W);
  with_nvmax(L, [&](auto lmax) {
    automask_kernel<decltype(lmax)::value><<<grid, 256, 0, s>>>(p);
    return 0;
  });
  return launch_check("%s: automask kernel launch failed (%ld)");
}

}  // namespace bts
