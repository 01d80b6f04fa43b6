// The image half of BTSWrapper.compute_nvs_metrics (models/bts/evaluator_nvs.py:141-178): PSNR and SSIM of the rendered target view
// against its ground truth over the 5 % crop at eval_resolution.  One row of eight doubles per frame stays on the device; nothing
// synchronises.  LPIPS (:171) stays with the caller.
//
// Two launches (blockIdx.y = frame):
//   nvs_tiles_kernel   one work-group per kTileY x kTileX tile of the INTERIOR (the crop pixels whose 7 x 7 window lies inside the
//                      crop).  Per channel: the (kTileY + 6) x (kTileX + 6) halo of both images is gathered once into LDS as fp64,
//                      through the nearest map and the element strides -- no resized or cropped image ever exists in memory; the
//                      seven-term row sums of x, y, x^2, y^2, xy go to LDS; each lane adds seven of those per output pixel, forms S
//                      and keeps its sum.  A crop pixel's squared error is counted by the one tile that owns it (the first kTileY
//                      rows / kTileX columns of a halo; the last tile of a row or column owns the rest).  Four fp64 partials per
//                      work-group (ssim of the three channels, squared error), lanes, then waves, in a fixed order.
//   nvs_finish_kernel  one wave per frame adds the partials in slot order and writes the row.
// The kernel boundary is the hand-over: no float atomics, no "last block" flag, so a rerun is bit-identical.
//
// All arithmetic is fp64 from the fp32 inputs, as skimage's (before 0.19 `multichannel=True` images were promoted to float64), with
// no contraction.  Quirks of the reference that are reproduced ON PURPOSE:
//   - F.interpolate's nearest source index is min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out in fp32
//     (:154-155), not the exact rational -- bts_common.h's nearest_src, the index bts_depth_metrics.hip documents;
//   - the crop box is the host's: ceil(0.05 * h), floor(0.95 * h) evaluated on Python floats (:158-161);
//   - cov_norm = 49 / 48: the sample covariance of skimage's default use_sample_covariance=True;
//   - the mean of S runs over the interior only (skimage crops (win_size - 1) // 2 = 3 pixels from every side), so the filter's
//     reflect border never reaches the result and no border mode exists here.
// Outside the contract: NaN or inf in either image (nothing faults, the row is unspecified).
#include "bts_host.h"
#include "bts_eval_device.h"

namespace bts {

constexpr int kNvsThreads = 256;
constexpr int kWin = 7;
constexpr int kTileY = 16, kTileX = 32;                            // interior pixels per work-group
constexpr int kHaloY = kTileY + kWin - 1, kHaloX = kTileX + kWin - 1;
constexpr int kHaloXP = kHaloX + 1;                                // 39 doubles per row: an odd pitch
constexpr int kRowXP = kTileX + 1;
constexpr int kNvsSlot = 4;                                        // doubles per work-group: ssim_c0, ssim_c1, ssim_c2, squared error

struct NvsGeom {
  const float* pred;
  const float* gt;
  long long pred_sb, pred_sy, pred_sx, pred_sc, gt_sb, gt_sy, gt_sx, gt_sc;
  int H, W, y0, x0, h, w;     // source size; the crop's origin at eval_resolution and its size
  int hi, wi, ntx, nblk;      // the interior's size, tiles per row, tiles per frame
  float sh, sw;
  double c1, c2, r2;
  double* part;               // (B, nblk, 4)
};

__global__ __launch_bounds__(kNvsThreads) void nvs_tiles_kernel(NvsGeom g) {
  __shared__ double s_x[kHaloY][kHaloXP], s_y[kHaloY][kHaloXP];
  __shared__ double s_row[5][kHaloY][kRowXP];
  __shared__ double s_part[kNvsThreads / 64][kNvsSlot];
  const int f = blockIdx.y, ty = blockIdx.x / g.ntx, tx = blockIdx.x - ty * g.ntx, t = threadIdx.x;
  const int cy0 = ty * kTileY, cx0 = tx * kTileX;                  // the halo's origin in crop coordinates = the tile's in interior ones
  // the halo rows / columns whose squared error this tile counts
  const int own_y = (cy0 + kTileY >= g.hi) ? kHaloY : kTileY, own_x = (cx0 + kTileX >= g.wi) ? kHaloX : kTileX;
  const float* pred_f = g.pred + (long long)f * g.pred_sb;
  const float* gt_f = g.gt + (long long)f * g.gt_sb;
  const double cov_norm = 49.0 / 48.0;
  double acc[kNvsSlot] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < 3; ++c) {
    // the halo through the nearest map; 0 outside the crop (such entries feed no interior pixel of the crop)
    for (int i = t; i < kHaloY * kHaloX; i += kNvsThreads) {
      const int r = i / kHaloX, q = i - r * kHaloX;
      const int cy = cy0 + r, cx = cx0 + q;
      double x = 0.0, y = 0.0;
      if (cy < g.h && cx < g.w) {
        const long long sy = nearest_src(g.y0 + cy, g.sh, g.H), sx = nearest_src(g.x0 + cx, g.sw, g.W);
        x = (double)pred_f[sy * g.pred_sy + sx * g.pred_sx + c * g.pred_sc];
        y = (double)gt_f[sy * g.gt_sy + sx * g.gt_sx + c * g.gt_sc];
        if (r < own_y && q < own_x) {
          const double d = x - y;
          acc[3] += d * d;
        }
      }
      s_x[r][q] = x, s_y[r][q] = y;
    }
    __syncthreads();
    // seven-term row sums of the five products, left to right
    for (int i = t; i < kHaloY * kTileX; i += kNvsThreads) {
      const int r = i / kTileX, q = i - r * kTileX;
      double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const double x = s_x[r][q + k], y = s_y[r][q + k];
        a[0] += x, a[1] += y, a[2] += x * x, a[3] += y * y, a[4] += x * y;
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) s_row[m][r][q] = a[m];
    }
    __syncthreads();
    // seven rows per output pixel, top to bottom, then S
    for (int i = t; i < kTileY * kTileX; i += kNvsThreads) {
      const int r = i / kTileX, q = i - r * kTileX;
      if (cy0 + r < g.hi && cx0 + q < g.wi) {
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
#pragma unroll
          for (int m = 0; m < 5; ++m) a[m] += s_row[m][r + k][q];
        }
        const double ux = a[0] / 49.0, uy = a[1] / 49.0, uxx = a[2] / 49.0, uyy = a[3] / 49.0, uxy = a[4] / 49.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double a1 = 2.0 * ux * uy + g.c1, a2 = 2.0 * vxy + g.c2, b1 = ux * ux + uy * uy + g.c1, b2 = vx + vy + g.c2;
        acc[c] += (a1 * a2) / (b1 * b2);
      }
    }
    __syncthreads();     // the next channel overwrites the halo and the row sums
  }
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < kNvsSlot; ++k) acc[k] = lane0_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kNvsSlot; ++k) s_part[wave][k] = acc[k];
  }
  __syncthreads();
  if (t < kNvsSlot) {
    double a = s_part[0][t];
    for (int w = 1; w < kNvsThreads / 64; ++w) a += s_part[w][t];
    g.part[((size_t)f * g.nblk + blockIdx.x) * kNvsSlot + t] = a;
  }
}

// row: ssim psnr mse ssim_c0 ssim_c1 ssim_c2 n_interior n_crop
__global__ __launch_bounds__(64) void nvs_finish_kernel(NvsGeom g, double* __restrict__ metrics) {
  __shared__ double s_s[kNvsSlot];
  const int f = blockIdx.x, lane = threadIdx.x;
  const double* part_f = g.part + (size_t)f * g.nblk * kNvsSlot;
  if (lane < kNvsSlot) {
    double a = 0.0;
    for (int b = 0; b < g.nblk; ++b) a += part_f[(size_t)b * kNvsSlot + lane];
    s_s[lane] = a;
  }
  __syncthreads();
  if (lane == 0) {
    const double n_int = (double)g.hi * (double)g.wi, n_crop = (double)g.h * (double)g.w;
    const double c0 = s_s[0] / n_int, c1 = s_s[1] / n_int, c2 = s_s[2] / n_int;
    const double mse = s_s[3] / (3.0 * n_crop);
    double* row = metrics + (size_t)f * 8;
    row[0] = (c0 + c1 + c2) / 3.0;
    row[1] = mse == 0.0 ? __longlong_as_double(0x7FF0000000000000LL) : 10.0 * log10(g.r2 / mse);   // :170
    row[2] = mse;
    row[3] = c0, row[4] = c1, row[5] = c2;
    row[6] = n_int, row[7] = n_crop;
  }
}

static int nvs_tiles(int n, int tile) { return n > kWin - 1 ? (n - (kWin - 1) + tile - 1) / tile : 1; }

// THE layout of bts_nvs_metrics' workspace: the partials of the largest crop eval_resolution admits
static void nvs_layout(Carver& w, NvsGeom& g, size_t B, int He, int We) {
  g.part = w.take<double>(B * nvs_tiles(He, kTileY) * nvs_tiles(We, kTileX) * kNvsSlot);
}

size_t nvs_metrics_bytes(int B, int He, int We) {
  Carver count(nullptr);
  NvsGeom g;
  nvs_layout(count, g, (size_t)B, He, We);
  return count.bytes();
}

int nvs_metrics_launch(const BtsNvsMetrics* a, void* workspace, hipStream_t s) {
  NvsGeom g;
  g.pred = a->pred, g.gt = a->gt;
  g.pred_sb = a->pred_sb, g.pred_sy = a->pred_sy, g.pred_sx = a->pred_sx, g.pred_sc = a->pred_sc;
  g.gt_sb = a->gt_sb, g.gt_sy = a->gt_sy, g.gt_sx = a->gt_sx, g.gt_sc = a->gt_sc;
  g.H = a->H, g.W = a->W, g.y0 = a->y0, g.x0 = a->x0, g.h = a->y1 - a->y0, g.w = a->x1 - a->x0;
  g.hi = g.h - (kWin - 1), g.wi = g.w - (kWin - 1);
  g.ntx = nvs_tiles(g.w, kTileX), g.nblk = g.ntx * nvs_tiles(g.h, kTileY);
  g.sh = (float)a->H / (float)a->He, g.sw = (float)a->W / (float)a->We;
  g.c1 = (0.01 * a->data_range) * (0.01 * a->data_range), g.c2 = (0.03 * a->data_range) * (0.03 * a->data_range);
  g.r2 = a->data_range * a->data_range;
  Carver carve(workspace);
  nvs_layout(carve, g, (size_t)a->B, a->He, a->We);
  nvs_tiles_kernel<<<dim3(g.nblk, a->B), kNvsThreads, 0, s>>>(g);
  if (int rc = launch_code()) return rc;
  nvs_finish_kernel<<<a->B, 64, 0, s>>>(g, a->metrics);
  return launch_code();
}

}  // namespace bts
