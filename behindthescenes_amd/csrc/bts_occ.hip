// The ground-truth half of the LiDAR occupancy evaluator (models/bts/evaluator_lidar.py:57-160, 163-168, 296-298, 314-330) as four short
// fp32 kernels: bin the clouds by angle and take a minimum per bin, finish one (362, 2) table per (slice, cloud), look every query
// point up in the tables of its slice, classify the points into six counters.  No matrix pipe, no inline assembly; every reduction is
// an integer / bit-pattern atomic, so reruns are bit-identical.
#include "bts_host.h"
#include "bts_eval_device.h"

namespace bts {

constexpr int kBins = 360;            // evaluator_lidar.py:64
constexpr int kRows = kBins + 2;      // the two wrap rows of :109
constexpr unsigned kInfBits = 0x7F800000u;
constexpr unsigned long long kNoFirst = ~0ull;

struct LidarOffsets {
  int off[BTS_LIDAR_MAX_CLOUDS + 1];
};
struct LidarSliceBounds {
  float lo[BTS_LIDAR_MAX_SLICES], hi[BTS_LIDAR_MAX_SLICES];
};

__global__ __launch_bounds__(256) void lidar_init_kernel(unsigned* __restrict__ bins, unsigned long long* __restrict__ first, int n_bins,
                                                         int n_first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_bins) bins[i] = kInfBits;
  if (i < n_first) first[i] = kNoFirst;
}

// get_lidar_slices (:76-102) up to the per-bin minimum.  blockIdx.y = cloud; a work-group takes `per_block` consecutive points of it.
// bins (y_res, T, 360): bit pattern of the smallest distance of the bin (distances are >= 0, so the uint32 order is the float order),
// +inf where no point fell.  first (y_res, T): (ordered angle bits << 32 | distance bits) of the selected point with the smallest angle
// -- the reference's initial carry slice_points_polar[0, 1] (:93).
__global__ __launch_bounds__(256) void lidar_bins_kernel(const float4* __restrict__ points, LidarOffsets offs, const float* __restrict__ velo_poses,
                                                         const float* __restrict__ borders, LidarSliceBounds yb, int y_res, float max_dist,
                                                         int per_block, int T, unsigned* __restrict__ bins, unsigned long long* __restrict__ first) {
  __shared__ float s_border[kBins + 1];
  __shared__ unsigned s_bins[BTS_LIDAR_MAX_SLICES * kBins];
  __shared__ unsigned long long s_first[BTS_LIDAR_MAX_SLICES];
  const int t = blockIdx.y;
  const int n_pts = offs.off[t + 1] - offs.off[t];
  const int begin = blockIdx.x * per_block;
  if (begin >= n_pts) return;   // (the whole work-group)
  const int end = min(begin + per_block, n_pts);
  for (int i = threadIdx.x; i <= kBins; i += 256) s_border[i] = borders[i];
  for (int i = threadIdx.x; i < y_res * kBins; i += 256) s_bins[i] = kInfBits;
  if (threadIdx.x < y_res) s_first[threadIdx.x] = kNoFirst;
  __syncthreads();

  const float* M = velo_poses + t * 16;
  const float m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7];
  const float m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3];
  const float m20 = M[8], m21 = M[9], m22 = M[10], m23 = M[11];
  const float4* pc = points + offs.off[t];
  for (int i = begin + threadIdx.x; i < end; i += 256) {
    const float4 p = pc[i];
    // pc_world = velo_pose @ pc (:77)
    const float xw = ((m00 * p.x + m01 * p.y) + m02 * p.z) + m03 * p.w;
    const float yw = ((m10 * p.x + m11 * p.y) + m12 * p.z) + m13 * p.w;
    const float zw = ((m20 * p.x + m21 * p.y) + m22 * p.z) + m23 * p.w;
    const bool far = sqrtf((xw * xw + yw * yw) + zw * zw) >= max_dist;   // a far point enters every slice (:79)
    // polar coordinates of the VELODYNE-frame x, y (:81-84)
    const float angle = atan2f(p.y, p.x);
    const float dist = sqrtf(p.x * p.x + p.y * p.y);
    // bin i holds [border_i, border_i+1): what searchsorted(sorted_angles, borders) selects (:96).  cnt = number of borders <= angle
    int lo = 0, hi = kBins + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_border[mid] <= angle) lo = mid + 1;
      else hi = mid;
    }
    const int bin = lo - 1;   // -1: below border_0; 360: at or above border_360 -- in no bin
    const unsigned dbits = __float_as_uint(dist);
    const unsigned long long key = ((unsigned long long)float_key(angle) << 32) | dbits;
    for (int s = 0; s < y_res; ++s) {
      if (far || (yw >= yb.lo[s] && yw <= yb.hi[s])) {
        if (bin >= 0 && bin < kBins) atomicMin(&s_bins[s * kBins + bin], dbits);
        atomicMin(&s_first[s], key);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < y_res * kBins; i += 256) {
    const unsigned v = s_bins[i];
    if (v != kInfBits) atomicMin(&bins[((long)(i / kBins) * T + t) * kBins + (i % kBins)], v);
  }
  if (threadIdx.x < y_res && s_first[threadIdx.x] != kNoFirst) atomicMin(&first[threadIdx.x * T + t], s_first[threadIdx.x]);
}

// :98-109: one wave per (slice, cloud).  An empty bin takes the previous bin's value, the very first carry is the distance of the
// smallest-angle point; rows 1..360 = ((border_i + border_i+1) * .5, dist_i), row 0 = (angle_359 - 2 pi, dist_359), row 361 =
// (angle_0 + 2 pi, dist_0).  No selected point at all: every distance stays +inf.
__global__ __launch_bounds__(64) void lidar_table_kernel(const unsigned* __restrict__ bins, const unsigned long long* __restrict__ first,
                                                         const float* __restrict__ borders, float* __restrict__ tables) {
  __shared__ unsigned s_raw[kBins];
  __shared__ float s_dist[kBins];
  const int tab = blockIdx.x;
  const int lane = threadIdx.x;
  for (int i = lane; i < kBins; i += 64) s_raw[i] = bins[(long)tab * kBins + i];
  __syncthreads();
  const unsigned long long f = first[tab];
  const float carry0 = f == kNoFirst ? __uint_as_float(kInfBits) : __uint_as_float((unsigned)(f & 0xFFFFFFFFu));
  float* out = tables + (long)tab * kRows * 2;
  const float two_pi = 6.283185307179586f;   // math.pi * 2 as the fp32 scalar torch subtracts (:109)
  for (int i = lane; i < kBins; i += 64) {
    int j = i;
    while (j >= 0 && s_raw[j] == kInfBits) --j;   // carry forward: the nearest non-empty bin at or below i
    const float d = j >= 0 ? __uint_as_float(s_raw[j]) : carry0;
    s_dist[i] = d;
    const float a = (borders[i] + borders[i + 1]) * .5f;
    out[(i + 1) * 2 + 0] = a, out[(i + 1) * 2 + 1] = d;
  }
  __syncthreads();
  if (lane == 0) {
    out[0] = (borders[kBins - 1] + borders[kBins]) * .5f - two_pi;
    out[1] = s_dist[kBins - 1];
    out[(kRows - 1) * 2 + 0] = (borders[0] + borders[1]) * .5f + two_pi;
    out[(kRows - 1) * 2 + 1] = s_dist[0];
  }
}

// check_occupancy (:118-160).  blockIdx.y = slice i, which owns the points [i * step, (i + 1) * step); blockIdx.y = y_res: the
// remainder points, which no slice touches (is_occupied = 1 / T > thresh, is_visible = 0).  Lane = query point; the T tables of the
// slice are staged in LDS (T * 362 * 8 B).
__global__ __launch_bounds__(256) void lidar_occupancy_kernel(const float* __restrict__ q_pts, int P, const float* __restrict__ tables, int y_res,
                                                              int T, const float* __restrict__ world_to_velo, float min_dist, float thresh,
                                                              unsigned char* __restrict__ is_occupied, unsigned char* __restrict__ is_visible) {
  extern __shared__ float s_tab[];   // (T, 362, 2)
  const int step = P / y_res;
  const int slice = blockIdx.y;
  const float fT = (float)T;
  if (slice == y_res) {
    const int i = y_res * step + blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
      const float acc = 1.0f / fT;
      is_occupied[i] = acc > thresh ? 1 : 0;
      is_visible[i] = 0;
    }
    return;
  }
  if (blockIdx.x * 256 >= step) return;   // (the whole work-group)
  const float* src = tables + (long)slice * T * kRows * 2;
  for (int i = threadIdx.x; i < T * kRows * 2; i += 256) s_tab[i] = src[i];
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= step) return;
  const long idx = (long)slice * step + k;
  const float px = q_pts[idx * 3 + 0], py = q_pts[idx * 3 + 1], pz = q_pts[idx * 3 + 2];
  float acc = 1.0f;   // the reference starts its vote at ones_like (:119)
  bool visible = false;
  for (int j = 0; j < T; ++j) {
    const float* M = world_to_velo + j * 16;   // (wave-uniform)
    // pts_velo = world_to_velo @ [p, 1] (:132)
    const float vx = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
    const float vy = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7];
    const float vz = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11];
    const float vw = ((M[12] * px + M[13] * py) + M[14] * pz) + M[15];
    const float angle = atan2f(vy, vx);
    // the norm over ALL FOUR components, the homogeneous 1 included: the reference's torch.norm(pts_velo, dim=-1) (:136), kept on purpose
    const float dist = sqrtf(((vx * vx + vy * vy) + vz * vz) + vw * vw);
    // indices = searchsorted(table angles, angle): the first row whose angle is >= the query's, found on the table's own values (:138)
    const float* tab = s_tab + j * kRows * 2;
    int lo = 0, hi = kRows;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tab[mid * 2] < angle) lo = mid + 1;
      else hi = mid;
    }
    lo = min(max(lo, 1), kRows - 1);   // an angle in [-pi, pi] lands in 1 .. 361 by itself; a NaN must not index outside the table
    const float la = tab[(lo - 1) * 2], ld = tab[(lo - 1) * 2 + 1], ra = tab[lo * 2], rd = tab[lo * 2 + 1];
    const float interp = (angle - la) / (ra - la);
    const float surface = ld * (1.0f - interp) + rd * interp;
    const bool occ = (dist > surface) | (dist < min_dist);
    acc += occ ? 1.0f : 0.0f;
    if (j == 0) visible = !occ;   // the first cloud alone decides visibility (:153)
  }
  acc /= fT;
  is_occupied[idx] = acc > thresh ? 1 : 0;
  is_visible[idx] = visible ? 1 : 0;
}

// BTSWrapper.forward :296-298 + :308 + :314-330 per query point: predicted visibility (project_into_cam :163-168, a nearest,
// border-clamped, align_corners=True look-up in the predicted z-depth map, dist <= pred_dist), predicted occupancy sigma > threshold,
// V = is_visible | is_visible_pred, O = is_occupied & !V, and the cell of (V, O, P) in bts_eval_device.h's order, counted by its
// count_cells.  masks (3, P): P, O, V as bytes, when given.
__global__ __launch_bounds__(256) void occ_metrics_kernel(const float* __restrict__ q_pts, int P, const float* __restrict__ sigma,
                                                          const unsigned char* __restrict__ is_occupied, const unsigned char* __restrict__ is_visible,
                                                          const float* __restrict__ depth_z, int H, int W, const float* __restrict__ proj,
                                                          const float* __restrict__ w2c, float occ_threshold, int* __restrict__ counts,
                                                          unsigned char* __restrict__ masks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < P;
  int cell = -1;
  if (valid) {
    const float px = q_pts[(long)i * 3 + 0], py = q_pts[(long)i * 3 + 1], pz = q_pts[(long)i * 3 + 2];
    // cam_pts = proj @ (inverse(pose)[:3, :] @ [p, 1]) (:165)
    const float cx = ((w2c[0] * px + w2c[1] * py) + w2c[2] * pz) + w2c[3];
    const float cy = ((w2c[4] * px + w2c[5] * py) + w2c[6] * pz) + w2c[7];
    const float cz = ((w2c[8] * px + w2c[9] * py) + w2c[10] * pz) + w2c[11];
    const float ux = (proj[0] * cx + proj[1] * cy) + proj[2] * cz;
    const float uy = (proj[3] * cx + proj[4] * cy) + proj[5] * cz;
    const float dist = (proj[6] * cx + proj[7] * cy) + proj[8] * cz;
    const float gx = ux / dist, gy = uy / dist;
    // grid_sample(mode="nearest", padding_mode="border", align_corners=True) (:297)
    const float pred_dist = depth_z[nearest_border_texel(gx, gy, H, W)];
    const bool vis_pred = dist <= pred_dist;
    const bool Pm = sigma[i] > occ_threshold;
    const bool V = (is_visible[i] != 0) | vis_pred;
    const bool O = (is_occupied[i] != 0) & !V;
    // the twin of bbox_metrics_kernel's lines (bts_bbox_occ.hip): as a function of bts_eval_device.h they change both kernels' instructions
    cell = V ? (Pm ? 0 : 1) : (O ? (Pm ? 2 : 3) : (Pm ? 4 : 5));
    if (masks) {
      masks[i] = Pm ? 1 : 0;
      masks[(long)P + i] = O ? 1 : 0;
      masks[2L * P + i] = V ? 1 : 0;
    }
  }
  count_cells(cell, counts);
}

// torch.linspace(lo, hi, y_res) in fp32 (:59) and the slice bounds of :67-72
static void slice_bounds(float y_lo, float y_hi, int y_res, LidarSliceBounds* yb) {
  if (y_res == 1) {
    yb->lo[0] = y_lo, yb->hi[0] = y_hi;
    return;
  }
  const float stepf = (y_hi - y_lo) / (float)(y_res - 1);
  float ys[BTS_LIDAR_MAX_SLICES];
  for (int i = 0; i < y_res; ++i) ys[i] = i < y_res / 2 ? y_lo + stepf * (float)i : y_hi - stepf * (float)(y_res - i - 1);
  const float half = (ys[1] - ys[0]) / 2.0f;
  for (int i = 0; i < y_res; ++i) yb->lo[i] = ys[i] - half, yb->hi[i] = ys[i] + half;
}


// THE layout of bts_lidar_slices' workspace: the per-bin minima (y_res, T, 360) and the smallest-angle keys (y_res, T)
LidarBins lidar_bins_layout(Carver& w, int T, int y_res) {
  LidarBins b;
  b.bins = w.take<unsigned>((size_t)y_res * T * kBins);
  b.first = w.take<unsigned long long>((size_t)y_res * T);
  return b;
}

size_t lidar_bins_bytes(int T, int y_res) {
  Carver count(nullptr);
  lidar_bins_layout(count, T, y_res);
  return count.bytes();
}

// THE layout of bts_occupancy_eval's workspace.  tables and sigma keep their slots when the caller brings buffers of its own, so the
// size does not depend on which outputs were asked for
OccEvalWs occ_eval_layout(Carver& w, int P, int T, int y_res) {
  OccEvalWs o;
  o.bins = w.take<char>(lidar_bins_bytes(T, y_res));
  o.tables = w.take<float>((size_t)y_res * T * kRows * 2);
  o.w2v = w.take<float>((size_t)T * 16);
  o.w2c = w.take<float>(16);
  o.is_occ = w.take<unsigned char>((size_t)P);
  o.is_vis = w.take<unsigned char>((size_t)P);
  o.sigma = w.take<float>((size_t)P);
  return o;
}

// offsets: HOST array of T + 1 point offsets (validated by the caller)
int lidar_slices_launch(const float* points, const int* offsets, int T, const float* velo_poses, const float* borders, float y_lo, float y_hi,
                        int y_res, float max_dist, void* bins_ws, float* tables, hipStream_t s) {
  LidarOffsets offs;
  int max_n = 0;
  for (int t = 0; t <= T; ++t) offs.off[t] = offsets[t];
  for (int t = 0; t < T; ++t) max_n = offsets[t + 1] - offsets[t] > max_n ? offsets[t + 1] - offsets[t] : max_n;
  LidarSliceBounds yb;
  slice_bounds(y_lo, y_hi, y_res, &yb);
  Carver carve(bins_ws);
  const LidarBins b = lidar_bins_layout(carve, T, y_res);
  const int n_bins = y_res * T * kBins, n_first = y_res * T;
  lidar_init_kernel<<<(n_bins + 255) / 256, 256, 0, s>>>(b.bins, b.first, n_bins, n_first);
  if (int rc = launch_code()) return rc;
  const int per_block = 256 * 8;
  lidar_bins_kernel<<<dim3((max_n + per_block - 1) / per_block, T), 256, 0, s>>>(reinterpret_cast<const float4*>(points), offs, velo_poses, borders, yb,
                                                                               y_res, max_dist, per_block, T, b.bins, b.first);
  if (int rc = launch_code()) return rc;
  lidar_table_kernel<<<y_res * T, 64, 0, s>>>(b.bins, b.first, borders, tables);
  return launch_code();
}

int lidar_occupancy_launch(const float* q_pts, int P, const float* tables, int y_res, int T, const float* world_to_velo, float min_dist,
                           unsigned char* is_occupied, unsigned char* is_visible, hipStream_t s) {
  const int dyn = T * kRows * 2 * 4;   // 92 672 B at T = 32
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(lidar_occupancy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != hipSuccess) {
    (void)launch_code();
    return BTS_E_LAUNCH;
  }
  const int step = P / y_res, rest = P - y_res * step;
  const int gx = ((step > rest ? step : rest) + 255) / 256;
  const float thresh = (float)((double)(T - 2) / (double)T);   // :122, compared in fp32 as torch compares a fp32 tensor with a Python scalar
  lidar_occupancy_kernel<<<dim3(gx > 0 ? gx : 1, y_res + 1), 256, dyn, s>>>(q_pts, P, tables, y_res, T, world_to_velo, min_dist, thresh, is_occupied,
                                                                           is_visible);
  return launch_code();
}

int occ_metrics_launch(const float* q_pts, int P, const float* sigma, const unsigned char* is_occupied, const unsigned char* is_visible,
                       const float* depth_z, int H, int W, const float* proj, const float* w2c, float occ_threshold, int* counts,
                       unsigned char* masks, hipStream_t s) {
  if (hipMemsetAsync(counts, 0, 6 * sizeof(int), s) != hipSuccess) {
    (void)launch_code();
    return BTS_E_LAUNCH;
  }
  occ_metrics_kernel<<<(P + 255) / 256, 256, 0, s>>>(q_pts, P, sigma, is_occupied, is_visible, depth_z, H, W, proj, w2c, occ_threshold, counts, masks);
  return launch_code();
}

}  // namespace bts
