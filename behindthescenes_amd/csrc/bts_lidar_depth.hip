// load_depth of the reference's two KITTI data sets (datasets/kitti_raw/kitti_raw_dataset.py:256-302, datasets/kitti_360/
// kitti_360_dataset.py:505-539): a Velodyne cloud projected and scattered into the ground-truth depth map of a frame.  One clear of the
// workspace and two launches on the caller's stream; nothing synchronises.
//
//   points pass: thread = point (grid-stride, blockIdx.y = frame): the front filter, the projection, the pixel index, the bounds test;
//                per pixel a record of four integers -- the count, the lowest and the highest index of its points, the minimum of z as
//                the order-preserving integer image of its bits (bts_common.h: float_key; double_key below for an fp64 P);
//   pixels pass: thread = pixel: the closed form of the reference's scatter and its "duplicates" loop from the pixel's record and its
//                key partner's, the clamp, the Eigen crop.  The z of a pixel's last point is formed again from that point by the same
//                device function the points pass ran (the same bits, and no plane of one z per point).
// Integer atomics only, so a rerun is bit-identical.  The rules (include/bts_render.h lists them) are reproduced ON PURPOSE; the plain
// z-buffer -- the nearest point of every pixel -- is a different function.
#include "bts_host.h"

namespace bts {

constexpr int kThreads = 256;
constexpr int kPointBlocks = 1024;   // the points pass's grid per frame at most: 262 144 points a trip

// monotone map double -> uint64, float_key's 64-bit counterpart
__device__ __forceinline__ unsigned long long double_key(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double double_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

template <class T>
struct Real;
template <>
struct Real<float> {
  using Key = unsigned;
  static __device__ __forceinline__ Key key(float z) { return float_key(z); }
  static __device__ __forceinline__ float unkey(Key k) { return float_unkey(k); }
  static __device__ __forceinline__ float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
  static __device__ __forceinline__ float rint(float a) { return rintf(a); }
};
template <>
struct Real<double> {
  using Key = unsigned long long;
  static __device__ __forceinline__ Key key(double z) { return double_key(z); }
  static __device__ __forceinline__ double unkey(Key k) { return double_unkey(k); }
  static __device__ __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
  static __device__ __forceinline__ double rint(double a) { return ::rint(a); }
};

template <class T>
struct LidarDepthGeom {
  const float* points;                          // (N, 4); column 3 is taken as 1
  const T* P;                                   // (3, 4)
  long long off[BTS_LIDAR_DEPTH_MAX_FRAMES + 1];
  int B, H, W, n_px, raw, eigen;
  int crop[4];                                  // rule 8: rows [crop0, crop1), columns [crop2, crop3)
  unsigned *cnt, *hi, *lo;                      // (B, H * W) each
  typename Real<T>::Key* zmin;                  // (B, H * W)
  T* out;                                       // (B, H, W)
};

// One row of u = P . (x, y, z, 1): the products accumulated left to right with one rounding per term, the order of a BLAS kernel's
// inner loop over k (np.dot at :265 / :513)
template <class T>
__device__ __forceinline__ T dot_row(const T* __restrict__ r, T x, T y, T z) {
  return Real<T>::fma(r[3], (T)1, Real<T>::fma(r[2], z, Real<T>::fma(r[1], y, r[0] * x)));
}

// Rules 1-4 for point i of the concatenated array.  false: the point is dropped; else its pixel and z = u2
template <class T>
__device__ __forceinline__ bool project_point(const LidarDepthGeom<T>& g, long long i, int& px_x, int& px_y, T& z) {
  const float4 p = *reinterpret_cast<const float4*>(g.points + 4 * i);
  if (g.raw && !(p.x >= 0.0f)) return false;                                   // kitti_raw :262
  const T x = (T)p.x, y = (T)p.y, zz = (T)p.z;
  const T u0 = dot_row(g.P, x, y, zz), u1 = dot_row(g.P + 4, x, y, zz), u2 = dot_row(g.P + 8, x, y, zz);
  T fx = u0 / u2, fy = u1 / u2;                                                // :266 / :514
  if (g.raw) {
    fx = Real<T>::rint(fx) - (T)1, fy = Real<T>::rint(fy) - (T)1;              // :274-275
  } else {
    fx = Real<T>::rint((fx * (T)0.5 + (T)0.5) * (T)g.W);                       // :517-518
    fy = Real<T>::rint((fy * (T)0.5 + (T)0.5) * (T)g.H);
  }
  // (NaN and u2 == 0 fall out through the comparisons, as in numpy)
  if (!(fx >= (T)0 && fy >= (T)0 && fx < (T)g.W && fy < (T)g.H)) return false;
  px_x = (int)fx, px_y = (int)fy, z = u2;
  return true;
}

template <class T>
__global__ __launch_bounds__(kThreads) void lidar_depth_points_kernel(LidarDepthGeom<T> g) {
  const int f = blockIdx.y;
  const long long first = g.off[f], n = g.off[f + 1] - first;
  const size_t plane = (size_t)f * g.n_px;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    int x, y;
    T z;
    if (!project_point(g, first + i, x, y, z)) continue;
    const size_t q = plane + (size_t)y * g.W + x;
    atomicAdd(&g.cnt[q], 1u);
    atomicMin(&g.lo[q], (unsigned)i);
    atomicMax(&g.hi[q], (unsigned)i);
    atomicMin(&g.zmin[q], Real<T>::key(z));
  }
}

template <class T>
__global__ __launch_bounds__(kThreads) void lidar_depth_pixels_kernel(LidarDepthGeom<T> g) {
  const int f = blockIdx.y;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= g.n_px) return;
  const size_t plane = (size_t)f * g.n_px;
  const int y = q / g.W, x = q - y * g.W;
  const unsigned n_q = g.cnt[plane + q];
  T z = (T)0;
  if (n_q) {
    // the other pixel of key y * (W - 1) + x - 1 (:285 / :530): (y, W - 1) and (y + 1, 0) share one
    int partner = -1;
    if (x == g.W - 1 && y + 1 < g.H) partner = q + 1;
    else if (x == 0 && y > 0) partner = q - 1;
    const unsigned n_p = partner >= 0 ? g.cnt[plane + partner] : 0u;
    const bool group = n_q + n_p >= 2u;                                        // Counter(inds) > 1 (:286 / :531)
    if (group && (!n_p || g.lo[plane + q] < g.lo[plane + partner])) {          // pts[0] lies here (:289-291 / :534-536)
      typename Real<T>::Key k = g.zmin[plane + q];
      if (n_p) {
        const typename Real<T>::Key kp = g.zmin[plane + partner];
        k = kp < k ? kp : k;
      }
      z = Real<T>::unkey(k);
    } else {                                                                   // the fancy assignment's last write (:282 / :527)
      int xx, yy;
      (void)project_point(g, g.off[f] + g.hi[plane + q], xx, yy, z);
    }
    if (z < (T)0) z = (T)0;                                                    // :292 / :537
    if (g.eigen) {                                                             // :295-300, on the value as a double
      const double d = (double)z;
      if (!(d > 1e-3 && d < 80.0 && y >= g.crop[0] && y < g.crop[1] && x >= g.crop[2] && x < g.crop[3])) z = (T)0;
    }
  }
  g.out[plane + q] = z;
}

// THE layout of bts_lidar_depth's workspace: count | highest index (cleared to 0) | lowest index | minimum key (cleared to all ones)
template <class T>
static size_t lidar_depth_layout(Carver& w, LidarDepthGeom<T>& g, size_t px) {
  g.cnt = w.take<unsigned>(px);
  g.hi = w.take<unsigned>(px);
  const size_t zeros = w.bytes() - kAlign;
  g.lo = w.take<unsigned>(px);
  g.zmin = w.take<typename Real<T>::Key>(px);
  return zeros;
}

size_t lidar_depth_bytes(int B, int H, int W, bool p_fp64) {
  Carver count(nullptr);
  const size_t px = (size_t)B * H * W;
  if (p_fp64) {
    LidarDepthGeom<double> g;
    (void)lidar_depth_layout(count, g, px);
  } else {
    LidarDepthGeom<float> g;
    (void)lidar_depth_layout(count, g, px);
  }
  return count.bytes();
}

template <class T>
static int lidar_depth_launch_t(const BtsLidarDepth* a, void* workspace, hipStream_t s) {
  LidarDepthGeom<T> g;
  g.points = a->points, g.P = static_cast<const T*>(a->P), g.out = static_cast<T*>(a->depth);
  g.B = a->B, g.H = a->H, g.W = a->W, g.n_px = a->H * a->W, g.raw = a->convention == BTS_LIDAR_DEPTH_KITTI_RAW, g.eigen = a->eigen_depth != 0;
  long long n_max = 0;
  for (int f = 0; f <= a->B; ++f) g.off[f] = a->offsets[f];
  for (int f = 0; f < a->B; ++f) n_max = n_max > g.off[f + 1] - g.off[f] ? n_max : g.off[f + 1] - g.off[f];
  // :296, the reference's own products on doubles, truncated as astype(np.int32) truncates them
  g.crop[0] = (int)(0.40810811 * a->H), g.crop[1] = (int)(0.99189189 * a->H);
  g.crop[2] = (int)(0.03594771 * a->W), g.crop[3] = (int)(0.96405229 * a->W);
  Carver carve(workspace);
  const size_t px = (size_t)a->B * g.n_px;
  const size_t zeros = lidar_depth_layout(carve, g, px);
  char* base = reinterpret_cast<char*>(g.cnt);
  const size_t total = carve.bytes() - kAlign;
  if (hipMemsetAsync(base, 0, zeros, s) != hipSuccess || hipMemsetAsync(base + zeros, 0xFF, total - zeros, s) != hipSuccess) {
    (void)launch_code();
    return BTS_E_LAUNCH;
  }
  if (n_max > 0) {
    long long blocks = (n_max + kThreads - 1) / kThreads;
    const long long cap = a->max_blocks > 0 ? a->max_blocks : kPointBlocks;
    if (blocks > cap) blocks = cap;
    lidar_depth_points_kernel<T><<<dim3((unsigned)blocks, a->B), kThreads, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
  }
  lidar_depth_pixels_kernel<T><<<dim3((g.n_px + kThreads - 1) / kThreads, a->B), kThreads, 0, s>>>(g);
  return launch_code();
}

int lidar_depth_launch(const BtsLidarDepth* a, void* workspace, hipStream_t s) {
  return a->p_fp64 ? lidar_depth_launch_t<double>(a, workspace, s) : lidar_depth_launch_t<float>(a, workspace, s);
}

}  // namespace bts
