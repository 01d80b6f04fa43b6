// BTSWrapper.compute_depth_metrics (models/bts/evaluator.py:96-151; evaluator_nvs.py:96-139 is the same function without scaling) as a
// handful of short fp32 kernels: the nearest resize of the prediction to the ground truth's size, median or least-squares scaling, the
// clamp, the seven metrics of the paper's depth table.  One row of twelve floats per frame stays on the device; nothing synchronises.
//
// Launches (blockIdx.y = frame, a work-group takes kPerBlock consecutive ground-truth pixels of it):
//   median: one clear of the histograms, three radix passes over 11 + 11 + 10 bits of the ordered bit pattern of the floats -- for the
//           median of gt[mask] and of pred[mask] at once --, the metrics pass, finish;
//   l2:     the moments pass, a one-work-group solve, the metrics pass, finish;
//   none:   the metrics pass, finish.
// No float atomics: the histograms are integer atomics (LDS, then the non-zero bins to global), every sum is an fp64 partial per
// work-group in a workspace slot that `finish` adds in slot order, so a rerun is bit-identical.  No work-group reads what another one
// wrote in the same launch: a radix pass rescans the previous pass's 2 048 bins itself, and what work-group 0 notes down for later
// (the prefix and the rank inside it) is read by the next launch only.
//
// Quirks of the reference that are reproduced ON PURPOSE:
//   - two masks: the scaling is fitted over gt > 0 (:104, :108), the metrics run over gt != 0 (:117) -- a negative ground-truth value
//     enters the metrics (and makes rmse_log NaN through log) but not the scaling;
//   - torch.median is the LOWER median, the element of rank (N - 1) / 2 (:105);
//   - F.interpolate's nearest source index is min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out in fp32 (:101),
//     not the exact rational (they differ e.g. for 26 -> 44 and 30 -> 58);
//   - a1 .. a3 compare against the fp32 roundings of 1.25, 1.25 ** 2, 1.25 ** 3 (:123-125).
// Outside the contract: NaN or inf in pred or gt (torch.maximum and torch.clamp propagate a NaN, a radix selection orders it; nothing
// faults, the row is unspecified), -0.0 in pred next to +0.0 at the median's rank (torch's sort calls them equal), and l2 scaling of a
// rank-deficient system (fewer than two distinct predictions under the mask: the coefficients are not finite here, LAPACK returns the
// minimum-norm solution).  N = 0 gives a NaN row and zero counts.
#include "bts_host.h"
#include "bts_eval_device.h"
#include "bts_loss_device.h"

namespace bts {

constexpr int kThreads = 256;
constexpr int kPerBlock = 2048;       // ground-truth pixels per work-group: two 16-byte loads per lane
constexpr int kBinsRadix = 2048;      // 11 bits; the last pass uses the lower 1 024 bins
constexpr int kHistFrame = 3 * 2 * kBinsRadix;   // uint32 per frame: (pass, gt | pred, bin)
constexpr int kStateFrame = 32;       // uint32 per frame: three notes of eight words
constexpr int kSlotDoubles = 8;       // a partial: four fp64 sums, then five int32 counts

struct DepthGeom {
  const float* pred;
  const float* gt;
  int H, W, Hg, Wg, n_px, nblk, vec, mode;
  float sh, sw, clamp_lo, clamp_hi;
  unsigned* hist;     // (B, 3, 2, 2048)
  unsigned* state;    // (B, 32)
  double* part;       // (B, nblk, 8)  the metrics pass
  double* mom;        // (B, nblk, 8)  the moments pass
};

// (upsample_nearest2d's source index of :101 is bts_common.h's nearest_src)
__device__ __forceinline__ float pred_at(const DepthGeom& g, const float* pred_f, int i) {
  const int y = i / g.Wg, x = i - y * g.Wg;
  return pred_f[(size_t)nearest_src(y, g.sh, g.H) * g.W + nearest_src(x, g.sw, g.W)];
}

// the four ground-truth pixels i0 .. i0 + 3 of a frame; 0 (= no measurement, in neither mask) past its end
__device__ __forceinline__ void load_gt4(const float* gt_f, int i0, int n_px, int vec, float (&v)[4]) {
  if (vec && i0 + 3 < n_px) {
    const float4 q = *reinterpret_cast<const float4*>(gt_f + i0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n_px ? gt_f[i0 + k] : 0.0f;
  }
}

// One radix pass of the two medians (:104-105).  PASS 0: bits 31..21 of every key under gt > 0.  PASS 1: bits 20..10 of the keys whose
// upper 11 bits are the bin of the wanted rank in pass 0's histogram.  PASS 2: bits 9..0 of the keys that share 22 bits.
// state words of a frame: [0..4] prefix_gt, rank_gt, prefix_pred, rank_pred, N after pass 0's histogram; [8..12] the same after pass 1's.
template <int PASS>
__global__ __launch_bounds__(kThreads) void depth_hist_kernel(DepthGeom g) {
  __shared__ unsigned s_hist[2 * kBinsRadix];
  __shared__ unsigned s_scan[kThreads];
  __shared__ unsigned s_sel[2][3];
  const int f = blockIdx.y;
  const float* gt_f = g.gt + (size_t)f * g.n_px;
  const float* pred_f = g.pred + (size_t)f * g.H * g.W;
  unsigned* hist_f = g.hist + (size_t)f * kHistFrame;
  unsigned* state_f = g.state + (size_t)f * kStateFrame;
  for (int i = threadIdx.x; i < 2 * kBinsRadix; i += kThreads) s_hist[i] = 0u;
  unsigned want_g = 0u, want_p = 0u;
  if (PASS == 1) {
    select_bin<true>(hist_f, 1, 0u, s_scan, s_sel[0]);
    select_bin<true>(hist_f + kBinsRadix, 1, 0u, s_scan, s_sel[1]);
    want_g = s_sel[0][0], want_p = s_sel[1][0];
    if (blockIdx.x == 0 && threadIdx.x == 0)
      state_f[0] = want_g, state_f[1] = s_sel[0][1], state_f[2] = want_p, state_f[3] = s_sel[1][1], state_f[4] = s_sel[0][2];
  } else if (PASS == 2) {
    const unsigned pg = state_f[0], rg = state_f[1], pp = state_f[2], rp = state_f[3], n = state_f[4];
    select_bin<true>(hist_f + 2 * kBinsRadix, 0, rg, s_scan, s_sel[0]);
    select_bin<true>(hist_f + 3 * kBinsRadix, 0, rp, s_scan, s_sel[1]);
    want_g = (pg << 11) | s_sel[0][0], want_p = (pp << 11) | s_sel[1][0];
    if (blockIdx.x == 0 && threadIdx.x == 0)
      state_f[8] = want_g, state_f[9] = s_sel[0][1], state_f[10] = want_p, state_f[11] = s_sel[1][1], state_f[12] = n;
  }
  __syncthreads();
  const int base = blockIdx.x * kPerBlock;
#pragma unroll
  for (int j = 0; j < kPerBlock / (kThreads * 4); ++j) {
    const int i0 = base + (j * kThreads + threadIdx.x) * 4;
    float v[4];
    load_gt4(gt_f, i0, g.n_px, g.vec, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (v[k] > 0.0f) {
        const unsigned kg = float_key(v[k]), kp = float_key(pred_at(g, pred_f, i0 + k));
        if (PASS == 0) {
          atomicAdd(&s_hist[kg >> 21], 1u);
          atomicAdd(&s_hist[kBinsRadix + (kp >> 21)], 1u);
        } else if (PASS == 1) {
          if ((kg >> 21) == want_g) atomicAdd(&s_hist[(kg >> 10) & 2047u], 1u);
          if ((kp >> 21) == want_p) atomicAdd(&s_hist[kBinsRadix + ((kp >> 10) & 2047u)], 1u);
        } else {
          if ((kg >> 10) == want_g) atomicAdd(&s_hist[kg & 1023u], 1u);
          if ((kp >> 10) == want_p) atomicAdd(&s_hist[kBinsRadix + (kp & 1023u)], 1u);
        }
      }
    }
  }
  __syncthreads();
  unsigned* dst = hist_f + PASS * 2 * kBinsRadix;
  for (int i = threadIdx.x; i < 2 * kBinsRadix; i += kThreads) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(&dst[i], c);
  }
}

// the work-group's four fp64 sums and up to five counts into its slot, in a fixed order: lanes, then waves
__device__ void store_partial(double (&s)[4], int (&c)[5], double* slot) {
  __shared__ double s_d[kThreads / 64][4];
  __shared__ int s_c[kThreads / 64][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = lane0_sum(s[k]);
#pragma unroll
  for (int k = 0; k < 5; ++k) c[k] = lane0_sum(c[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_d[wave][k] = s[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) s_c[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double a = s_d[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; ++w) a += s_d[w][threadIdx.x];
    slot[threadIdx.x] = a;
  } else if (threadIdx.x < 9) {
    const int k = threadIdx.x - 4;
    int a = 0;
    for (int w = 0; w < kThreads / 64; ++w) a += s_c[w][k];
    reinterpret_cast<int*>(slot + 4)[k] = a;
  }
}

// l2 scaling (:108-113): the moments of the normal equations over gt > 0 -- sum p, sum p^2, sum g, sum p g in fp64 (the products of two
// fp32 values are exact there) and N
__global__ __launch_bounds__(kThreads) void depth_moments_kernel(DepthGeom g) {
  const int f = blockIdx.y;
  const float* gt_f = g.gt + (size_t)f * g.n_px;
  const float* pred_f = g.pred + (size_t)f * g.H * g.W;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int c[5] = {0, 0, 0, 0, 0};
  const int base = blockIdx.x * kPerBlock;
#pragma unroll
  for (int j = 0; j < kPerBlock / (kThreads * 4); ++j) {
    const int i0 = base + (j * kThreads + threadIdx.x) * 4;
    float v[4];
    load_gt4(gt_f, i0, g.n_px, g.vec, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (v[k] > 0.0f) {
        const double p = (double)pred_at(g, pred_f, i0 + k), q = (double)v[k];
        s[0] += p, s[1] += p * p, s[2] += q, s[3] += p * q;
        c[0] += 1;
      }
    }
  }
  store_partial(s, c, g.mom + ((size_t)f * g.nblk + blockIdx.x) * kSlotDoubles);
}

// x = lstsq([p, 1], g) (:113) from the moments, in fp64, rounded to fp32 once.  One wave per frame; state words [16], [17] = x0, x1.
__global__ __launch_bounds__(64) void depth_solve_kernel(DepthGeom g) {
  __shared__ double s_m[5];
  const int f = blockIdx.x, lane = threadIdx.x;
  const double* mom_f = g.mom + (size_t)f * g.nblk * kSlotDoubles;
  if (lane < 4) {
    double a = 0.0;
    for (int b = 0; b < g.nblk; ++b) a += mom_f[(size_t)b * kSlotDoubles + lane];
    s_m[lane] = a;
  } else if (lane == 4) {
    long long n = 0;
    for (int b = 0; b < g.nblk; ++b) n += reinterpret_cast<const int*>(mom_f + (size_t)b * kSlotDoubles + 4)[0];
    s_m[4] = (double)n;
  }
  __syncthreads();
  if (lane == 0) {
    const double sp = s_m[0], spp = s_m[1], sg = s_m[2], spg = s_m[3], n = s_m[4];
    const double det = n * spp - sp * sp;
    const double x0 = (n * spg - sp * sg) / det, x1 = (spp * sg - sp * spg) / det;
    unsigned* state_f = g.state + (size_t)f * kStateFrame;
    state_f[16] = __float_as_uint((float)x0), state_f[17] = __float_as_uint((float)x1);
  }
}

// :105-106 / :114, :116-140 per pixel.  Partials per work-group: sums of (g - p)^2, (log g - log p)^2, |g - p| / g, (g - p)^2 / g and
// the counts of gt != 0, gt > 0, a1, a2, a3.  mode 1: the last radix step (the bin of the wanted rank among the keys that share 22 bits)
// gives both medians; work-group 0 notes scale and shift for `finish` (state words [16], [17]).
__global__ __launch_bounds__(kThreads) void depth_terms_kernel(DepthGeom g) {
  __shared__ unsigned s_scan[kThreads];
  __shared__ unsigned s_sel[2][3];
  const int f = blockIdx.y;
  const float* gt_f = g.gt + (size_t)f * g.n_px;
  const float* pred_f = g.pred + (size_t)f * g.H * g.W;
  unsigned* state_f = g.state + (size_t)f * kStateFrame;
  float x0 = 1.0f, x1 = 0.0f;
  if (g.mode == 1) {
    const unsigned pg = state_f[8], rg = state_f[9], pp = state_f[10], rp = state_f[11], n = state_f[12];
    select_bin<true>(g.hist + (size_t)f * kHistFrame + 4 * kBinsRadix, 0, rg, s_scan, s_sel[0]);
    select_bin<true>(g.hist + (size_t)f * kHistFrame + 5 * kBinsRadix, 0, rp, s_scan, s_sel[1]);
    const float med_g = float_unkey((pg << 10) | s_sel[0][0]), med_p = float_unkey((pp << 10) | s_sel[1][0]);
    x0 = n ? med_g / med_p : __uint_as_float(0x7FC00000u);   // the median of an empty selection
    if (blockIdx.x == 0 && threadIdx.x == 0) state_f[16] = __float_as_uint(x0), state_f[17] = __float_as_uint(0.0f);
  } else if (g.mode == 2) {
    x0 = __uint_as_float(state_f[16]), x1 = __uint_as_float(state_f[17]);
  }
  const float t1 = 1.25f, t2 = 1.5625f, t3 = 1.953125f;   // (float)1.25, (float)(1.25 ** 2), (float)(1.25 ** 3): all three exact
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int c[5] = {0, 0, 0, 0, 0};
  const int base = blockIdx.x * kPerBlock;
#pragma unroll
  for (int j = 0; j < kPerBlock / (kThreads * 4); ++j) {
    const int i0 = base + (j * kThreads + threadIdx.x) * 4;
    float v[4];
    load_gt4(gt_f, i0, g.n_px, g.vec, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float q = v[k];
      if (q != 0.0f) {
        float p = pred_at(g, pred_f, i0 + k);
        if (g.mode == 1) p = __fmul_rn(x0, p);                       // :106
        else if (g.mode == 2) p = __fadd_rn(__fmul_rn(p, x0), x1);   // :114, two rounded operations
        p = p != p ? p : fminf(fmaxf(p, g.clamp_lo), g.clamp_hi);    // :116 (torch.clamp keeps a NaN)
        const float thresh = fmaxf(q / p, p / q);                    // :122
        const float d = q - p, sq = d * d;                           // :130
        const float lg = logf(q) - logf(p);                          // :133
        s[0] += (double)sq, s[1] += (double)(lg * lg), s[2] += (double)(fabsf(d) / q), s[3] += (double)(sq / q);   // :130, :133, :136, :139
        c[0] += 1, c[1] += q > 0.0f ? 1 : 0;
        c[2] += thresh < t1 ? 1 : 0, c[3] += thresh < t2 ? 1 : 0, c[4] += thresh < t3 ? 1 : 0;   // :123-125
      }
    }
  }
  store_partial(s, c, g.part + ((size_t)f * g.nblk + blockIdx.x) * kSlotDoubles);
}

// The means (:126-140) from the partials, in slot order.  One wave per frame.  row: abs_rel sq_rel rmse rmse_log a1 a2 a3 scale shift
// n_metric n_scale 0; counts: n_metric n_scale a1 a2 a3.
__global__ __launch_bounds__(64) void depth_finish_kernel(DepthGeom g, float* __restrict__ metrics, int* __restrict__ counts) {
  __shared__ double s_s[4];
  __shared__ long long s_c[5];
  const int f = blockIdx.x, lane = threadIdx.x;
  const double* part_f = g.part + (size_t)f * g.nblk * kSlotDoubles;
  if (lane < 4) {
    double a = 0.0;
    for (int b = 0; b < g.nblk; ++b) a += part_f[(size_t)b * kSlotDoubles + lane];
    s_s[lane] = a;
  } else if (lane < 9) {
    long long n = 0;
    for (int b = 0; b < g.nblk; ++b) n += reinterpret_cast<const int*>(part_f + (size_t)b * kSlotDoubles + 4)[lane - 4];
    s_c[lane - 4] = n;
  }
  __syncthreads();
  if (lane == 0) {
    const unsigned* state_f = g.state + (size_t)f * kStateFrame;
    const double n = (double)s_c[0];
    const float fn = (float)s_c[0];
    float* row = metrics + (size_t)f * 12;
    row[0] = (float)(s_s[2] / n);
    row[1] = (float)(s_s[3] / n);
    row[2] = sqrtf((float)(s_s[0] / n));
    row[3] = sqrtf((float)(s_s[1] / n));
    row[4] = (float)s_c[2] / fn, row[5] = (float)s_c[3] / fn, row[6] = (float)s_c[4] / fn;
    row[7] = g.mode ? __uint_as_float(state_f[16]) : 1.0f;
    row[8] = g.mode ? __uint_as_float(state_f[17]) : 0.0f;
    row[9] = fn, row[10] = (float)s_c[1], row[11] = 0.0f;
    if (counts) {
#pragma unroll
      for (int k = 0; k < 5; ++k) counts[(size_t)f * 5 + k] = (int)s_c[k];
    }
  }
}

static int n_blocks(int Hg, int Wg) { return (int)(((long)Hg * Wg + kPerBlock - 1) / kPerBlock); }

// THE layout of bts_depth_metrics' workspace: histograms | notes | partials of the metrics pass | partials of the moments pass, each per frame
static void depth_layout(Carver& w, DepthGeom& g, size_t B, size_t nblk) {
  g.hist = w.take<unsigned>(B * kHistFrame);
  g.state = w.take<unsigned>(B * kStateFrame);
  g.part = w.take<double>(B * nblk * kSlotDoubles);
  g.mom = w.take<double>(B * nblk * kSlotDoubles);
}

size_t depth_metrics_bytes(int B, int Hg, int Wg) {
  Carver count(nullptr);
  DepthGeom g;
  depth_layout(count, g, (size_t)B, (size_t)n_blocks(Hg, Wg));
  return count.bytes();
}

int depth_metrics_launch(const BtsDepthMetrics* a, void* workspace, hipStream_t s) {
  DepthGeom g;
  g.pred = a->pred, g.gt = a->gt;
  g.H = a->H, g.W = a->W, g.Hg = a->Hg, g.Wg = a->Wg, g.n_px = a->Hg * a->Wg, g.nblk = n_blocks(a->Hg, a->Wg), g.mode = a->mode;
  // 16-byte loads of gt where every frame starts on a 16-byte boundary
  g.vec = ((uintptr_t)a->gt & 15) == 0 && (a->B == 1 || (g.n_px & 3) == 0);
  g.sh = (float)a->H / (float)a->Hg, g.sw = (float)a->W / (float)a->Wg;
  g.clamp_lo = a->clamp_lo, g.clamp_hi = a->clamp_hi;
  Carver carve(workspace);
  depth_layout(carve, g, (size_t)a->B, (size_t)g.nblk);
  const dim3 grid(g.nblk, a->B);
  if (a->mode == 1) {
    if (hipMemsetAsync(g.hist, 0, (size_t)a->B * kHistFrame * 4, s) != hipSuccess) {
      (void)launch_code();
      return BTS_E_LAUNCH;
    }
    depth_hist_kernel<0><<<grid, kThreads, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
    depth_hist_kernel<1><<<grid, kThreads, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
    depth_hist_kernel<2><<<grid, kThreads, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
  } else if (a->mode == 2) {
    depth_moments_kernel<<<grid, kThreads, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
    depth_solve_kernel<<<a->B, 64, 0, s>>>(g);
    if (int rc = launch_code()) return rc;
  }
  depth_terms_kernel<<<grid, kThreads, 0, s>>>(g);
  if (int rc = launch_code()) return rc;
  depth_finish_kernel<<<a->B, 64, 0, s>>>(g, a->metrics, a->counts);
  return launch_code();
}

}  // namespace bts
