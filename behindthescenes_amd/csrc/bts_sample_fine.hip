// bts_sample_fine.hip -- what sits between the coarse and the fine render of NeRFRenderer.forward (models/common/render/nerf.py:161-208,
// 356-367) and sample_coarse_from_dist (:125-159) in ONE launch: a ray's coarse weights -> its pdf and cdf -> the importance draws by
// inverse-cdf search, the draws around the coarse depth, and the ascending merge with the coarse depths.  include/bts_render.h lists
// the reference's quirks next to bts_sample_fine.  No backward: the render has no gradient with respect to z_samp and the reference
// detaches the weights.
//   a wave takes 64 / K' rays at once, K' = the power of two at or above the largest per-ray count of the call (K' <= 64: segmented
//   butterflies / scans inside K' lanes; above: one ray, a lane holds 2 or 4 values, template NPL).  Per ray slot of a wave, LDS slabs
//   of K' * NPL words:
//     cdf   the inclusive scan of pdf_k = (w_k + 1e-5) / S (the leading 0 of the reference's cdf is implicit: upper_bound(cdf, u) - 1
//           clamped at 0 IS the number of scan entries that are not above u)
//     zz    from-dist only: the (reciprocal) depths the borders are read from
//   every lane searches its ray's cdf slab with a fixed number of steps; the merge is a bitonic network in registers over keys that
//   order like torch.sort (the sign-flipped bit pattern, every NaN last), element e of the sorted row is output e: a coalesced store.
// Plain fp32, IEEE divisions, no contraction.  The only atomic is the integer NaN counter (at most one per wave, none when the wave
// produced no NaN); reruns are bit-identical.  Control flow is uniform per launch: every lane reaches the one barrier.
#include <hip/hip_runtime.h>

#include "bts_host.h"

namespace bts {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct SampleParams {
  const float *rays, *weights, *z_in, *depth, *u, *t, *noise;
  float *z_out, *z_depth_out;
  int* nan_count;
  long B;
  int Kc;             // weights per ray (from-dist: ns)
  int n_imp;          // importance draws per ray (from-dist: n_coarse)
  int Kfd;            // depth draws per ray
  int Ktot;           // values per ray of the merge / of z_out
  int seg_log2;       // a ray's lanes = 1 << seg_log2
  int search_top;     // the largest power of two <= Kc
  int lindisp, sorted;
  float depth_std;
};

// torch.min / torch.max of two tensors: a NaN operand gives NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float torch_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ float torch_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// keys that order like torch.sort's ascending floats: negative < positive by the flipped bit pattern, every NaN last (the keys of the
// NaN bit patterns are free: the largest two are the NaN key and, behind it, the key of an empty slot of the merge)
constexpr unsigned kNanKey = 0xFFFFFFFEu, kPadKey = 0xFFFFFFFFu;
__device__ __forceinline__ unsigned sort_key(float v) {
  const unsigned b = __float_as_uint(v);
  if (v != v) return kNanKey;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
  if (k == kNanKey) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// searchsorted(cdf, u, right=True) - 1 clamped at 0 over the reference's [0 | scan] = the number of scan entries that are NOT above u
// (ATen's own comparison: a NaN u walks to the end).  Fixed trip count: top, top / 2, ... 1; every read is below Kc.
__device__ __forceinline__ int count_not_above(const float* cdf, int Kc, int top, float u) {
  int pos = 0;
  for (int step = top; step >= 1; step >>= 1) {
    const int nxt = pos + step;
    if (nxt <= Kc && !(cdf[nxt - 1] > u)) pos = nxt;
  }
  return pos;
}

// borders = [z_0, (z_i + z_{i-1}) / 2, z_{ns-1}] over the staged (reciprocal) depths; 0 <= i <= ns
__device__ __forceinline__ float border_at(const float* zz, int ns, int i) {
  if (i == 0) return zz[0];
  if (i == ns) return zz[ns - 1];
  return 0.5f * (zz[i] + zz[i - 1]);
}

// kFromDist = false: sample_fine | sample_fine_depth | the sorted union with z_in (z_in == NULL: the two pieces, unsorted);
// kFromDist = true: sample_coarse_from_dist over (weights, z_in)
template <int NPL, bool kFromDist>
__global__ __launch_bounds__(kThreads) void sample_fine_kernel(const SampleParams p) {
  __shared__ float s_cdf[kWaves * 64 * NPL];
  __shared__ float s_zz[kFromDist ? kWaves * 64 * NPL : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = 1 << p.seg_log2, sl = lane & (seg - 1), slot = lane >> p.seg_log2;   // NPL > 1: seg = 64, slot = 0
  const long ray = ((long)blockIdx.x * kWaves + wave) * (64 >> p.seg_log2) + slot;
  const bool act = ray < p.B;
  const long r0 = act ? ray : 0;
  float* cdf = s_cdf + wave * 64 * NPL + slot * seg * NPL;
  float* zz = kFromDist ? s_zz + wave * 64 * NPL + slot * seg * NPL : s_zz;
  const int Kc = p.Kc, n_imp = p.n_imp, Ktot = p.Ktot;

  if (kFromDist || n_imp > 0) {
    const float* wrow = p.weights + r0 * Kc;
    float w[NPL];
    float S = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int k = sl + i * seg;
      w[i] = (act && k < Kc) ? wrow[k] + 1e-5f : 0.0f;
      S += w[i];
    }
    for (int off = seg >> 1; off >= 1; off >>= 1) S += __shfl_xor(S, off, 64);
    float carry = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int k = sl + i * seg;
      float v = w[i] / S;
      for (int off = 1; off < seg; off <<= 1) {
        const float up = __shfl_up(v, off, seg);
        if (sl >= off) v += up;
      }
      v = carry + v;
      if (k < Kc) cdf[k] = v;
      if (NPL > 1) carry = __shfl(v, 63, 64);
    }
    if (kFromDist) {
      const float* zrow = p.z_in + r0 * Kc;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int k = sl + i * seg;
        if (k < Kc) {
          const float z = act ? zrow[k] : 1.0f;
          zz[k] = p.lindisp ? 1.0f / z : z;
        }
      }
    }
  }
  __syncthreads();

  const float near = p.rays ? p.rays[r0 * 8 + 6] : 0.0f, far = p.rays ? p.rays[r0 * 8 + 7] : 0.0f;
  const int c0 = (!kFromDist && p.z_in) ? Kc : 0;      // the coarse depths lead the merge
  float cand[NPL];
  int nans = 0;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int o = sl + i * seg;
    float z = 0.0f;
    if (act && o < Ktot) {
      if (kFromDist) {
        const float u = p.u[ray * n_imp + o], t = p.t[ray * n_imp + o];
        int id = count_not_above(cdf, Kc, p.search_top, u);
        id = id < n_imp - 1 ? id : n_imp - 1;          // the reference clamps by n_coarse, not by ns
        const float left = border_at(zz, Kc, id), right = border_at(zz, Kc, id + 1);
        z = left * (1.0f - t) + right * t;
        if (p.lindisp) z = 1.0f / z;
        nans += z != z;
      } else if (o < c0) {
        z = p.z_in[ray * Kc + o];
      } else if (o - c0 < n_imp) {
        const int j = o - c0;
        const float u = p.u[ray * n_imp + j], t = p.t[ray * n_imp + j];
        const int ind = count_not_above(cdf, Kc, p.search_top, u);      // no upper clamp: u at or above the last entry gives Kc
        z = depth_at(((float)ind + t) / (float)Kc, near, far, p.lindisp != 0);
        nans += z != z;
      } else {
        const int j = o - c0 - n_imp;
        z = __fadd_rn(p.depth[ray], __fmul_rn(p.noise[ray * p.Kfd + j], p.depth_std));
        z = torch_max(torch_min(z, far), near);
        nans += z != z;
      }
    }
    cand[i] = z;
  }
  if (p.nan_count) {
    for (int off = 32; off >= 1; off >>= 1) nans += __shfl_xor(nans, off, 64);
    if (lane == 0 && nans) atomicAdd(p.nan_count, nans);
  }

  if (!p.sorted) {      // the pieces, or from-dist as drawn
    if (act) {
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int o = sl + i * seg;
        if (o >= Ktot) continue;
        if (kFromDist || o < n_imp) p.z_out[ray * n_imp + o] = cand[i];
        else p.z_depth_out[ray * p.Kfd + (o - n_imp)] = cand[i];
      }
    }
    return;             // (uniform: `sorted` is a launch constant)
  }

  // the merge: a bitonic network over the ray's 1 << seg_log2 lanes x NPL registers, element e = sl + i * seg.  Partners less than a
  // segment apart are another lane's register (__shfl_xor inside the segment), the others this lane's own; the slots behind Ktot
  // carry the largest key and end up behind it, so element e of the sorted row IS output e.  No LDS, no barrier; values only, like
  // the reference, which discards torch.sort's permutation
  unsigned mine[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) mine[i] = sl + i * seg < Ktot ? sort_key(cand[i]) : kPadKey;
  const int N = seg * NPL;
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (NPL == 1 || j < seg) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          const unsigned other = __shfl_xor(mine[i], j, 64);
          const int e = sl + i * seg;
          const bool keep_min = ((e & k) == 0) == ((e & j) == 0);
          mine[i] = keep_min ? (other < mine[i] ? other : mine[i]) : (other > mine[i] ? other : mine[i]);
        }
      } else {
        const int jj = j >> 6;      // NPL > 1: seg = 64, the partner is register i ^ jj
#pragma unroll
        for (int q = 1; q < NPL; q <<= 1) {
          if (q != jj) continue;
#pragma unroll
          for (int i = 0; i < NPL; ++i) {
            if (i & q) continue;
            const unsigned a = mine[i], b = mine[i | q];
            const bool up = ((sl + i * seg) & k) == 0;
            const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
            mine[i] = up ? lo : hi, mine[i | q] = up ? hi : lo;
          }
        }
      }
    }
  }
  if (act) {
    float* out = p.z_out + ray * Ktot;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int o = sl + i * seg;
      if (o < Ktot) out[o] = key_value(mine[i]);
    }
  }
}

template <bool kFromDist>
void launch(const SampleParams& p, int kmax, unsigned grid, hipStream_t s) {
  if (kmax <= 64) sample_fine_kernel<1, kFromDist><<<grid, kThreads, 0, s>>>(p);
  else if (kmax <= 128) sample_fine_kernel<2, kFromDist><<<grid, kThreads, 0, s>>>(p);
  else sample_fine_kernel<4, kFromDist><<<grid, kThreads, 0, s>>>(p);
}

}  // namespace

// the entry has checked the arguments (bts_api.hip): every per-ray count is at most 256
int sample_fine_launch(const BtsSampleFineArgs* a, hipStream_t s) {
  const bool from_dist = a->mode == BTS_SAMPLE_FROM_DIST;
  SampleParams p;
  p.rays = a->rays, p.weights = a->weights, p.z_in = a->z_coarse, p.depth = a->depth, p.u = a->u, p.t = a->t, p.noise = a->noise;
  p.z_out = a->z_out, p.z_depth_out = a->z_depth_out, p.nan_count = a->nan_count;
  p.B = (long)a->B, p.Kc = a->Kc, p.lindisp = a->lindisp ? 1 : 0, p.depth_std = a->depth_std;
  int kmax;
  if (from_dist) {
    p.n_imp = a->n_coarse, p.Kfd = 0, p.Ktot = a->n_coarse, p.sorted = a->sorted ? 1 : 0;
    kmax = a->Kc;
  } else {
    p.n_imp = a->Kf - a->Kfd, p.Kfd = a->Kfd;
    p.sorted = a->z_coarse ? 1 : 0;
    p.Ktot = a->z_coarse ? a->Kc + a->Kf : a->Kf;
    kmax = a->Kc + a->Kf;
  }
  p.seg_log2 = 1;
  while ((1 << p.seg_log2) < kmax && p.seg_log2 < 6) ++p.seg_log2;
  p.search_top = 1;
  while (p.search_top * 2 <= p.Kc) p.search_top *= 2;
  const long per_group = (long)kWaves * (64 >> p.seg_log2);
  const unsigned grid = (unsigned)((p.B + per_group - 1) / per_group);
  if (from_dist) launch<true>(p, kmax, grid, s);
  else launch<false>(p, kmax, grid, s);
  return launch_code();
}

}  // namespace bts
