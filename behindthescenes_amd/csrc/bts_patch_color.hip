// Patch colours (image_processor {type: patch}, models/bts/model/image_processor.py:69-93): every colour frame stands for its
// PatchProcessor(3) output, 27 channels (y * 3 + x) * 3 + c = the RGB frame at the nine clamped integer shifts (y - 1, x - 1).  The
// 27-channel frames are never formed: a bilinear border tap of them is a tap of the rgb0 frames the renderer holds with a SECOND clamp,
//   colour[(y, x, c)] = sum_{a, b} w_ab * rgb0[clamp(y_a + y - 1, 0, H - 1), clamp(x_b + x - 1, 0, W - 1)].c
// with make_taps_xy's y_0, y_1, x_0, x_1 and its four weights (bts_common.h).  Of the six row indices clamp(y_a + dy) two are the same
// texel row whatever the border does -- clamp(y_0 + 1) = min(y_0 + 1, H - 1) = y_1 = clamp(y_1 + 0) -- so five rows and five columns, 25
// texels, serve the 36 (tap, shift) pairs; at a border clamp(y_1 - 1) is NOT y_0 (y_1 = y_0 = H - 1 gives H - 2) and nothing else merges.
// Colours are linear in the compositing weights, so the render runs unchanged and these kernels form rgb from its weights:
//   pc_fwd_kernel    lane = sample: its 27 colours of one render view times w_k into LDS, then one lane per (ray, channel) sums the ray's K
//                    products front to back; rgb_samps on request.  A work-group takes 256 / K whole rays, or one ray in chunks of 256 samples.
//   pc_bwd_kernel    lane = sample: the taps again, g_weights[k] = sum_{v, ch} g_rgb[v, ch] colour[k, v, ch] (- sum g_rgb with white_bkgd);
//                    the ray's incoming gradients are staged in LDS one view at a time.  Written, never accumulated.
//   pc_query_kernel  lane = point: the colours of n x P world points.
// fp32, fixed-order sums, no atomics: a rerun is bit-identical.  A sample's position in a render view is the render kernels' (o + z d with
// an unfused multiply-add, project<false>, make_taps); a sample outside a view reads the clamped border colours, as padding_mode="border".
#include "bts_host.h"

#include <cstring>

namespace bts {

constexpr int kPcThreads = 256;
constexpr int kPcPatch = 3;                            // the one compiled patch size
constexpr int kPcCh = 3 * kPcPatch * kPcPatch;         // 27

struct PcParams {
  const float *rays, *z_samp, *weights, *xyz;          // (B, 8), (B, K), (B, K) | (n, P, 3)
  const float *imgs, *K_r, *w2c_r;                     // (n, nv, H, W, 4), (n, nv, 9), (n, nv, 16)
  const float* g_rgb;                                  // (B, nv * 27)
  float *rgb, *rgb_samps, *g_weights;                  // (B, nv * 27), (B, K, nv * 27) or null, (B, K)
  long Bp, B;                                          // rays (points) per batch element, n * Bp
  int nv, H, W, K, white_bkgd;
  int R, chunks;                                       // rays per work-group, chunks of 256 samples per ray
};

// the 27 colours of the point (px, py, pz) in render view `view` (= sample * nv + v)
__device__ __forceinline__ void pc_colours(const PcParams& p, long view, float px, float py, float pz, float (&col)[kPcCh]) {
  const Cam cj = load_cam_v(p.w2c_r + view * 16, p.K_r + view * 9);
  const Proj pc = project<false>(cj, px, py, pz);
  int x0, y0, x1, y1;
  const Taps tc = make_taps_xy(pc.x, pc.y, p.H, p.W, x0, y0, x1, y1);
  const int Hm = p.H - 1, Wm = p.W - 1;
  const auto cl = [](int i, int hi) { return max(0, min(i, hi)); };
  // rows / columns 0: clamp(i_0 - 1), 1: i_0, 2: i_1 (= clamp(i_0 + 1)), 3: clamp(i_1 - 1), 4: clamp(i_1 + 1); every index is clamped again, so
  // no coordinate (a NaN's either) leaves the frame
  const int ry[5] = {cl(y0 - 1, Hm), cl(y0, Hm), cl(y1, Hm), cl(y1 - 1, Hm), cl(y1 + 1, Hm)};
  const int cx[5] = {cl(x0 - 1, Wm), cl(x0, Wm), cl(x1, Wm), cl(x1 - 1, Wm), cl(x1 + 1, Wm)};
  constexpr int kOf[2][3] = {{0, 1, 2}, {3, 2, 4}};   // [tap a][shift d + 1] -> the index above
  const float4* img = reinterpret_cast<const float4*>(p.imgs) + view * p.H * p.W;
  float4 t[5][5];
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int c = 0; c < 5; ++c) t[r][c] = img[ry[r] * p.W + cx[c]];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 a = t[kOf[0][dy]][kOf[0][dx]], b = t[kOf[0][dy]][kOf[1][dx]], cc = t[kOf[1][dy]][kOf[0][dx]], d = t[kOf[1][dy]][kOf[1][dx]];
      float* o = col + (dy * 3 + dx) * 3;
      o[0] = ((a.x * tc.w00 + b.x * tc.w01) + cc.x * tc.w10) + d.x * tc.w11;   // the render kernels' order
      o[1] = ((a.y * tc.w00 + b.y * tc.w01) + cc.y * tc.w10) + d.y * tc.w11;
      o[2] = ((a.z * tc.w00 + b.z * tc.w01) + cc.z * tc.w10) + d.z * tc.w11;
    }
}

// this lane's sample in chunk `chunk` of the work-group's rays
struct PcLane {
  int r_loc, k;
  long ray;
  bool live;
};
__device__ __forceinline__ PcLane pc_lane(const PcParams& p, long ray0, int chunk) {
  const int tid = threadIdx.x;
  PcLane l;
  if (p.chunks == 1) {
    l.r_loc = tid / p.K;
    l.k = tid - l.r_loc * p.K;
  } else {
    l.r_loc = 0;
    l.k = chunk * kPcThreads + tid;
  }
  l.ray = ray0 + l.r_loc;
  l.live = l.r_loc < p.R && l.ray < p.B && l.k < p.K;
  return l;
}
// the sample's world point: nerf.py:231, multiply then add
__device__ __forceinline__ void pc_point(const PcParams& p, const PcLane& l, float& px, float& py, float& pz) {
  const float* rr = p.rays + l.ray * 8;
  const float z = p.z_samp[l.ray * p.K + l.k];
  px = rr[0] + z * rr[3], py = rr[1] + z * rr[4], pz = rr[2] + z * rr[5];
}

__global__ __launch_bounds__(kPcThreads) void pc_fwd_kernel(const PcParams p) {
  __shared__ float s_c[kPcThreads][kPcCh];   // w_k * colour; the odd stride spreads the lanes' rows over the banks
  __shared__ float s_w[kPcThreads];
  const int tid = threadIdx.x, K = p.K;
  const long ray0 = (long)blockIdx.x * p.R;
  const auto store = [&](long ray, int v, int ch, float acc, float wsum) {
    p.rgb[(ray * p.nv + v) * kPcCh + ch] = p.white_bkgd ? (acc + 1.0f) - wsum : acc;   // nerf.py:301-304
  };
  for (int v = 0; v < p.nv; ++v) {
    float acc = 0.0f, wsum = 0.0f;   // a ray in chunks: lane ch < 27 carries channel ch's sums from chunk to chunk
    for (int chunk = 0; chunk < p.chunks; ++chunk) {
      const PcLane l = pc_lane(p, ray0, chunk);
      __syncthreads();   // the previous round's sums are done with s_c
      if (l.live) {
        float px, py, pz, col[kPcCh];
        pc_point(p, l, px, py, pz);
        const long view = (l.ray / p.Bp) * p.nv + v;
        pc_colours(p, view, px, py, pz, col);
        const long i = l.ray * K + l.k;
        const float w = p.weights[i];
        s_w[tid] = w;
#pragma unroll
        for (int ch = 0; ch < kPcCh; ++ch) s_c[tid][ch] = w * col[ch];
        if (p.rgb_samps) {
          float* o = p.rgb_samps + (i * p.nv + v) * kPcCh;
#pragma unroll
          for (int ch = 0; ch < kPcCh; ++ch) o[ch] = col[ch];
        }
      }
      __syncthreads();
      if (p.chunks == 1) {
        // one lane per (ray, channel), front to back
        for (int e = tid; e < p.R * kPcCh; e += kPcThreads) {
          const int r = e / kPcCh, ch = e - r * kPcCh;
          if (ray0 + r >= p.B) break;
          float a = 0.0f, ws = 0.0f;
          for (int kk = 0; kk < K; ++kk) a = a + s_c[r * K + kk][ch], ws = ws + s_w[r * K + kk];
          store(ray0 + r, v, ch, a, ws);
        }
      } else if (tid < kPcCh) {
        const int cnt = min(kPcThreads, K - chunk * kPcThreads);
        for (int kk = 0; kk < cnt; ++kk) acc = acc + s_c[kk][tid], wsum = wsum + s_w[kk];
      }
    }
    if (p.chunks > 1 && tid < kPcCh) store(ray0, v, tid, acc, wsum);
  }
}

__global__ __launch_bounds__(kPcThreads) void pc_bwd_kernel(const PcParams p) {
  __shared__ float s_g[kPcThreads][kPcCh];   // the incoming gradients of the work-group's rays, one render view at a time
  const int tid = threadIdx.x, K = p.K;
  const long ray0 = (long)blockIdx.x * p.R;
  for (int chunk = 0; chunk < p.chunks; ++chunk) {
    const PcLane l = pc_lane(p, ray0, chunk);
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (l.live) pc_point(p, l, px, py, pz);
    float acc = 0.0f, gsum = 0.0f;
    for (int v = 0; v < p.nv; ++v) {
      __syncthreads();   // the previous view's readers are done
      for (int e = tid; e < p.R * kPcCh; e += kPcThreads) {
        const int r = e / kPcCh, ch = e - r * kPcCh;
        s_g[r][ch] = ray0 + r < p.B ? p.g_rgb[((ray0 + r) * p.nv + v) * kPcCh + ch] : 0.0f;
      }
      __syncthreads();
      if (l.live) {
        float col[kPcCh];
        pc_colours(p, (l.ray / p.Bp) * p.nv + v, px, py, pz, col);
#pragma unroll
        for (int ch = 0; ch < kPcCh; ++ch) {
          const float g = s_g[l.r_loc][ch];
          acc = __builtin_fmaf(g, col[ch], acc), gsum = gsum + g;
        }
      }
    }
    if (l.live) p.g_weights[l.ray * K + l.k] = p.white_bkgd ? acc - gsum : acc;   // rgb += 1 - sum(weights): d/dw_k = -sum(g_rgb)
  }
}

__global__ __launch_bounds__(kPcThreads) void pc_query_kernel(const PcParams p) {
  const long idx = (long)blockIdx.x * kPcThreads + threadIdx.x;
  if (idx >= p.B) return;
  const float* x = p.xyz + idx * 3;
  for (int v = 0; v < p.nv; ++v) {
    float col[kPcCh];
    pc_colours(p, (idx / p.Bp) * p.nv + v, x[0], x[1], x[2], col);
    float* o = p.rgb + (idx * p.nv + v) * kPcCh;
#pragma unroll
    for (int ch = 0; ch < kPcCh; ++ch) o[ch] = col[ch];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
bool patch_color_size_ok(int patch) { return patch == kPcPatch; }

static int pc_params(PcParams& p, const BtsPatchColor* a, long per_sample, const char* who) {
  memset(&p, 0, sizeof(p));
  p.imgs = a->imgs_nhwc4, p.K_r = a->K_r, p.w2c_r = a->w2c_r;
  p.Bp = per_sample, p.B = (long)a->n * per_sample;
  p.nv = a->nv, p.H = a->H, p.W = a->W, p.white_bkgd = a->white_bkgd;
  if (p.B > 0x7FF00000L) {
    set_error("%s: too many rays or points in one call (%ld)", who, p.B);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}
static void pc_ray_geometry(PcParams& p, const BtsPatchColor* a) {
  p.rays = a->rays, p.z_samp = a->z_samp, p.weights = a->weights, p.K = a->K;
  p.R = a->K <= kPcThreads ? kPcThreads / a->K : 1;
  p.chunks = a->K <= kPcThreads ? 1 : (a->K + kPcThreads - 1) / kPcThreads;
}
static int pc_status(const char* who) { return launch_check("%s: kernel launch failed (HIP error %ld)", who); }

int patch_color_fwd_impl(const BtsPatchColor* a, hipStream_t s) {
  PcParams p;
  if (int rc = pc_params(p, a, a->rays_per_sample, "bts_patch_color_fwd")) return rc;
  pc_ray_geometry(p, a);
  p.rgb = a->rgb, p.rgb_samps = a->rgb_samps;
  pc_fwd_kernel<<<(int)((p.B + p.R - 1) / p.R), kPcThreads, 0, s>>>(p);
  return pc_status("bts_patch_color_fwd");
}

int patch_color_bwd_impl(const BtsPatchColor* a, const float* g_rgb, float* g_weights, hipStream_t s) {
  PcParams p;
  if (int rc = pc_params(p, a, a->rays_per_sample, "bts_patch_color_bwd")) return rc;
  pc_ray_geometry(p, a);
  p.g_rgb = g_rgb, p.g_weights = g_weights;
  pc_bwd_kernel<<<(int)((p.B + p.R - 1) / p.R), kPcThreads, 0, s>>>(p);
  return pc_status("bts_patch_color_bwd");
}

int patch_color_query_impl(const BtsPatchColor* a, const float* xyz, int P, float* rgb, hipStream_t s) {
  PcParams p;
  if (int rc = pc_params(p, a, P, "bts_patch_color_query")) return rc;
  p.xyz = xyz, p.rgb = rgb;
  pc_query_kernel<<<(int)((p.B + kPcThreads - 1) / kPcThreads), kPcThreads, 0, s>>>(p);
  return pc_status("bts_patch_color_query");
}

}  // namespace bts
