// What the reference's demo scripts do to a rendered novel view before it becomes a video frame (scripts/inference_setup.py:182-198
// render_poses, utils/plotting.py:41-46 color_tensor, scripts/videos/gen_vid_nvs.py:102-120, gen_vid_transition.py:140-171,
// gen_vid_seq.py:108-137): the invalid mask, the inverse-depth normalisation, matplotlib's colour map, the panels' concatenation
// and the conversion to bytes -- on the device, into a zero-filled (P, Hc, Wc, 3) uint8 canvas.  Nothing synchronises.
//
//   frames_minmax_kernel       per image: the partial min / max / "a NaN was seen" of up to kFramesPartials work-groups (two-stage reduce:
//                              the consumer's first wave folds the partials; min and max do not depend on the order, so a rerun is
//                              bit-identical and nothing needs initialising)
//   colorize_kernel            color_tensor: optional (x - min) / (max - min), the colour-map index, then either three doubles per
//                              pixel or three bytes into a canvas panel
//   pack_u8_kernel             a float image, read through element strides, as x * scale + shift into a canvas panel
//   novel_view_finish_kernel   render_poses' mask (+ black_invalid) on the render's rgb / depth / invalid_wsum, the image panel and
//                              the colour-mapped inverse-depth panel
//
// Plain fp32 with correctly rounded division (__fdiv_rn), no contraction, no reciprocal approximations: the panels are compared byte
// for byte with numpy / torch on the host.  Quirks of the reference that are reproduced ON PURPOSE are listed in include/bts_render.h.
#include "bts_host.h"
#include "bts_eval_device.h"

namespace bts {

constexpr int kFramesThreads = 256;
constexpr int kFramesPartials = BTS_FRAMES_PARTIALS;   // work-groups of the min / max pre-pass per image = lanes of the wave that folds them

struct CanvasDev {
  unsigned char* data;
  int Hc, Wc;
};

// matplotlib's Colormap.__call__ on a float32 array (colors.py): xa *= N in fp32; xa == N -> N - 1; < 0 -> under (N), >= N -> over
// (N + 1), NaN -> bad (N + 2); otherwise astype(int), a truncation
__device__ __forceinline__ int cmap_index(float x, int N) {
  const float t = x * (float)N;
  if (t != t) return N + 2;
  if (t == (float)N) return N - 1;
  if (t < 0.0f) return N;
  if (t >= (float)N) return N + 1;
  return (int)t;
}

// numpy's (v * 255).astype(uint8) for v in [0, 1]; outside it (numpy's result is unspecified there) saturated, NaN -> 0
__device__ __forceinline__ unsigned char to_u8(float v) {
  const double t = (double)v * 255.0;
  if (!(t > 0.0)) return 0;
  return t >= 255.0 ? (unsigned char)255 : (unsigned char)(int)t;
}

__device__ __forceinline__ void canvas_put(const CanvasDev& cv, int p, int y, int x, unsigned char r, unsigned char g, unsigned char b) {
  unsigned char* o = cv.data + (((size_t)p * cv.Hc + y) * cv.Wc + x) * 3;
  o[0] = r, o[1] = g, o[2] = b;
}

// partials (B, kFramesPartials, 3): min, max, NaN flag (0 / 1) of the pixels this work-group strides over; +inf / -inf for none
__global__ __launch_bounds__(kFramesThreads) void frames_minmax_kernel(const float* __restrict__ x, long n, float* __restrict__ partials) {
  __shared__ float s_lo[kFramesThreads / 64], s_hi[kFramesThreads / 64], s_nan[kFramesThreads / 64];
  const int b = blockIdx.y, t = threadIdx.x;
  const float* xb = x + (size_t)b * n;
  float lo = __int_as_float(0x7F800000), hi = __int_as_float(0xFF800000), bad = 0.0f;
  for (long i = (long)blockIdx.x * kFramesThreads + t; i < n; i += (long)gridDim.x * kFramesThreads) {
    const float v = xb[i];
    if (v != v) bad = 1.0f;
    else lo = fminf(lo, v), hi = fmaxf(hi, v);
  }
  const MinMaxBad m = lane0_minmax(lo, hi, bad);
  lo = m.lo, hi = m.hi, bad = m.bad;
  if ((t & 63) == 0) s_lo[t >> 6] = lo, s_hi[t >> 6] = hi, s_nan[t >> 6] = bad;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kFramesThreads / 64; ++w) lo = fminf(lo, s_lo[w]), hi = fmaxf(hi, s_hi[w]), bad = fmaxf(bad, s_nan[w]);
    float* o = partials + ((size_t)b * kFramesPartials + blockIdx.x) * 3;
    o[0] = lo, o[1] = hi, o[2] = bad;
  }
}

// the image's min / max from its `nb` partials, by the first wave of a work-group; a NaN anywhere makes both NaN (torch's min() / max())
__device__ __forceinline__ void fold_minmax(const float* __restrict__ partials, int b, int nb, float* s_mm) {
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    const float* p = partials + ((size_t)b * kFramesPartials + l) * 3;
    float lo = l < nb ? p[0] : __int_as_float(0x7F800000), hi = l < nb ? p[1] : __int_as_float(0xFF800000), bad = l < nb ? p[2] : 0.0f;
    // (the steps of lane0_minmax, written out: called as that function this fold changes colorize_kernel's instructions)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) minmax_step(lo, hi, bad, o);
    if (l == 0) {
      const float nan = __int_as_float(0x7FC00000);
      s_mm[0] = bad != 0.0f ? nan : lo, s_mm[1] = bad != 0.0f ? nan : hi;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kFramesThreads) void colorize_kernel(const float* __restrict__ x, int h, int w, int N, const float* __restrict__ partials,
                                                                  int nb, const double* __restrict__ lut, const unsigned char* __restrict__ lut_u8,
                                                                  double* __restrict__ out, CanvasDev cv, int row0, int col0) {
  __shared__ float s_mm[2];
  const int b = blockIdx.y;
  const long n = (long)h * w;
  if (partials) fold_minmax(partials, b, nb, s_mm);
  const long i = (long)blockIdx.x * kFramesThreads + threadIdx.x;
  if (i >= n) return;
  float v = x[(size_t)b * n + i];
  if (partials) v = __fdiv_rn(v - s_mm[0], s_mm[1] - s_mm[0]);     // a constant image: 0 / 0 = NaN, the bad colour
  const int k = cmap_index(v, N);
  if (out) {
    double* o = out + ((size_t)b * n + i) * 3;
    o[0] = lut[3 * k], o[1] = lut[3 * k + 1], o[2] = lut[3 * k + 2];
  }
  if (cv.data) {
    const int y = (int)(i / w), xx = (int)(i - (long)y * w);
    canvas_put(cv, b, row0 + y, col0 + xx, lut_u8[3 * k], lut_u8[3 * k + 1], lut_u8[3 * k + 2]);
  }
}

__global__ __launch_bounds__(kFramesThreads) void pack_u8_kernel(const float* __restrict__ x, long sb, long sy, long sx, long sc, int h, int w, float scale,
                                                                 float shift, CanvasDev cv, int row0, int col0) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * kFramesThreads + threadIdx.x;
  if (i >= (long)h * w) return;
  const int y = (int)(i / w), xx = (int)(i - (long)y * w);
  const float* p = x + b * sb + y * sy + xx * sx;
  canvas_put(cv, b, row0 + y, col0 + xx, to_u8(p[0] * scale + shift), to_u8(p[sc] * scale + shift), to_u8(p[2 * sc] * scale + shift));
}

struct FinishParams {
  float* rgb;                  // (P, h * w, 3)
  float* depth;                // (P, h * w)
  const float* wsum;           // (P, h * w)
  const float* norm_range;     // (P, 2): 1 / d_max and 1 / d_min - 1 / d_max, rounded to fp32 by the host
  const float* partials;       // the depth's min / max partials (black_invalid) or NULL
  const unsigned char* lut_u8; // (N + 3, 3)
  int nb, h, w, N, black_invalid, write_back;
  CanvasDev cv;
  int img_row0, img_col0, dep_row0, dep_col0;   // negative row: panel off
};

__global__ __launch_bounds__(kFramesThreads) void novel_view_finish_kernel(const FinishParams q) {
  __shared__ float s_mm[2];
  const int p = blockIdx.y;
  const long n = (long)q.h * q.w;
  if (q.partials) fold_minmax(q.partials, p, q.nb, s_mm);
  const long i = (long)blockIdx.x * kFramesThreads + threadIdx.x;
  if (i >= n) return;
  const size_t ray = (size_t)p * n + i;
  float d = q.depth[ray], r = q.rgb[3 * ray], g = q.rgb[3 * ray + 1], bl = q.rgb[3 * ray + 2];
  if (q.black_invalid && q.wsum[ray] > 0.8f) {      // the threshold as fp32: the comparison runs on a float32 tensor (:192)
    d = s_mm[1], r = g = bl = 0.0f;                 // depth.max() over ALL pixels, before any assignment (:195-196)
    if (q.write_back) q.depth[ray] = d, q.rgb[3 * ray] = 0.0f, q.rgb[3 * ray + 1] = 0.0f, q.rgb[3 * ray + 2] = 0.0f;
  }
  const int y = (int)(i / q.w), x = (int)(i - (long)y * q.w);
  if (q.img_row0 >= 0) canvas_put(q.cv, p, q.img_row0 + y, q.img_col0 + x, to_u8(r), to_u8(g), to_u8(bl));
  if (q.dep_row0 >= 0) {
    // ((1 / depth - 1 / d_max) / (1 / d_min - 1 / d_max)).clamp(0, 1) (gen_vid_nvs.py:106); a NaN stays a NaN (the bad colour)
    float t = __fdiv_rn(__fdiv_rn(1.0f, d) - q.norm_range[2 * p], q.norm_range[2 * p + 1]);
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    const int k = cmap_index(t, q.N);
    canvas_put(q.cv, p, q.dep_row0 + y, q.dep_col0 + x, q.lut_u8[3 * k], q.lut_u8[3 * k + 1], q.lut_u8[3 * k + 2]);
  }
}

static int frames_blocks(long n) { return (int)((n + kFramesThreads - 1) / kFramesThreads); }
static int frames_partials(long n) {
  const long b = (n + 4 * kFramesThreads - 1) / (4 * kFramesThreads);
  return (int)(b < kFramesPartials ? b : kFramesPartials);
}

int colorize_launch(const float* x, int B, int h, int w, int norm, int N, const double* lut, const unsigned char* lut_u8, float* partials,
                    double* out, unsigned char* canvas, int Hc, int Wc, int row0, int col0, hipStream_t s) {
  const long n = (long)h * w;
  const int nb = frames_partials(n);
  if (norm) {
    frames_minmax_kernel<<<dim3(nb, B), kFramesThreads, 0, s>>>(x, n, partials);
    if (int rc = launch_code()) return rc;
  }
  colorize_kernel<<<dim3(frames_blocks(n), B), kFramesThreads, 0, s>>>(x, h, w, N, norm ? partials : nullptr, nb, lut, lut_u8, out,
                                                                       CanvasDev{canvas, Hc, Wc}, row0, col0);
  return launch_code();
}

int pack_u8_launch(const float* x, long sb, long sy, long sx, long sc, int B, int h, int w, float scale, float shift, unsigned char* canvas,
                   int Hc, int Wc, int row0, int col0, hipStream_t s) {
  pack_u8_kernel<<<dim3(frames_blocks((long)h * w), B), kFramesThreads, 0, s>>>(x, sb, sy, sx, sc, h, w, scale, shift, CanvasDev{canvas, Hc, Wc},
                                                                                row0, col0);
  return launch_code();
}

// the max pre-pass (black_invalid only) and the finish kernel on a chunk's render
int novel_view_finish_launch(const BtsNovelViews* a, hipStream_t s) {
  const long n = (long)a->h * a->w;
  FinishParams q;
  q.rgb = a->rgb, q.depth = a->depth, q.wsum = a->invalid_wsum, q.norm_range = a->norm_range, q.lut_u8 = a->lut_u8;
  q.partials = nullptr, q.nb = frames_partials(n);
  q.h = a->h, q.w = a->w, q.N = a->lut_N, q.black_invalid = a->black_invalid, q.write_back = a->write_masked;
  q.cv = CanvasDev{a->canvas, a->Hc, a->Wc};
  q.img_row0 = a->canvas ? a->img_row0 : -1, q.img_col0 = a->img_col0, q.dep_row0 = a->canvas ? a->depth_row0 : -1, q.dep_col0 = a->depth_col0;
  if (a->black_invalid) {
    frames_minmax_kernel<<<dim3(q.nb, a->P), kFramesThreads, 0, s>>>(a->depth, n, a->frame_max);
    if (int rc = launch_code()) return rc;
    q.partials = a->frame_max;
  }
  novel_view_finish_kernel<<<dim3(frames_blocks(n), a->P), kFramesThreads, 0, s>>>(q);
  return launch_code();
}

}  // namespace bts
