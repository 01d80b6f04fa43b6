// The render kernel of the default path (projected feature map G), software-pipelined for gfx950.
//
// lane = SAMPLE, like render_kernel in bts_field_kernel.h (one ray -- or 64/lpr short rays -- per wave iteration, XCD-contiguous
// ray ranges, persistent grid), but the iteration is laid out so that its long-latency pieces overlap instead of forming one
// dependency chain (section ablation of the previous kernel: 40 % of the time was exposed latency at 2 waves / SIMD):
//   * z of the NEXT ray is prefetched while the current ray is evaluated; with one ray per wave the ray itself is wave-uniform
//     and lives in scalar registers (s_load);
//   * colour taps (<= 2 views) are issued right after the geometry, they land during the MFMA phase;
//   * the gather of G runs three blocks ahead through a per-wave ring in LDS (GatherLds below) and is blended INTO the running
//     accumulators between the positional-encoding octaves: the MFMAs of a region cover the latency of the blocks behind it and
//     the blend's packed FMAs fill the matrix pipe's issue gaps (summation order only);
//   * alpha compositing is a DPP scan (row_shr / row_bcast) instead of ds_bpermute shuffles.
// Replaces: nerf.py:210-313, models_bts.py:138-338, resnetfc.py:132-184, code.py:30-42 of the reference.
#pragma once
#include "bts_field_kernel.h"

namespace bts {

#ifdef BTS_PROBE
#define BTS_TICK(i)                                                  \
  if (p.ablate & 128) {                                              \
    const unsigned long long t_now = __builtin_readcyclecounter();   \
    t_acc[i] += t_now - t_last;                                      \
    t_last = t_now;                                                  \
  }
#else
#define BTS_TICK(i)
#endif

// ---- DPP (data-parallel primitives) helpers: lanes whose source is outside its row / whose row is masked keep `old` ----------
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL,
                                                               ROW_MASK, 0xF, false));
}
constexpr int kDppRowShr = 0x110;   // + n
constexpr int kDppWaveShr1 = 0x138;  // lane i <- lane i - 1
constexpr int kDppWaveShl1 = 0x130;  // lane i <- lane i + 1
constexpr int kDppBcast15 = 0x142;  // lane 15 of each row -> every lane of the next row
constexpr int kDppBcast31 = 0x143;  // lane 31 -> rows 2, 3

// inclusive prefix product over each group of lpr consecutive lanes (lpr in {8, 16, 32, 64}); kl = lane & (lpr - 1).
// row_shr leaves `old` (the operation's identity) in the lanes whose source lies outside their 16-lane row, so for lpr >= 16 the shifted
// value needs no per-lane select and the DPP move folds into the multiply / add (one VALU instruction per step); only groups of 8
// lanes, which share a row with a neighbour group, mask the steps.
__device__ __forceinline__ float seg_scan_mul(float x, int lpr, int kl) {
  float y;
  if (lpr == 48) {   // lanes 0-47 one segment (rows 0, 1, 2), lanes 48-63 (row 3) another: see render_kernel_p's 48-lane mode
    x *= dpp_f<kDppRowShr + 1>(1.0f, x);
    x *= dpp_f<kDppRowShr + 2>(1.0f, x);
    x *= dpp_f<kDppRowShr + 4>(1.0f, x);
    x *= dpp_f<kDppRowShr + 8>(1.0f, x);
    x *= dpp_f<kDppBcast15, 0x2>(1.0f, x);   // row 1 <- row 0's total
    x *= dpp_f<kDppBcast31, 0x4>(1.0f, x);   // row 2 <- the scan through row 1
    return x;
  }
  if (lpr >= 16) {
    x *= dpp_f<kDppRowShr + 1>(1.0f, x);
    x *= dpp_f<kDppRowShr + 2>(1.0f, x);
    x *= dpp_f<kDppRowShr + 4>(1.0f, x);
    x *= dpp_f<kDppRowShr + 8>(1.0f, x);
  } else {
    y = dpp_f<kDppRowShr + 1>(1.0f, x), x *= (kl >= 1) ? y : 1.0f;
    y = dpp_f<kDppRowShr + 2>(1.0f, x), x *= (kl >= 2) ? y : 1.0f;
    y = dpp_f<kDppRowShr + 4>(1.0f, x), x *= (kl >= 4) ? y : 1.0f;
  }
  if (lpr >= 32) x *= dpp_f<kDppBcast15, 0xA>(1.0f, x);
  if (lpr >= 64) x *= dpp_f<kDppBcast31, 0xC>(1.0f, x);
  return x;
}
// inclusive prefix sum; the LAST lane of each group holds the group's total
__device__ __forceinline__ float seg_scan_add(float x, int lpr, int kl) {
  float y;
  if (lpr == 48) {
    x += dpp_f<kDppRowShr + 1>(0.0f, x);
    x += dpp_f<kDppRowShr + 2>(0.0f, x);
    x += dpp_f<kDppRowShr + 4>(0.0f, x);
    x += dpp_f<kDppRowShr + 8>(0.0f, x);
    x += dpp_f<kDppBcast15, 0x2>(0.0f, x);
    x += dpp_f<kDppBcast31, 0x4>(0.0f, x);
    return x;
  }
  if (lpr >= 16) {
    x += dpp_f<kDppRowShr + 1>(0.0f, x);
    x += dpp_f<kDppRowShr + 2>(0.0f, x);
    x += dpp_f<kDppRowShr + 4>(0.0f, x);
    x += dpp_f<kDppRowShr + 8>(0.0f, x);
  } else {
    y = dpp_f<kDppRowShr + 1>(0.0f, x), x += (kl >= 1) ? y : 0.0f;
    y = dpp_f<kDppRowShr + 2>(0.0f, x), x += (kl >= 2) ? y : 0.0f;
    y = dpp_f<kDppRowShr + 4>(0.0f, x), x += (kl >= 4) ? y : 0.0f;
  }
  if (lpr >= 32) x += dpp_f<kDppBcast15, 0xA>(0.0f, x);
  if (lpr >= 64) x += dpp_f<kDppBcast31, 0xC>(0.0f, x);
  return x;
}

// ---------------------------------------------------------------------------------------------------------------
// Split-precision lin_in on the f16 matrix pipe.
// Measured on gfx950 (tools/ubench/mfma_valu_overlap*.hip): v_mfma_f32_32x32x2_f32 occupies the SIMD for its full 64 cycles -- no
// VALU instruction of the same or of another wave issues underneath it (fp32 "MFMA" runs at, and instead of, the vector FMA rate) --
// whereas v_mfma_f32_32x32x16_f16 costs ~5 cycles when 8+ VALU instructions sit between two of them.  So the 36 sin/cos inputs of
// lin_in (values in [-1, 1]) go through the f16 pipe as  W.X = Wh.Xh + Wl.Xh + Wh.Xl  with  x = xh + xl, xh = f16_rne(x),
// xl = f16_rne(x - xh)  (two round-to-nearest halves carry 12 + 12 significand bits; the dropped Wl.Xl term is 2^-24 relative; fp32
// accumulation in the MFMA).  tools/ubench/f16split_gemm.hip: max error 3.8e-7 / rms 8e-8 against fp64 at K = 48, |D| ~ 2 -- slightly
// better than the fp32-input MFMA (6.1e-7 / 9.3e-8).  Weights are pre-split once per work-group and scaled by 2^S (S chosen from
// max |w| so that the low halves stay normal f16 numbers); everything else that enters the accumulators carries the same 2^S
// (exact), removed again after lin_out.  The raw inputs x, y, code use the spare k rows of the slices (bounded on this path: larger
// arguments take the exact routine); the bias row is the fp32 C operand of each accumulator tile's first MFMA.
// ---------------------------------------------------------------------------------------------------------------
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int C, int HD, int NB>
struct LdsH {  // in floats, placed behind Lds<C, HD, NB, true>
  static constexpr int HT = HD / 32;
  static constexpr int W_RAW = 0;                              // [4][HD] k-major rows x, y, code, bias -- times 2^S
  static constexpr int W_F16 = W_RAW + 4 * HD;                 // [term hi/lo][region 3][HT][64 lanes][8 halves = 4 dwords]
  static constexpr int TERM_STRIDE = 3 * HT * 64 * 4;
  static constexpr int BIAS = W_F16 + 2 * TERM_STRIDE;         // per block: b0 [HD], b1 [HD] -- times 2^S
  static constexpr int EMPTY = BIAS + NB * 2 * HD;             // projected empty feature -- times 2^S
  static constexpr int SCALE = EMPTY + HD;                     // [0] 2^S, [1] 2^-S, [2] max |w| (as int bits)
  // ResnetBlockFC linears on the f16 pipe (d_hidden = 32): per layer [term hi/lo][k-slice 2][64 lanes][8 halves] -- times 2^S.
  // k slot (slice s, lane half h, i) is the hidden row mfma_row(8 s + i, h): exactly the 8 accumulator values a lane holds for it,
  // so the C layout of one layer feeds the next layer's B operand from the lane's own registers.
  static constexpr int W_BLK = SCALE + 4;
  static constexpr int BLK_TERM_STRIDE = 2 * 64 * 4;
  static constexpr int BLK_LAYER_STRIDE = 2 * BLK_TERM_STRIDE;
  static constexpr int TOTAL = W_BLK + NB * 2 * BLK_LAYER_STRIDE;
};

// empty_proj: the projected empty feature [HD] (fp32, unscaled) as stage_weights left it in LDS
template <int C, int HD, int NB>
__device__ __forceinline__ void stage_weights_h(float* lh, const float* empty_proj, const float* __restrict__ mlp) {
  using LH = LdsH<C, HD, NB>;
  constexpr int HT = HD / 32;
  constexpr int D_IN = C + kPeDim;
  const MlpLayout ml{D_IN, HD, NB};
  int* mx = reinterpret_cast<int*>(lh + LH::SCALE + 2);
  if (threadIdx.x == 0) *mx = 0;
  __syncthreads();
  float m = 0.0f;
  for (int i = threadIdx.x; i < 39 * HD; i += blockDim.x) m = fmaxf(m, fabsf(mlp[ml.w_in() + (i % HD) * D_IN + C + i / HD]));  // x, y, code + 36 trig rows
  for (int i = threadIdx.x; i < NB * 2 * HD * HD; i += blockDim.x) {   // fc_0 / fc_1 weights share the scale (same f16 range)
    const int b = i / (2 * HD * HD), j = i % (2 * HD * HD);
    m = fmaxf(m, fabsf(mlp[(j < HD * HD ? ml.blk_w0(b) : ml.blk_w1(b)) + j % (HD * HD)]));
  }
  atomicMax(mx, __float_as_int(m));  // non-negative floats order like their bit patterns
  __syncthreads();
  const float wmax = __int_as_float(*mx);
  int ex = 0;
  if (wmax > 0.0f && wmax < 3.0e38f) frexpf(wmax, &ex);
  const int S = max(-40, min(40, 14 - ex));  // max |w| 2^S in [2^13, 2^14): far below the f16 limit, low halves normal down to |w| ~ 2^-13 max
  const float scale = ldexpf(1.0f, S);
  if (threadIdx.x == 0) lh[LH::SCALE] = scale, lh[LH::SCALE + 1] = ldexpf(1.0f, -S);
  for (int i = threadIdx.x; i < 4 * HD; i += blockDim.x) {
    const int k = i / HD, hid = i % HD;
    lh[LH::W_RAW + i] = (k < 3 ? mlp[ml.w_in() + hid * D_IN + C + k] : mlp[ml.b_in() + hid]) * scale;
  }
  _Float16* wf = reinterpret_cast<_Float16*>(lh + LH::W_F16);
  for (int i = threadIdx.x; i < 3 * HT * 64 * 8; i += blockDim.x) {
    const int e = i & 7, lane = (i >> 3) & 63, ht = (i >> 9) % HT, r = i / (HT * 512);
    const int slot = 8 * (lane >> 5) + e, hid = ht * 32 + (lane & 31);
    float w = 0.0f;
    if (slot < 12) w = mlp[ml.w_in() + hid * D_IN + C + 3 + 6 * (2 * r + slot / 6) + slot % 6] * scale;
    else if (r == 0 && slot < 14) w = mlp[ml.w_in() + hid * D_IN + C + (slot - 12)] * scale;   // spare rows of region 0: raw x, y
    else if (r == 1 && slot == 12) w = mlp[ml.w_in() + hid * D_IN + C + 2] * scale;             // spare row of region 1: raw depth code
    asm("" : "+v"(w));
    const _Float16 hi = (_Float16)w;
    wf[i] = hi;
    wf[i + LH::TERM_STRIDE * 2] = (_Float16)(w - (float)hi);  // TERM_STRIDE floats = 2 x halves
  }
  if constexpr (NB > 0) {
    static_assert(HD == 32, "f16 ResnetBlockFC layers are laid out for d_hidden = 32");
    _Float16* wb = reinterpret_cast<_Float16*>(lh + LH::W_BLK);
    for (int i = threadIdx.x; i < NB * 2 * 2 * 64 * 8; i += blockDim.x) {
      const int e = i & 7, lane = (i >> 3) & 63, sl = (i >> 9) & 1, layer = i >> 10;   // layer = 2 * block + {0: fc_0, 1: fc_1}
      const int kin = mfma_row(8 * sl + e, lane >> 5), out = lane & 31;
      float w = mlp[((layer & 1) ? ml.blk_w1(layer >> 1) : ml.blk_w0(layer >> 1)) + out * HD + kin] * scale;
      asm("" : "+v"(w));
      const _Float16 hi = (_Float16)w;
      _Float16* dst = wb + layer * LH::BLK_LAYER_STRIDE * 2 + (sl * 64 + lane) * 8 + e;
      dst[0] = hi;
      dst[LH::BLK_TERM_STRIDE * 2] = (_Float16)(w - (float)hi);
    }
  }
  for (int i = threadIdx.x; i < NB * 2 * HD; i += blockDim.x) {
    const int b = i / (2 * HD), j = i % (2 * HD);
    lh[LH::BIAS + i] = (j < HD ? mlp[ml.blk_b0(b) + j] : mlp[ml.blk_b1(b) + j - HD]) * scale;
  }
  for (int i = threadIdx.x; i < HD; i += blockDim.x) lh[LH::EMPTY + i] = empty_proj[i] * scale;
}

// The staged MLP of render_kernel_p as ONE block of floats: Lds<C, HD, NB, true> | pad to 16 bytes | LdsH<C, HD, NB>.  The evaluation frame's
// prep launch (bts_aux.hip: eval_prep_kernel) runs stage_weights / stage_weights_h once and writes the block to global memory; the
// frame's render launch copies it into LDS -- FLOATS / 4 coalesced 16-byte loads and one barrier per work-group instead of ~33 strided
// 4-byte loads per thread, a 64-term FMA chain and five barriers, 512 times per frame.  The same bits by construction.
template <int C, int HD, int NB>
struct MlpImage {
  static constexpr int LH_OFF = (Lds<C, HD, NB, true>::TOTAL + 3) & ~3;
  static constexpr int FLOATS = (LH_OFF + LdsH<C, HD, NB>::TOTAL + 3) & ~3;
  static constexpr int LDS_FLOATS = Lds<C, HD, NB, true>::TOTAL + LdsH<C, HD, NB>::TOTAL + 4;   // render_kernel_p's static array
  static_assert(FLOATS <= LDS_FLOATS, "the image is copied into render_kernel_p's array as whole float4");
};

// stage the MLP of render_kernel_p (fp32 part and split-f16 part) into `lds` from the packed parameter vector; ends with a barrier
template <int C, int HD, int NB>
__device__ __forceinline__ void stage_mlp(float* lds, const float* mlp, const float* empty) {
  stage_weights<C, HD, NB, true>(lds, mlp, empty);
  __syncthreads();
  stage_weights_h<C, HD, NB>(lds + MlpImage<C, HD, NB>::LH_OFF, lds + Lds<C, HD, NB, true>::EMPTY, mlp);
  __syncthreads();
}

__device__ __forceinline__ void swap32u(unsigned& a, unsigned& b) {
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0], b = r[1];
}
__device__ __forceinline__ unsigned pack_h2(_Float16 a, _Float16 b) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, (h2){a, b});
}
// The f16 split of TWO fp32 values, packed: hi = {f16_rne(e0), f16_rne(e1)}, lo = {f16_rne(e0 - hi0), f16_rne(e1 - hi1)} in THREE
// instructions -- v_cvt_pk_f16_f32, v_fma_mixlo_f16, v_fma_mixhi_f16 (the mixed-precision fma reads the f16 half in place and rounds the
// EXACT difference once: e - hi has at most 13 significant bits, so this is the very value f16(e - float(hi)) of the scalar form).
// Rounds 2 - 5 wrote hi = (_Float16)e; lo = (_Float16)(e - (float)hi) per value, which hipcc compiles to EIGHT instructions per pair (each
// hi converted twice, once alone for the way back to fp32 and once packed; two conversions back; two subtractions; the packed lo).
// `neg1` = -1.0f as an OPAQUE scalar (opaque_neg1()): with the literal the compiler rewrites fma(x, -1, e) as e - x and the mixed form is gone.
// e0, e1 must be opaque fp32 VALUES (see f16_region: a producer folded into one of the conversions is rounded differently there).
__device__ __forceinline__ float opaque_neg1() {
  float k = -1.0f;
  asm("" : "+s"(k));
  return k;
}
__device__ __forceinline__ void split2_f16(float e0, float e1, float neg1, unsigned& hi, unsigned& lo) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  const h2 hp = __builtin_convertvector((f2){e0, e1}, h2);
  h2 lp;
  lp[0] = (_Float16)__builtin_fmaf((float)hp[0], neg1, e0);
  lp[1] = (_Float16)__builtin_fmaf((float)hp[1], neg1, e1);
  hi = __builtin_bit_cast(unsigned, hp), lo = __builtin_bit_cast(unsigned, lp);
}

// 12 encoding entries (two octaves) of this lane's sample -> both point tiles' B operands (high and low halves) -> 12 f16 MFMAs
template <int HD, int NE = 12, bool FIRST = false>
__device__ __forceinline__ void f16_region(f32x16 (&acc)[HD / 32][2], const float* wf /* lane-resolved, this region */, int term_stride,
                                           const float (&e)[NE], const f32x16* bias = nullptr) {
  static_assert(NE >= 8 && NE <= 16, "one 16-row k-slice");
  constexpr int HT = HD / 32;
  // The entries as opaque fp32 VALUES.  Otherwise hipcc folds the producing fma / multiply into ONE of the two conversions of the split
  // (v_fma_mixlo_f16: a single rounding of the exact result) while the other goes through v_cvt_pk_f16_f32 of the rounded fp32
  // value; in the 2^-13 of cases where double rounding matters the MFMA operand hi and the hi inside lo then differ by one f16
  // ulp and hi + lo misses e by 5e-4 |e| (tools/ubench/f16_split_fusion.hip; seen as 1e-4 jumps of the MLP output).
  float ev[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ev[i] = i < NE ? e[i] : 0.0f;
    if (i < NE) asm("" : "+v"(ev[i]));
  }
  const float neg1 = opaque_neg1();
  unsigned ph[4], qh[4], pl[4], ql[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    split2_f16(ev[2 * j], ev[2 * j + 1], neg1, ph[j], pl[j]);
    if (8 + 2 * j < NE) split2_f16(ev[8 + 2 * j], ev[9 + 2 * j], neg1, qh[j], ql[j]);   // (an odd NE: entry NE is the constant 0, hi = lo = 0)
    else qh[j] = 0u, ql[j] = 0u;
    swap32u(ph[j], qh[j]);  // p*: point tile 0 (k 0-7 from its own lanes, k 8-15 from the partner half), q*: point tile 1
    swap32u(pl[j], ql[j]);
  }
  const h8 b0h = __builtin_bit_cast(h8, (u32x4){ph[0], ph[1], ph[2], ph[3]});
  const h8 b1h = __builtin_bit_cast(h8, (u32x4){qh[0], qh[1], qh[2], qh[3]});
  const h8 b0l = __builtin_bit_cast(h8, (u32x4){pl[0], pl[1], pl[2], pl[3]});
  const h8 b1l = __builtin_bit_cast(h8, (u32x4){ql[0], ql[1], ql[2], ql[3]});
  h8 ah[HT], al[HT];
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    ah[ht] = *reinterpret_cast<const h8*>(wf + ht * 256);
    al[ht] = *reinterpret_cast<const h8*>(wf + term_stride + ht * 256);
  }
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    // FIRST: the accumulators are born here, from the bias row (both point tiles share it)
    acc[ht][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ht], b0h, FIRST ? bias[ht] : acc[ht][0], 0, 0, 0);
    acc[ht][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ht], b1h, FIRST ? bias[ht] : acc[ht][1], 0, 0, 0);
  }
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    acc[ht][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ht], b0h, acc[ht][0], 0, 0, 0);
    acc[ht][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ht], b1h, acc[ht][1], 0, 0, 0);
  }
#pragma unroll
  for (int ht = 0; ht < HT; ++ht) {
    acc[ht][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ht], b0l, acc[ht][0], 0, 0, 0);
    acc[ht][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ht], b1l, acc[ht][1], 0, 0, 0);
  }
}

// out[pt] += (W 2^S) . relu(in[pt]) 2^-S for one ResnetBlockFC linear of width 32 on the f16 pipe (split precision, as lin_in):
// the lane's own 16 accumulator values of a point tile are the B operand of two 16-row k-slices -- no data movement between layers.
// `in` carries 2^S (like every accumulator of this path); it is unscaled on the way into f16 and the pre-scaled weights put 2^S back.
__device__ __forceinline__ void hidden_layer_h(f32x16 (&out)[1][2], const f32x16 (&in)[1][2], const float* wl /* lane-resolved, this layer */,
                                               int term_stride, float inv_scale) {
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const h8 ah = *reinterpret_cast<const h8*>(wl + sl * 256);
    const h8 al = *reinterpret_cast<const h8*>(wl + term_stride + sl * 256);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      float vc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        // relu, then back to the true magnitude; the upper clamp only keeps a (never observed) 6e4 activation from turning into inf
        const float v = __builtin_amdgcn_fmed3f(in[0][pt][8 * sl + i], 0.0f, 3.4028234663852886e38f) * inv_scale;
        vc[i] = fminf(v, 6.0e4f);
        asm("" : "+v"(vc[i]));   // opaque fp32 value: both conversions of the split must see the same rounding (see f16_region)
      }
      const float neg1 = opaque_neg1();
      unsigned uh[4], ul[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split2_f16(vc[2 * j], vc[2 * j + 1], neg1, uh[j], ul[j]);
      const h8 bh = __builtin_bit_cast(h8, (u32x4){uh[0], uh[1], uh[2], uh[3]});
      const h8 bl = __builtin_bit_cast(h8, (u32x4){ul[0], ul[1], ul[2], ul[3]});
      out[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, out[0][pt], 0, 0, 0);
      out[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, out[0][pt], 0, 0, 0);
      out[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, out[0][pt], 0, 0, 0);
    }
  }
}

// The octave chain of the three encoding regions (region R = octaves 2R, 2R + 1).  Direct evaluations (Cody-Waite + polynomials, ~26
// instructions per argument) at octaves 0 and 3 only; 1, 2 and 4, 5 by angle doubling (fl(v 2f) = 2 fl(v f) exactly; ~1e-7 absolute error
// per doubling, two in a row at most).  Rounds 1 - 2 evaluated directly at 0, 2, 4 with one doubling each: +69 instructions
// per ray.  `raw` = octave 2R on entry and octave 2R + 2 on exit; `pre` carries octave 3 from region 0 (where it is evaluated, a region
// ahead of its use like every direct evaluation) to region 1.
template <int R>
__device__ __forceinline__ void pe_second_octave(SinCos3& r1, const SinCos3& raw, const SinCos3& pre) {
  if constexpr (R == 1) r1 = pre;
  else pe_double(r1, raw);
}
template <int R>
__device__ __forceinline__ void pe_advance(SinCos3& raw, SinCos3& pre, const SinCos3& r1, const float (&v3)[3], float ff) {
  if constexpr (R + 1 < 3) {
    pe_double(raw, r1);                                   // octave 2R + 2 from octave 2R + 1
    if constexpr (R == 0) pe_direct(pre, v3, ff * 8.0f);  // octave 3
  }
}

constexpr int kGatherLdsPerWave = 3 * 4096 + 768;
// ---------------------------------------------------------------------------------------------------------------
// The gather of G through LDS.
//
// PMC and the per-view split of the eval frame say the forward is bound by the texture addresser for every ray that does NOT pass
// through the encoder camera (profiles/README.md, r02f): there each sample of a ray hits its own texels, lane (h, col) reads its 64
// bytes as four 16-byte loads, and every one of the 64 gather instructions of a ray presents 64 different cache lines to the L1
// tag pipeline (one per clock): 4 096 clocks per ray and CU, exactly the measured 6.4 ns per ray against 4.2 ns for encoder-camera
// rays (whose samples share their texels: one line per instruction).
// Here EIGHT ADJACENT LANES fetch one whole 128-byte row half (global_load_lds_dwordx4: 16 bytes per lane straight into LDS, no
// VGPRs): 8 lines per instruction instead of 64.  The hardware puts lane L's 16 bytes at M0 + 16 L, so the row of point 8j + m
// (instruction j of a block, m = L >> 3) lands at block + j * 1024 + m * 128; the pieces of row r = 8 j + m are fetched rotated by
// (r >> 1) & 7 = (4 j + (m >> 1)) & 7 so that the consumer -- lane (h, col) reading the four pieces 4h .. 4h + 3 of row col as
// ds_read_b128 -- spreads over all banks.  gfx950 serves a ds_read_b128 in four 16-lane groups, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
// and the same + 32 (MI355X_MICROARCH.md, LDS), 256 bytes = 16 slots of 16 bytes per cycle: a group's eight even rows need eight different
// rotations, and so do its eight odd rows (slot = 8 (r & 1) + ((piece - rot) & 7)).  (r >> 1) & 7 is a bijection on each of those sets;
// rounds 2 - 5 rotated by (r & 7) >> 1, which pairs rows 0-3 with 24-27 and 12-15 with 20-23: every read took two cycles per group
// -- SQ_LDS_BANK_CONFLICT 62.9 M cycles per eval frame = 64 reads x 4 extra cycles x 245 760 rays, profiles/r05m/traffic_fwd_def.json.)
// A block = one tap of one (point tile, hidden tile) = 32 rows = 4 KB; a ring of three blocks per wave; block T + 3 is issued into
// the slot of block T once T has been blended.  The tap offsets of the 64 samples go through a 768-byte per-wave table (lane = sample
// writes, lane (m, piece) reads the row of sample 32 pt + 8 j + m).  52 KB of dynamic LDS per work-group on top of the weights: two
// work-groups per CU still fit for every shape (the RE10K model's 29 KB of weights included).
struct GatherLds {
  const char* ring;     // this wave's ring (3 blocks of 4 KB), generic pointer
  unsigned ring_m0;     // ... as an LDS byte address (M0 of the DMA loads)
  unsigned* tab;        // this wave's tap table: [64 samples][3] byte offsets into G of the taps nw, ne, sw
  unsigned rd[4];       // byte offset inside a block of this lane's piece q as the CONSUMER (h, col)
  unsigned piece16;     // 16 * the piece this lane FETCHES in the EVEN instructions of a block: ((L & 7) + (L >> 4)) & 7, i.e. rotated by m >> 1, m = L >> 3
  unsigned piece16x;    // ... in the ODD instructions (rows 8 .. 15, 24 .. 31): rotated by 4 more = piece16 ^ 64
  int m;                // L >> 3
};
// lane = sample writes its row of the tap table: byte offsets into G of three taps, o11 = o10 + (o01 - o00) (gl_offsets).  The caller
// fences the wave's LDS traffic on both sides.
template <int HD>
__device__ __forceinline__ void gl_write_taps(const GatherLds& gl, const Taps& tp, int lane) {
  gl.tab[lane * 3 + 0] = (unsigned)tp.o00 * (HD * 4u), gl.tab[lane * 3 + 1] = (unsigned)tp.o01 * (HD * 4u), gl.tab[lane * 3 + 2] = (unsigned)tp.o10 * (HD * 4u);
}
template <int HD, int T>
struct GBlock {   // block T of a ray: tap T % 2 of tap pair (T / 2) % 2 of hidden tile ht of point tile pt, in the order they are blended
  static constexpr int HT = HD / 32;
  static constexpr int S = T / 2, pt = S / (2 * HT), ht = (S / 2) % HT, tap = 2 * (S % 2) + T % 2, slot = T % 3;
  static constexpr int NBLK = 8 * HT;
};
// The four per-lane byte offsets (instructions j = 0..3) of block T.  The instruction offset of an LDS-DMA load is added to the global
// AND to the LDS address; j's 1 KB step inside the block therefore rides in the INSTRUCTION (one M0 per block instead of one per load:
// s_mov m0 + its wait state + the scalar add were 192 of the ~2 600 instructions a wave issues per ray) and is taken back out of the
// global side here: offsets are relative to G - kGlBias (gl_issue passes that base), + kGlBias - 1024 j >= 0.
constexpr unsigned kGlBias = 3 * 1024;
template <int HD, int T>
__device__ __forceinline__ void gl_offsets(const GatherLds& c, unsigned (&off)[4]) {
  using B = GBlock<HD, T>;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned* row = c.tab + (32 * B::pt + 8 * j + c.m) * 3;   // [o00, o01, o10]; o11 = o10 + (o01 - o00) (clamped taps included)
    off[j] = (B::tap < 3 ? row[B::tap] : row[2] + row[1] - row[0]) + ((j & 1 ? c.piece16x : c.piece16) + kGlBias - 1024u * j);
  }
}
// The PINNED kernels' form of the table lookup (render_kernel_p: the only kernels with the registers for it, the unpinned two-loop
// sibling sits at 256 VGPRs).  gl_offsets<HD, T> reads the lane's rows 8 j + m of point tile pt again for every block T, and each read is
// a full LDS round trip in the step's serial chain (table read -> wait -> add -> next read); but the rows depend on (pt, j) alone -- the
// tap is a choice among their three dwords, the hidden tile an instruction offset.  Here the lane reads its 4 x 3 dwords of a point
// tile ONCE, back to back, and forms every block's offsets from registers with the same integer expression: the same numbers, 2 x 12
// dword lookups per ray instead of 64 and no table wait in the step (profiles/r22a).
struct GTapRegs {
  unsigned t[2][4][3];   // [point tile][j][o00, o01, o10] of table row 32 pt + 8 j + m
};
template <int PT>
__device__ __forceinline__ void gl_read_taps(const GatherLds& c, GTapRegs& t) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) t.t[PT][j][i] = c.tab[(32 * PT + 8 * j + c.m) * 3 + i];
}
template <int HD, int T>
__device__ __forceinline__ void gl_offsets_r(const GatherLds& c, const GTapRegs& t, unsigned (&off)[4]) {
  using B = GBlock<HD, T>;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned (&row)[3] = t.t[B::pt][j];
    off[j] = (B::tap < 3 ? row[B::tap] : row[2] + row[1] - row[0]) + ((j & 1 ? c.piece16x : c.piece16) + kGlBias - 1024u * j);
  }
}
// the step whose offsets (block T + 4) are the last of point tile 0: tile 1's rows are read behind them, in front of the step's row
// request -- LDS returns in order per wave, so they have landed when the next step's blend has its rows, a whole step before their
// first use, and tile 0's registers are free by then.  (HD = 32: block 4 is tile 1 already, both tiles are read in the prologue.)
template <int HD>
constexpr int kTapsStep = GBlock<HD, 0>::NBLK / 2 - 5;
// what the overwrite of a slot must wait for: one value computed from EACH of the four row pieces (ds_read_b128) of the block that
// lived there.  See gl_issue.
struct GDep {
  float d[4];
};
template <int HD, int T>
__device__ __forceinline__ void gl_issue(const GatherLds& c, const float4* G, const unsigned (&off)[4], const GDep& dep) {
  using B = GBlock<HD, T>;
  // `dep`: the DMA write into LDS does not queue behind this wave's ds_reads -- a ds_read_b128 of the slot's previous block that is
  // still waiting in the LDS queue when the new rows arrive returns the NEW rows (seen on the RE10K shapes, where eight waves'
  // weight reads keep the queue hundreds of cycles deep: a handful of rays per frame differed from run to run, r03i / r03j).  The
  // memory clobber orders only the ISSUE of those reads, so the issue takes one input computed from each of the four pieces: the
  // compiler has to wait for all four reads to RETURN before the first load of the block goes out.  (One value of the last piece
  // is not enough: the scheduler reorders the four reads and sinks the blend of the others below the loads.)
  // M0 = the slot's LDS address minus the hidden tile's share of the instruction offset (ht * 128: that part belongs to the global
  // address only); the loads' instruction offsets ht * 128 + j * 1024 then place row group j at slot + j * 1024.
  const unsigned m0v = c.ring_m0 + B::slot * 4096 - B::ht * 128;
  const char* Gb = reinterpret_cast<const char*>(G) - kGlBias;
  asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %0, %5 offset:%6\n\t"
               "global_load_lds_dwordx4 %1, %5 offset:%7\n\t"
               "global_load_lds_dwordx4 %2, %5 offset:%8\n\t"
               "global_load_lds_dwordx4 %3, %5 offset:%9"
               :: "v"(off[0]), "v"(off[1]), "v"(off[2]), "v"(off[3]), "s"(m0v), "s"(Gb), "n"(B::ht * 128), "n"(B::ht * 128 + 1024),
                  "n"(B::ht * 128 + 2048), "n"(B::ht * 128 + 3072), "v"(dep.d[0]), "v"(dep.d[1]), "v"(dep.d[2]), "v"(dep.d[3])
               : "memory", "m0");
}
struct GRows {
  float4 v[2][4];   // the lane's four 16-byte pieces of two blocks (even / odd T)
};
// wait until block T has landed, read this lane's pieces.  ISSUED = blocks issued after T at this point of the schedule
template <int HD, int T, int ISSUED>
__device__ __forceinline__ void gl_fetch(const GatherLds& c, GRows& r) {
  using B = GBlock<HD, T>;
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * ISSUED) : "memory");
#pragma unroll
  for (int q = 0; q < 4; ++q) r.v[T & 1][q] = *reinterpret_cast<const float4*>(c.ring + B::slot * 4096 + c.rd[q]);
}
// one step: block T (its rows requested from LDS one step ago) is blended (acc += w_tap * row, the order of gblend), block T + 3 goes
// out into T's slot, the offsets of block T + 4 are fetched from the table, and the rows of block T + 1 are requested from LDS -- last,
// when block T + 1 has had the whole step to land (two blocks may still be in flight behind it).  -DBTS_GL_FETCH_EARLY requests them
// first instead (rounds 1 - 2 shipped that order; 3 % slower on the eval frame, profiles/r03_experiments/r03k).
// PIN (the PINNED kernels): the offsets come from `taps` (GTapRegs above).
template <int HD, int T, bool PIN = false>
__device__ __forceinline__ void gl_consume(f32x16 (&acc)[HD / 32][2], const GatherLds& c, GRows& r, const float4* G, const float (&w)[2][4],
                                           unsigned (&off_next)[4], GTapRegs* taps = nullptr) {
  using B = GBlock<HD, T>;
#ifdef BTS_GL_FETCH_EARLY
  if constexpr (T + 1 < B::NBLK) gl_fetch<HD, T + 1, (T + 2 < B::NBLK ? 1 : 0)>(c, r);   // issued so far: blocks 0 .. T + 2
#endif
  const f32x2 wv = {w[B::pt][B::tap], w[B::pt][B::tap]};
  f32x16& a = acc[B::ht][B::pt];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const float* x = reinterpret_cast<const float*>(&r.v[T & 1][q]) + e;
      const f32x2 xv = {x[0], x[1]};
      const f32x2 res = __builtin_elementwise_fma(xv, wv, (f32x2){a[4 * q + e], a[4 * q + e + 1]});
      a[4 * q + e] = res[0], a[4 * q + e + 1] = res[1];
    }
  }
  if constexpr (T + 3 < B::NBLK) {
    gl_issue<HD, T + 3>(c, G, off_next, GDep{{a[3], a[7], a[11], a[15]}});
    if constexpr (PIN) {
      if constexpr (T + 4 < B::NBLK) gl_offsets_r<HD, T + 4>(c, *taps, off_next);
      // (the table is not written before the next ray's fences, and these reads are waited for long before: no new hazard)
      if constexpr (T == kTapsStep<HD>) gl_read_taps<1>(c, *taps);
    } else {
      if constexpr (T + 4 < B::NBLK) gl_offsets<HD, T + 4>(c, off_next);
    }
  }
#ifndef BTS_GL_FETCH_EARLY
  if constexpr (T + 1 < B::NBLK) gl_fetch<HD, T + 1, (T + 3 < B::NBLK ? 2 : (T + 2 < B::NBLK ? 1 : 0))>(c, r);   // issued: blocks 0 .. T + 3
#endif
}
// start of a ray: table written and fenced by the caller; blocks 0, 1, 2 go out, block 0 is requested from LDS, the offsets of block 3
// wait in off_next
template <int HD, bool PIN = false>
__device__ __forceinline__ void gl_prologue(const GatherLds& c, GRows& r, const float4* G, unsigned (&off_next)[4], GTapRegs* taps = nullptr) {
  unsigned o0[4], o1[4], o2[4];
  if constexpr (PIN) {
    // the lane's twelve dwords of point tile 0, back to back, in front of the one wait below.  They are read after the caller's fences
    // behind this ray's table write and waited for before anything else of the ray: the next ray's table write cannot overtake them.
    gl_read_taps<0>(c, *taps);
    if constexpr (kTapsStep<HD> < 0) gl_read_taps<1>(c, *taps);
    gl_offsets_r<HD, 0>(c, *taps, o0), gl_offsets_r<HD, 1>(c, *taps, o1), gl_offsets_r<HD, 2>(c, *taps, o2);
  } else {
    gl_offsets<HD, 0>(c, o0), gl_offsets<HD, 1>(c, o1), gl_offsets<HD, 2>(c, o2);
  }
  // nothing of the previous ray may still be queued in LDS when its slots are overwritten (gl_issue): the table reads above need the
  // wait anyway, LDS returns in order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const GDep none = {{0.0f, 0.0f, 0.0f, 0.0f}};
  gl_issue<HD, 0>(c, G, o0, none), gl_issue<HD, 1>(c, G, o1, none), gl_issue<HD, 2>(c, G, o2, none);
  if constexpr (PIN) gl_offsets_r<HD, 3>(c, *taps, off_next);
  else gl_offsets<HD, 3>(c, off_next);
}
// ---------------------------------------------------------------------------------------------------------------
// Rays whose samples share their texels (render_kernel_p's second loop).  A ray that starts at the encoder camera's centre projects
// every sample onto the same pixel: its 64 samples fetch the same four rows of G, 1 KB, sixty-four times through the ring above.
// Here the wave fetches them ONCE -- one global_load_lds_dwordx4, lane L the 16-byte piece L % (HD / 4) of tap L / (HD / 4) -- into
// the first KB of its ring: the IMAGE, tap t at t * HD * 4.  Block T is then blended where gl_consume<HD, T> blends it, with the same
// eight packed FMAs and each sample's own weight; lane (h, col) reads the pieces 4h .. 4h + 3 of half-row ht of the tap from the
// image, the same address for every col (a broadcast).  No ring, no tap table, no per-block wait: only the source of the rows differs
// from the general path, so the results are the same bits.
// u00, u01, u10: byte offsets into G of the ray's taps (wave-uniform); o11 = o10 + (o01 - o00) as in gl_offsets.
template <int HD>
__device__ __forceinline__ void gs_issue(const GatherLds& c, const float4* G, unsigned u00, unsigned u01, unsigned u10, int lane) {
  constexpr int PPR = HD / 4;   // 16-byte pieces per row (HD = 32: lanes 32 - 63 fetch the four rows again, behind the image)
  const unsigned u11 = u10 + u01 - u00;
  const int t = (lane / PPR) & 3;
  const unsigned off = (t == 0 ? u00 : (t == 1 ? u01 : (t == 2 ? u10 : u11))) + 16u * (unsigned)(lane % PPR);
  // nothing of the previous ray (its image reads, or the ring reads of a ray of the general loop) may still be queued in LDS when
  // the image is overwritten: the DMA write does not queue behind this wave's ds_reads (gl_issue).  LDS returns in order.
  asm volatile("s_waitcnt lgkmcnt(0)\n\t"
               "s_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %0, %2"
               :: "v"(off), "s"(c.ring_m0), "s"(G)
               : "memory", "m0");
}
// this lane's four pieces of block T out of the image.  (Blocks T and T + 8 read the same bytes for the two point tiles: the empty
// asm keeps the compiler from holding the first tile's rows in registers until the second tile's turn.)
template <int HD, int T>
__device__ __forceinline__ void gs_fetch(const GatherLds& c, GRows& r, int h) {
  using B = GBlock<HD, T>;
  asm volatile("" ::: "memory");
  const char* src = c.ring + B::tap * (HD * 4) + B::ht * 128 + h * 64;
#pragma unroll
  for (int q = 0; q < 4; ++q) r.v[T & 1][q] = *reinterpret_cast<const float4*>(src + 16 * q);
}
// the ONE wait of a shared ray (the image has landed), then block 0's rows
template <int HD>
__device__ __forceinline__ void gs_first(const GatherLds& c, GRows& r, int h) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  gs_fetch<HD, 0>(c, r, h);
}
// gl_consume's step for a shared ray: blend block T (the same arithmetic in the same order), request the rows of block T + 1.
// (Requested here, the four reads end up directly in front of their first FMA and the two halves of GRows::v fold into one.  Requesting
// them in front of the blend, held there by an empty asm over block T's rows, hides that round trip under the eight packed FMAs -- and
// gains nothing measurable on its own, the partner wave covers it already: profiles/r22a, not kept.)
template <int HD, int T>
__device__ __forceinline__ void gs_consume(f32x16 (&acc)[HD / 32][2], const GatherLds& c, GRows& r, const float (&w)[2][4], int h) {
  using B = GBlock<HD, T>;
  const f32x2 wv = {w[B::pt][B::tap], w[B::pt][B::tap]};
  f32x16& a = acc[B::ht][B::pt];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const float* x = reinterpret_cast<const float*>(&r.v[T & 1][q]) + e;
      const f32x2 xv = {x[0], x[1]};
      const f32x2 res = __builtin_elementwise_fma(xv, wv, (f32x2){a[4 * q + e], a[4 * q + e + 1]});
      a[4 * q + e] = res[0], a[4 * q + e + 1] = res[1];
    }
  }
  if constexpr (T + 1 < B::NBLK) gs_fetch<HD, T + 1>(c, r, h);
}
// one step of either kind (SH: the ray shares its texels; PIN: the PINNED kernels' general step, offsets from `taps`)
template <int HD, int T, bool SH, bool PIN = false>
__device__ __forceinline__ void g_step(f32x16 (&acc)[HD / 32][2], const GatherLds& c, GRows& r, const float4* G, const float (&w)[2][4],
                                       unsigned (&off_next)[4], int h, GTapRegs* taps = nullptr) {
  if constexpr (SH) gs_consume<HD, T>(acc, c, r, w, h);
  else gl_consume<HD, T, PIN>(acc, c, r, G, w, off_next, taps);
}

// Region R = octaves 2R (sines computed directly, one region ahead) and 2R + 1 (by angle doubling); the gather blocks 4R .. 4R + 3 are
// blended behind the region's MFMAs.  The regions are not fenced from each other: the scheduler may pull the next region's
// trigonometry under this region's MFMAs.
template <int HD, int R, bool SH = false, bool PIN = false>
__device__ __forceinline__ void region_seq_li(f32x16 (&acc)[HD / 32][2], const GatherLds& gl, GRows& rows, const float4* __restrict__ G,
                                              const float (&wq)[2][4], unsigned (&off_next)[4], const float* wf, int term_stride, SinCos3& raw,
                                              SinCos3& pre, const float (&v3)[3], float ff, const f32x16* bias, int h = 0, GTapRegs* taps = nullptr) {
  constexpr int HT = HD / 32;
  constexpr int NS = 4 * HT;
  if constexpr (R < 3) {
    constexpr int NE = R == 0 ? 14 : (R == 1 ? 13 : 12);
    float e[NE];
    float t[6];
    pe_entries(t, raw, v3, ff);
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = t[i];
    SinCos3 r1;
    pe_second_octave<R>(r1, raw, pre);
    pe_entries(t, r1, v3, ff * 2.0f);
#pragma unroll
    for (int i = 0; i < 6; ++i) e[6 + i] = t[i];
    if constexpr (R == 0) e[12] = v3[0], e[13] = v3[1];
    if constexpr (R == 1) e[12] = v3[2];
    pe_advance<R>(raw, pre, r1, v3, ff);
    f16_region<HD, NE, R == 0>(acc, wf + R * HT * 256, term_stride, e, bias);
    if constexpr (2 * R < NS) {
      if constexpr (R == 0) {
        if constexpr (SH) gs_first<HD>(gl, rows, h);
        else gl_fetch<HD, 0, 2>(gl, rows);   // blocks 1, 2 were issued after block 0
      }
      g_step<HD, 4 * R + 0, SH, PIN>(acc, gl, rows, G, wq, off_next, h, taps);
      g_step<HD, 4 * R + 1, SH, PIN>(acc, gl, rows, G, wq, off_next, h, taps);
      g_step<HD, 4 * R + 2, SH, PIN>(acc, gl, rows, G, wq, off_next, h, taps);
      g_step<HD, 4 * R + 3, SH, PIN>(acc, gl, rows, G, wq, off_next, h, taps);
    }
    region_seq_li<HD, R + 1, SH, PIN>(acc, gl, rows, G, wq, off_next, wf, term_stride, raw, pre, v3, ff * 4.0f, bias, h, taps);
  }
}
template <int HD, int R, bool SH = false, bool PIN = false>
__device__ __forceinline__ void region_seq_l(f32x16 (&acc)[HD / 32][2], const GatherLds& gl, GRows& rows, const float4* __restrict__ G,
                                             const float (&wq)[2][4], unsigned (&off_next)[4], const float* wf, int term_stride, SinCos3& raw,
                                             const float (&v3)[3], float ff, const f32x16* bias, int h = 0, GTapRegs* taps = nullptr) {
  static_assert(R == 0, "entered at region 0");
  SinCos3 pre;
  region_seq_li<HD, 0, SH, PIN>(acc, gl, rows, G, wq, off_next, wf, term_stride, raw, pre, v3, ff, bias, h, taps);
}

// Cold path: a wave in which some sample's encoding argument leaves the fast sincos range (|arg| > 1e5: points within millimetres
// of the encoder's camera plane) evaluates that iteration with the compact lane = point routine (libm range reduction inside).
// Kept out of line -- inlining 36 libm sines next to the pipelined path costs ~240 spilled VGPRs on the HOT path.
template <int C, int HD, int NB>
__device__ __attribute__((noinline)) float eval_point_exact(const float* lds, const float4* G, const float* w2c, const float* Kc, int H, int W,
                                                            int fs, int code_mode, int inv_z, float inv_dmax, float inv_range, float d_min, float range,
                                                            float freq_factor, int learn_empty, float b_out, float px, float py, float pz) {
  FwdParams q;
  q.H = H, q.W = W, q.fs = fs, q.code_mode = code_mode, q.inv_z = inv_z, q.inv_dmax = inv_dmax, q.inv_range = inv_range, q.d_min = d_min;
  q.range = range, q.freq_factor = freq_factor, q.learn_empty = learn_empty, q.ablate = 0;
  const Cam enc = load_cam(w2c, Kc);
  Proj pe;
  return eval_point<C, HD, NB, true>(q, lds, enc, G, (int)(threadIdx.x & 63), b_out, px, py, pz, pe);
}

// What the top of an iteration of the persistent kernels needs of the kernel parameters (cameras, ray, sample positions, projection,
// depth code).  With PIN they are fetched from the kernarg segment in ONE batch (the empty asm takes every member as an
// operand, so the compiler has to issue all the scalar loads in front of it and waits once) instead of in ten dependent round trips;
// measured, that loses (below), so the product reads them where they are used like every other parameter.
template <bool PIN>
struct IterHeadT {
  const float* w2c_enc;
  const float* K_enc;
  const float* proj;
  const float* rays;
  const float* z_samp;
  const float* jitter;
  int K, H, W, nv, fs, code_mode, inv_z, learn_empty;
  float inv_dmax, inv_range, d_min, range, freq_factor;
  template <typename Q>
  __device__ __forceinline__ explicit IterHeadT(Q q) {
    const FwdParams __attribute__((address_space(4)))* f = head_of(q);
    w2c_enc = f->w2c_enc, K_enc = f->K_enc, proj = f->proj, rays = f->rays, z_samp = f->z_samp, jitter = f->jitter;
    K = f->K, H = f->H, W = f->W, nv = f->nv, fs = f->fs, code_mode = f->code_mode, inv_z = f->inv_z, learn_empty = f->learn_empty;
    inv_dmax = f->inv_dmax, inv_range = f->inv_range, d_min = f->d_min, range = f->range, freq_factor = f->freq_factor;
    // A/B (profiles/r03_experiments/r03q): with the pin the FORWARD is 1.5 % slower -- the second wave of the SIMD hides the scalar round trips, and
    // the 22 more spilled SGPRs are VALU instructions in a VALU-bound loop.  Without it this struct is only a list of names: the
    // compiler sinks every load to its use.  The backward's pass A is the other way round (it waits, it does not issue): PIN = true.
    if constexpr (PIN)
    asm volatile("" : "+s"(w2c_enc), "+s"(K_enc), "+s"(proj), "+s"(rays), "+s"(z_samp), "+s"(K), "+s"(H), "+s"(W), "+s"(nv), "+s"(fs),
                 "+s"(code_mode), "+s"(inv_z), "+s"(learn_empty), "+s"(inv_dmax), "+s"(inv_range), "+s"(d_min), "+s"(range), "+s"(freq_factor));
  }
  // the FwdParams at the head of the parameter block: the block itself (forward) or its first member (backward / query blocks)
  static __device__ __forceinline__ const FwdParams __attribute__((address_space(4)))* head_of(const FwdParams __attribute__((address_space(4)))* q) { return q; }
  template <typename B>
  static __device__ __forceinline__ const FwdParams __attribute__((address_space(4)))* head_of(const B __attribute__((address_space(4)))* q) { return &q->f; }
};
using IterHead = IterHeadT<false>;

// one 16-byte store through either kind of output pointer of render_kernel_p (generic, or global: PINNED)
__device__ __forceinline__ void store4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void store4(float __attribute__((address_space(1)))* p, const float4& v) {
  *(f32x4 __attribute__((address_space(1)))*)p = (f32x4){v.x, v.y, v.z, v.w};
}

// EPI: also reduce weights * invalid and max invalid over each ray's samples (BtsRenderArgs.invalid_wsum / invalid_any).  A template
// parameter, not a run-time test: the evaluation instantiations carry no trace of it (16 more spilled SGPRs otherwise).
// DYN: the groups behind FwdParams::dyn_first are not on the waves' lists, they are claimed from the counter FwdParams::sched (below:
// "Work distribution").  Built for the evaluation frame's kernels only; every other instantiation carries no trace of it.
// IMG: the preheader copies the staged MLP from FwdParams::mlp_image instead of staging it (MlpImage above).  A template parameter like
// DYN, and for the same reason: the instantiations without it are, instruction for instruction, the kernels they were -- a run-time
// test in the preheader re-colours the registers of the whole per-ray loop.  Built for the evaluation frame's kernels (no loss epilogue,
// at most two render views); a launch with an image and no such instantiation stages in place.
// PINNED: the switches of PinnedSet (bts_field_kernel.h) are compile-time constants -- BTS_PIN(constant, field) below is the constant here
// and the field everywhere else -- so their scalar loads from the kernarg segment, their branches and the registers both hold are not
// in the kernel, and the five arrays it writes are global pointers.  The same arithmetic in the same order: only tests whose outcome the
// set fixes go away.  One more form of the evaluation frame's DYN + IMG kernel with one render view; like DYN and IMG it leaves no trace
// in any other instantiation.
#define BTS_PIN(constant, field) (PINNED ? (constant) : (field))
template <int C, int HD, int NB, int NVMAX, bool ONE_RAY, bool F16, bool EPI = false, bool DYN = false, bool IMG = false, bool PINNED = false>
__global__ __launch_bounds__(256, kFwdWaves) void render_kernel_p(const FwdParams p) {
  static_assert(F16, "lin_in runs on the f16 matrix pipe in split precision: the fp32-input-MFMA form of rounds 1 - 2 is gone (git history)");
  static_assert(!PINNED || (ONE_RAY && !EPI && DYN && IMG && NB == 0 && NVMAX == PinnedSet::nv), "the pinned set is the evaluation frame's");
  using OutP = std::conditional_t<PINNED, float __attribute__((address_space(1)))*, float*>;   // the arrays the iteration writes
  using L = Lds<C, HD, NB, true>;
  using LH = LdsH<C, HD, NB>;
  constexpr int HT = HD / 32;
  constexpr int NS = 4 * HT;
  __shared__ __attribute__((aligned(16))) float lds[L::TOTAL + LH::TOTAL + 4];
  float* const lh = lds + ((L::TOTAL + 3) & ~3);  // 16-byte aligned: the f16 A operands are read as ds_read_b128
#ifdef BTS_PROBE
  const unsigned long long t_entry = __builtin_readcyclecounter();
#endif
  if constexpr (IMG) {
    // the staged MLP ready-made (MlpImage: the prep launch of bts_eval_frame_prep ran the two routines below once for the frame)
    const float4* src = reinterpret_cast<const float4*>(p.mlp_image);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < MlpImage<C, HD, NB>::FLOATS / 4; i += 256) dst[i] = src[i];
    __syncthreads();
  } else {
    stage_weights<C, HD, NB, true>(lds, p.mlp, p.empty_feature);
    __syncthreads();
    stage_weights_h<C, HD, NB>(lh, lds + L::EMPTY, p.mlp);
    __syncthreads();
  }
#ifdef BTS_PROBE
  // the preheader: kernel entry to the barrier behind the staged (or copied) MLP, per wave (tools/section_probe.py --lifetimes folds the
  // waves of a work-group); 16 bits of cycles, saturated, above XCC_ID in the last counter word -- exact through the tools' float64 tables
  const unsigned long long t_stage = __builtin_readcyclecounter() - t_entry;
#endif
  // 2^S carried by the accumulators
  const float scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lh[LH::SCALE])));
  const float inv_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lh[LH::SCALE + 1])));

  const int lane = threadIdx.x & 63;
  const int h0 = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  extern __shared__ __attribute__((aligned(128))) char gather_lds[];   // per wave: ring of 3 x 4 KB + 768 B tap table
  GatherLds gl;
  {
    char* base = gather_lds + wave * kGatherLdsPerWave;
    gl.ring = base;
    gl.ring_m0 = (unsigned)(unsigned long)base;     // low 32 bits of a generic LDS address = the LDS byte address
    gl.tab = reinterpret_cast<unsigned*>(base + 3 * 4096);
    gl.m = lane >> 3;
    gl.piece16 = 16u * (unsigned)(((lane & 7) + (lane >> 4)) & 7);
    gl.piece16x = gl.piece16 ^ 64u;
    const int col = lane & 31;
#pragma unroll
    for (int q = 0; q < 4; ++q) gl.rd[q] = (unsigned)(col * 128 + ((4 * h0 + q - (col >> 1)) & 7) * 16);
  }
  const int nwg = gridDim.x;  // multiple of 8
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int wg_per_xcd = nwg >> 3;
  const int xcd = wg / wg_per_xcd;
  const int lw = (wg - xcd * wg_per_xcd) * 4 + wave;  // wave index inside its XCD
  const int waves_per_xcd = wg_per_xcd * 4;
  // 48-lane mode (render_geometry: 32 < K <= 48 and the rays of a batch element a multiple of four -- exp_re10k.yaml's n_coarse = 48):
  // a wave takes FOUR rays in THREE iterations -- lanes 0-47 one whole ray per iteration, lanes 48-63 one 16-sample row of the
  // fourth -- instead of idling a quarter of its lanes on every instruction.  The fourth ray's transmittance and partial sums cross
  // the three iterations (the chunk loop below, reused); everything per sample is lane-local anyway.
  const int lpr = ONE_RAY ? 64 : p.lpr;
  const bool pk48 = !ONE_RAY && lpr == 48;
  const bool mainl = lane < 48;
  const int R = pk48 ? 4 : 64 / lpr;   // rays per group
  const int kl = pk48 ? (mainl ? lane : lane - 48) : lane & (lpr - 1);
  auto lane_ray = [&](int gg, int it) -> long { return pk48 ? (long)gg * 4 + (mainl ? it : 3) : (long)gg * R + lane / lpr; };
  auto lane_k = [&](int it) -> int { return pk48 && !mainl ? 16 * it + kl : kl; };
  // Work distribution.  Ray groups are cut into chunks of 2^chunk_log2 consecutive groups; chunk c belongs to XCD c % 8, and the
  // waves of an XCD walk its chunks in order (consecutive waves = consecutive rays, so the texel footprints of the waves resident
  // on an XCD still overlap in its L2).  Round 1 gave every XCD ONE contiguous eighth of the rays: with the two stereo views of
  // eval_depth in one launch, XCDs 0-3 got the encoder camera's own rays (0.56 ms for all of them alone) and XCDs 4-7 the partner's
  // (0.86 ms alone) -- the launch took 1.69 ms, the slower half's 2 x 0.86, instead of 1.42.
  const int CHL = p.chunk_log2;
  // (group indices fit 32 bits -- render_fwd_impl refuses more than 2^31 - 2^20 groups: 64-bit scalar arithmetic here was ~120 SALU
  // instructions per iteration)
  const int n_groups = (int)p.groups;
  const int n_chunks = (n_groups + (1 << CHL) - 1) >> CHL;
  auto group_of = [&](int idx) -> int {   // idx-th group of this XCD's chunk list, or -1 past the end
    const int c = ((idx >> CHL) << 3) + xcd;
    const int gg = (c << CHL) + (idx & ((1 << CHL) - 1));
    return (c < n_chunks && gg < n_groups) ? gg : -1;
  };
  const int Bp = p.Bp;
  const float b_out = as_const(p.mlp)[MlpLayout{C + kPeDim, HD, NB}.b_out()];
  const int lane_off0 = h0 * HD + (lane & 31);

#ifdef BTS_PROBE
  unsigned long long t_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last = __builtin_readcyclecounter();
  const unsigned long long t_begin = t_last;
  // where the wave runs (tools/section_probe.py --lifetimes: per-XCD and per-CU lifetimes): XCC_ID << 32 | HW_ID
  unsigned hw_id = 0, xcc_id = 0;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc_id));
#endif
  const int groups_per_sample = Bp / R;   // Bp % R == 0 (render_geometry)
  int sample_end = groups_per_sample;
  int sample = 0;
  int idx = lw;
  int g = group_of(idx);
  // DYN: a static part and a claimed tail.  Groups [0, dyn_first) -- whole chunks on every XCD, positions [0, dyn_first / 8) of its
  // chunk list -- are walked as above; when a wave's list runs out it takes tickets from its XCD's counter sched[32 * xcd]: ticket t is
  // position dyn_first / 8 + t of the XCD's chunk list, a position past the list's end ends the wave.  (A persistent launch lasts as
  // long as its slowest wave, and on equal lists the two waves of a SIMD finish a fifth of the launch apart: profiles/r15a.)  One
  // counter per XCD, each on a cache line of its own, not one for the chip: 2 048 waves' claims on ONE line serialise at 11.5 ns each
  // (profiles/r05n), three times the 3.5 ns in which the chip finishes a ray -- measured, a chip-wide counter, and eight counters in
  // one line alike, made the launch 10 - 30 % longer (profiles/r15a/fraction.txt) -- and the imbalance is inside every CU, the XCDs'
  // sums are equal to half a percent; the tail keeps the static part's locality in L2.
  // The iteration prefetches its successor's ray record and jitter row, so the group of iteration i + 1 has to be known at the top
  // of iteration i: its ticket is drawn at the top of iteration i - 1 (`pend`, one lane's atomicAdd, the one VGPR this costs across
  // the back-edge) and read a whole iteration later, where the prefetched record is waited for anyway.
  // g_nx is the successor of g; both loops advance through `next_group`, and an iteration that leaves its loop for the other one does
  // not advance: g, g_nx and the pending ticket stay what they are, nothing is claimed twice and nothing is dropped.
  int g_nx = -1;
  unsigned pend = 0u;
  // (dyn_first and the counters are read from the kernarg segment where they are used, like the iteration's parameters: kernarg_view)
  auto n_static = [&]() -> int { return kernarg_view<FwdParams>()->dyn_first >> 3; };   // the static part in positions of an XCD's chunk list
  auto claim = [&]() -> unsigned {
    unsigned t = 0u;
    if (lane == 0) t = atomicAdd(kernarg_view<FwdParams>()->sched + 32 * xcd, 1u);
    return t;
  };
  auto claimed_group = [&](unsigned ticket) -> int { return group_of(n_static() + (int)__builtin_amdgcn_readfirstlane(ticket)); };
  // the successor of the group an iteration has just finished (the loops' latch; idx is that successor's position already)
  auto next_group = [&]() -> int {
    const int gn = g_nx;
    if (gn >= 0) {
      const int ns = n_static();
      g_nx = idx + waves_per_xcd < ns ? group_of(idx + waves_per_xcd) : claimed_group(pend);
      if (g_nx >= 0 && idx + 2 * waves_per_xcd >= ns) pend = claim();
    }
    return gn;
  };
  if constexpr (DYN) {
    const int ns = n_static();
    g = idx < ns ? group_of(idx) : claimed_group(claim());
    if (g >= 0) g_nx = idx + waves_per_xcd < ns ? group_of(idx + waves_per_xcd) : claimed_group(claim());
    if (g_nx >= 0 && idx + 2 * waves_per_xcd >= ns) pend = claim();
  }
  // z of the first ray group -- or, without z_samp, its jitter u: sample_coarse then runs at the top of the iteration (coarse_depth)
  float z_pre = 0.0f, zn_pre = 0.0f;
  if (g >= 0) {
    const int K = BTS_PIN(PinnedSet::K, p.K);
    const long row = lane_ray(g, 0) * K;
    const int kk = min(lane_k(0), K - 1);
    if (BTS_PIN(false, p.z_samp != nullptr)) z_pre = p.z_samp[row + kk], zn_pre = p.z_samp[row + min(kk + 1, K - 1)];
    else z_pre = p.jitter[row + kk];
  }
  // one ray per iteration: the ray (origin, direction, near, far: 32 bytes, wave-uniform) of the NEXT iteration is fetched while this one
  // is evaluated -- as a VECTOR load (all lanes the same address: one request), because a scalar load in flight turns every LDS wait
  // behind it into lgkmcnt(0) (scalar loads return out of order), i.e. the round trip would stall the first weight read instead of the
  // loop head.  Lane i (mod 8) holds float i of the record: one register, one 32-byte request; the loop head moves eight lanes into SGPRs.
  float nrec = 0.0f;
  if constexpr (ONE_RAY) {
    if (g >= 0) nrec = p.rays[(long)g * 8 + (lane & 7)];
  }
  const int K0 = BTS_PIN(PinnedSet::K, p.K);
  const float step0 = 1.0f / (float)K0;                        // nerf.py:107
  const float base0 = coarse_base(K0, min(kl, K0 - 1));        // linspace(0, 1 - step, K)[k] of this lane's sample (first chunk)

  // Two loops (kTwoLoops: one ray per wave): the general one, and one for rays whose 64 samples hit the same four texels
  // of G (every ray that starts at the encoder camera's centre: half of the eval frame) -- see gs_issue.  The test sits behind
  // make_taps and is wave-uniform: every lane's (o00, o01, o10) against lane 0's.  An iteration whose ray is of the other kind puts
  // back what it prefetched and leaves its loop WITHOUT advancing; the wave goes on in the other loop, which computes the ray's
  // geometry again (a frame's rays are sorted by view: one switch per wave and batch element).  Two loop nests (the body is
  // bts_render_iter.h, included once per nest) instead of a branch in one body: the general loop keeps its registers and schedule.
  // Built where the second nest costs no spilled VGPR: no ResnetBlocks, at most two render views -- the evaluation kernels, whose
  // rays are the ones that start at the encoder camera.  -DBTS_NO_SHARED_TEXELS: the general loop alone, the kernels as they were.
#ifndef BTS_NO_SHARED_TEXELS
  constexpr bool kTwoLoops = ONE_RAY && !EPI && NB == 0 && NVMAX <= 2;
#else
  constexpr bool kTwoLoops = false;
#endif
  if constexpr (kTwoLoops) {
    bool shared_loop = K0 <= 64;
    while (g >= 0) {
      if (shared_loop) {
        for (; g >= 0; idx += waves_per_xcd, g = DYN ? next_group() : group_of(idx))
#define BTS_ITER_SHARED true
#include "bts_render_iter.h"
      } else {
        for (; g >= 0; idx += waves_per_xcd, g = DYN ? next_group() : group_of(idx))
#define BTS_ITER_SHARED false
#include "bts_render_iter.h"
      }
      shared_loop = !shared_loop;
    }
  } else {
    for (; g >= 0; idx += waves_per_xcd, g = DYN ? next_group() : group_of(idx))
#define BTS_ITER_SHARED false
#include "bts_render_iter.h"
  }
#ifdef BTS_PROBE
  if ((p.ablate & 128) && p.dbg && lane == 0) {
    unsigned long long* d = p.dbg + ((long)blockIdx.x * 4 + wave) * 8;
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = t_acc[i];
    d[6] = __builtin_readcyclecounter() - t_begin;
    d[7] = ((t_stage < 0xFFFFull ? t_stage : 0xFFFFull) << 36) | ((unsigned long long)xcc_id << 32) | hw_id;
  }
#endif
}

#ifndef BTS_NO_LAUNCH_GLUE
// One of up to seven instantiations per (shape, NVMAX, EPI): ONE_RAY x {plain, IMG}, plus DYN (with and without IMG) for the evaluation
// frame's one-ray kernels with two loops, plus PINNED on top of DYN + IMG at one render view (`pin`: the caller allows it).  A launch that asks for a form its shape was not built in takes the next plainer one: a
// staged image without an IMG kernel is staged in place, a claimed tail without a DYN kernel is walked as static lists.
template <int C, int HD, int NB, int NVMAX, bool EPI>
static int launch_render_p_one(const FwdParams& p, int grid, hipStream_t s, bool pin) {
  auto go = [&](auto kern) {
    launch_dyn_lds(kern, grid, 4 * kGatherLdsPerWave, s, p);
    return launch_check();
  };
  constexpr bool kImg = !EPI && NVMAX <= 2;   // built with the staged MLP ready-made (FwdParams::mlp_image)
  constexpr bool kDyn = kImg && NB == 0;      // built with the claimed tail (FwdParams::sched); one ray per wave only
  const bool one_ray = p.lpr == 64;
  const bool dyn = kDyn && one_ray && p.sched && p.dyn_first < p.groups;
  const bool img = kImg && p.mlp_image;
  if constexpr (kDyn && NVMAX == PinnedSet::nv) {   // the evaluation frame's kernel with the frame's switches compiled in (PinnedSet)
    if (dyn && img && pin && PinnedSet::matches(p)) return go(render_kernel_p<C, HD, NB, NVMAX, true, true, EPI, true, true, true>);
  }
  if constexpr (kDyn) {
    if (dyn) return img ? go(render_kernel_p<C, HD, NB, NVMAX, true, true, EPI, true, true>) : go(render_kernel_p<C, HD, NB, NVMAX, true, true, EPI, true>);
  }
  if constexpr (kImg) {
    if (img) return one_ray ? go(render_kernel_p<C, HD, NB, NVMAX, true, true, EPI, false, true>) : go(render_kernel_p<C, HD, NB, NVMAX, false, true, EPI, false, true>);
  }
  return one_ray ? go(render_kernel_p<C, HD, NB, NVMAX, true, true, EPI>) : go(render_kernel_p<C, HD, NB, NVMAX, false, true, EPI>);
}

template <bool EPI>
inline int launch_render_p(const FwdParams& p, int C, int HD, int NB, int grid, hipStream_t s, bool pin = false) {
  return with_shape(C, HD, NB, [&](auto sh) {
    using S = decltype(sh);
    return with_nvmax(p.nv, [&](auto nvmax) { return launch_render_p_one<S::C, S::HD, S::NB, nvmax(), EPI>(p, grid, s, pin); });
  });
}
#endif  // BTS_NO_LAUNCH_GLUE

}  // namespace bts
