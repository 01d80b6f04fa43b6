// bts_eval_device.h -- the rules the evaluation kernels share, each written ONCE: bts_occ.hip (LiDAR occupancy), bts_bbox_occ.hip (3D-box
// occupancy), bts_depth_metrics.hip, bts_nvs_metrics.hip and bts_frames.hip (novel-view frames) include it.  Device code only, every
// function inlined into its kernel.
//   - wave reductions by __shfl_down whose result stands in LANE 0 only: the fp64 / int32 sum, the (min, max, NaN flag) triple
//   - the six cells of (V, O, P) of the two occupancy evaluators: their order, and the six-ballot count
// The general look-ups live in bts_common.h: nearest_src, nearest_border_texel, float_key / float_unkey.
// The lane-0 reductions are NOT bts_loss_device.h's wave_sum: that one is a __shfl_xor butterfly after which EVERY lane holds the sum (its
// callers go on computing with it in all lanes), these leave lanes 1 .. 63 with partial garbage and their callers store from lane 0.
// The two add in different orders, so swapping one for the other changes fp64 results in the last bit.  Keep them apart.
// As in bts_loss_device.h, a rule is here only where calling it leaves every kernel the instruction stream it had with the rule written
// inline (tools/asm_compare.py).
#pragma once
#include <hip/hip_runtime.h>

namespace bts {

// ---- lane-0 reductions
__device__ __forceinline__ double lane0_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
__device__ __forceinline__ int lane0_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// One step of the (min, max, NaN flag) reduction and the six of them: the wave's minimum of lo, maximum of hi and of the flag bad (0 / 1).
// By value and returned: with reference parameters frames_minmax_kernel changes its instructions.  bts_frames.hip's fold_minmax runs
// the six steps itself (called as lane0_minmax it changes colorize_kernel's)
struct MinMaxBad {
  float lo, hi, bad;
};
__device__ __forceinline__ void minmax_step(float& lo, float& hi, float& bad, int o) {
  lo = fminf(lo, __shfl_down(lo, o)), hi = fmaxf(hi, __shfl_down(hi, o)), bad = fmaxf(bad, __shfl_down(bad, o));
}
__device__ __forceinline__ MinMaxBad lane0_minmax(float lo, float hi, float bad) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) minmax_step(lo, hi, bad, o);
  return MinMaxBad{lo, hi, bad};
}

// ---- the occupancy evaluators' six cells (evaluator_lidar.py:314-330, evaluator_3dbb.py:283-299)
// The cell of a query point from V (visible), O (occupied & !V) and P (predicted occupied):
//   0: V & P   1: V & !P   2: !V & O & P   3: !V & O & !P   4: !V & !O & P   5: !V & !O & !P
// and masks (3, P): P, O, V as bytes.  occ_metrics_kernel and bbox_metrics_kernel each WRITE THESE LINES OUT (a comment there names the
// twin): as a function -- by value, by reference, as int, the cell and the stores apart, either alone, O formed inside, V and O formed
// inside -- they change both kernels' instructions.  Shared is the count:
// counts[c] += the wave's lanes whose cell is c (-1: a lane past the last point), one ballot and one atomic per wave and cell.  Every
// lane of the work-group calls this
__device__ __forceinline__ void count_cells(int cell, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const unsigned long long b = __ballot(cell == c);
    if (lane == 0 && b) atomicAdd(&counts[c], __popcll(b));
  }
}

}  // namespace bts
