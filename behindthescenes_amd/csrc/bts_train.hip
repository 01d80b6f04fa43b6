// bts_train_step_fwd / bts_train_step_bwd (ABI 7): a training step's share of the renderer enqueued from ONE call per direction.
//
// Nothing here computes anything new: the forward is camera hand-over -> rgb0 packing of the render frames -> patch rays, then per
// scale tile flags -> projection of the flagged tiles -> the fused render kernel (lean outputs + the backward's saved state) -> the
// photometric loss pass, and one reduction of the per-patch sums; the backward is, per scale, the three render passes and the tile
// projection backward.  The kernels, their launch geometry and their arguments are those of the entry-by-entry path
// (bts_render_fwd, bts_photometric_loss, ...: the *_impl functions those entry points call) -- what goes away is the HOST work
// between them: ~20 ctypes calls, ~40 allocator round trips, the autograd nodes and ~25 small torch kernels per exp_kitti_raw.yaml
// step, which took longer to issue (1.1 ms) than the GPU needed to run the step's kernels (0.5 ms).
// Reference: BTSWrapper.forward (models/bts/trainer.py:208-259) + the criterion call of utils/base_trainer.py:287-297.
#include "bts_host.h"

#include <cstring>

namespace bts {

// ---- loss_vals = loss_matrix . [per-scale sums of the loss pass' per-patch parts]: one work-group, lanes stride the patches
struct FinishParams {
  const float* parts[BTS_MAX_SCALES];   // (n_patches, 4) each
  int n_scales, n_patches;
  float M[9 * 3 * BTS_MAX_SCALES];
  float* out;   // (9)
};
__global__ __launch_bounds__(256) void loss_finish_kernel(const FinishParams p) {
  __shared__ float red[4][3 * BTS_MAX_SCALES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[3 * BTS_MAX_SCALES];
#pragma unroll
  for (int i = 0; i < 3 * BTS_MAX_SCALES; ++i) acc[i] = 0.0f;
#pragma unroll
  for (int s = 0; s < BTS_MAX_SCALES; ++s) {
    if (s >= p.n_scales) break;
    const float4* q = reinterpret_cast<const float4*>(p.parts[s]);
    for (int i = threadIdx.x; i < p.n_patches; i += 256) {
      const float4 v = q[i];
      acc[3 * s] += v.x, acc[3 * s + 1] += v.y, acc[3 * s + 2] += v.z;
    }
  }
#pragma unroll
  for (int i = 0; i < 3 * BTS_MAX_SCALES; ++i) {
    float v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int cols = 3 * p.n_scales;
    float o = 0.0f;
    for (int c = 0; c < cols; ++c) o += p.M[threadIdx.x * cols + c] * (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]);
    p.out[threadIdx.x] = o;
  }
}

// ---- gs = g * (coefficient of the scale's sum in the loss * upstream gradient): what autograd does with the loss pass' gradients on the
// entry-by-entry path (`g_rgb * g[0]`, g = loss_matrix[8] * upstream: the same two roundings)
struct ScaleGradParams {
  const float* g_rgb[BTS_MAX_SCALES];
  const float* g_depth[BTS_MAX_SCALES];
  float* gs_rgb[BTS_MAX_SCALES];
  float* gs_depth[BTS_MAX_SCALES];
  float c_rgb[BTS_MAX_SCALES], c_eas[BTS_MAX_SCALES];
  const float* g_loss;   // device scalar or null (1)
  int n_scales;
  long n_rgb, n_depth;   // elements per scale
  // regions the backward accumulates into: the packed parameter gradient, the projected empty feature's, pass C's slot copies (float counts)
  float* zero[2 + BTS_MAX_SCALES];
  long zero_n[2 + BTS_MAX_SCALES];
  int n_zero;
};
__global__ __launch_bounds__(256) void scale_grads_kernel(const ScaleGradParams p) {
  const float up = p.g_loss ? *p.g_loss : 1.0f;
  const int s = blockIdx.y;
  const float a = p.c_rgb[s] * up, b = p.c_eas[s] * up;
  const float* gr = p.g_rgb[s];
  const float* gd = p.g_depth[s];
  float* orr = p.gs_rgb[s];
  float* od = p.gs_depth[s];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < p.n_rgb; i += (long)gridDim.x * 256) orr[i] = gr[i] * a;
  if (gd && od)
    for (long i = blockIdx.x * 256L + threadIdx.x; i < p.n_depth; i += (long)gridDim.x * 256) od[i] = gd[i] * b;
  if (s == 0)      // (one launch instead of a fill per region: each was a dispatch gap of its own on the queue)
    for (int r = 0; r < p.n_zero; ++r)
      for (long i = blockIdx.x * 256L + threadIdx.x; i < p.zero_n[r]; i += (long)gridDim.x * 256) p.zero[r][i] = 0.0f;
}

// ---- learn_empty: the render backward leaves the gradient of the PROJECTED empty feature e_p = w_in[:, :C] . e in d_empty_proj (Hd);
// chain rule on parameter-sized tensors: d e[c] = sum_h w_in[h, c] d e_p[h],  d w_in[h, c] += d e_p[h] e[c]
__global__ __launch_bounds__(256) void empty_grad_kernel(const float* __restrict__ mlp, const float* __restrict__ empty, const float* __restrict__ d_eproj,
                                                       int C, int HD, int d_in, float* __restrict__ d_mlp, float* __restrict__ d_empty) {
  for (int i = threadIdx.x; i < HD * C; i += 256) {
    const int h = i / C, c = i - h * C;
    if (d_mlp) d_mlp[h * d_in + c] += d_eproj[h] * empty[c];
  }
  if (d_empty)
    for (int c = threadIdx.x; c < C; c += 256) {
      float a = 0.0f;
      for (int h = 0; h < HD; ++h) a += mlp[h * d_in + c] * d_eproj[h];
      d_empty[c] = a;
    }
}

// ---- independent scales on independent queues.  A "multiscale" step (trainer.py:220-242; exp_re10k.yaml) renders the same rays against four
// maps: four chains of small kernels (flag, project, render, loss | rows, scatter, dW_pe, reduce, projection backward) that share nothing
// but read-only inputs and the atomically accumulated parameter gradient.  One after the other on one queue every kernel pays its own
// ramp-up and tail (a persistent grid's last waves run alone) and ~45 launch gaps per step; on side queues the chains fill each other's
// tails.  The queues and their fork / join events are created once per host thread and device (handles only, no device memory) and
// are ordered INSIDE the caller's stream: the first kernel of a side chain waits for an event recorded on the caller's stream, the
// caller's stream waits for every chain's last kernel before the call's last kernel -- to the caller the call is still one stream-ordered
// unit.
struct SideQueues {
  hipStream_t q[BTS_MAX_SCALES - 1];
  hipEvent_t fork, first, join[BTS_MAX_SCALES - 1];
  bool ok;
};
static SideQueues* side_queues() {
  static thread_local SideQueues* per_dev[16] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!per_dev[dev]) {
    SideQueues* sq = new SideQueues;
    sq->ok = hipEventCreateWithFlags(&sq->fork, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sq->first, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < BTS_MAX_SCALES - 1; ++i)
      sq->ok = sq->ok && hipStreamCreateWithFlags(&sq->q[i], hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&sq->join[i], hipEventDisableTiming) == hipSuccess;
    per_dev[dev] = sq;
  }
  return per_dev[dev]->ok ? per_dev[dev] : nullptr;
}

static long map_texels(const BtsTrainStep* st, int s) { return (long)(st->cfg.H >> st->scale[s].feat_shift) * (st->cfg.W >> st->scale[s].feat_shift); }

static int check_step(const BtsTrainStep* st, const char* who, bool bwd) {
  if (!st) {
    set_error("%s: NULL step", who);
    return BTS_E_INVALID;
  }
  const BtsFieldCfg& c = st->cfg;
  if (c.n <= 0 || c.H <= 0 || c.W <= 0 || st->v <= 0 || st->P <= 0 || st->ph <= 0 || st->pw <= 0 || st->K <= 0 || st->ph * st->pw > 64 ||
      st->ph > c.H || st->pw > c.W) {
    set_error("%s: non-positive size, or a patch of more than 64 pixels / larger than the frame (n=%ld, P=%ld, K=%ld)", who, c.n, st->P, st->K);
    return BTS_E_INVALID;
  }
  if (!shape_supported(c.C, c.d_hidden, c.n_blocks) || c.num_freqs != kNumFreqs || c.nv < 1 || c.nv > BTS_MAX_VIEWS) {
    set_error("%s: configuration outside the compiled envelope (C=%ld d_hidden=%ld n_blocks=%ld; needs num_freqs=6, 1 <= nv <= 8)", who, c.C, c.d_hidden,
              c.n_blocks);
    return BTS_E_UNSUPPORTED;
  }
  if (st->n_scales < 1 || st->n_scales > BTS_MAX_SCALES || st->n_loss < 1 || st->n_loss > BTS_MAX_LOSS_VIEWS) {
    set_error("%s: n_scales=%ld must be 1..4 and n_loss=%ld 1..16", who, st->n_scales, st->n_loss);
    return BTS_E_INVALID;
  }
  if (st->invalid_policy < 0 || st->invalid_policy > 2 || (c.code_mode != 0 && c.code_mode != 1) || c.enc_render_view < -1 || c.enc_render_view >= c.nv) {
    set_error("%s: invalid_policy=%ld / code_mode=%ld / enc_render_view=%ld out of range", who, st->invalid_policy, c.code_mode, c.enc_render_view);
    return BTS_E_INVALID;
  }
  bool ids_ok = st->id_encoder >= 0 && st->id_encoder < st->v;
  for (int j = 0; j < c.nv; ++j) ids_ok = ids_ok && st->ids_render[j] >= 0 && st->ids_render[j] < st->v;
  for (int j = 0; j < st->n_loss; ++j) ids_ok = ids_ok && st->ids_loss[j] >= 0 && st->ids_loss[j] < st->v;
  if (!ids_ok) {
    set_error("%s: a frame id outside [0, v=%ld)", who, st->v);
    return BTS_E_INVALID;
  }
  if (!st->images || !st->Ks || !st->poses_c2w || !st->patch_v || !st->patch_y || !st->patch_x || !st->mlp_params || !st->rays || !st->rgb_gt ||
      !st->loss_vals || !st->cams || !st->imgs_nhwc4 || (c.learn_empty && !st->empty_feature)) {
    set_error("%s: NULL input / output / scratch pointer", who);
    return BTS_E_INVALID;
  }
  for (int s = 0; s < st->n_scales; ++s) {
    const BtsTrainScale& q = st->scale[s];
    const int fs = q.feat_shift;
    if (fs < 0 || fs > 6 || (c.H & ((1 << fs) - 1)) || (c.W & ((1 << fs) - 1))) {
      set_error("%s: scale %ld: feat_shift=%ld needs 0..6 and H, W multiples of 2^feat_shift", who, s, fs);
      return BTS_E_INVALID;
    }
    if ((reinterpret_cast<uintptr_t>(q.sampled_tiles) & 3) != 0) {
      set_error("%s: scale %ld: sampled_tiles must be 4-byte aligned (the hand-over kernel clears the flags word-wise)", who, s);
      return BTS_E_INVALID;
    }
    if (!q.feat_nchw || !q.jitter || !q.rgb || !q.depth || !q.invalid_wsum || !q.invalid_any || !q.proj_nhwc || !q.sampled_tiles || !q.z_samp ||
        !q.sigma_raw || !q.trans || !q.rgb_samps || !q.loss_parts || !q.g_rgb || !q.g_depth) {
      set_error("%s: scale %ld: NULL pointer", who, s);
      return BTS_E_INVALID;
    }
    if (bwd && (!q.gs_rgb || !q.gs_depth || !q.d_proj_nhwc || !q.d_proj_tiles)) {
      set_error("%s: scale %ld: NULL backward pointer (gs_rgb, gs_depth, d_proj_nhwc, d_proj_tiles)", who, s);
      return BTS_E_INVALID;
    }
  }
  return BTS_OK;
}

// the per-scale views of the step as the single-call entry points take them
struct ScaleView {
  BtsFieldCfg cfg;
  BtsFieldTensors t;
  BtsRenderArgs a;
};
static ScaleView scale_view(const BtsTrainStep* st, int s) {
  ScaleView v;
  memset(&v, 0, sizeof(v));
  const BtsTrainScale& q = st->scale[s];
  v.cfg = st->cfg;
  v.cfg.feat_shift = q.feat_shift;
  // the scale's tile geometry: 16 x 4 blocks for a channels-last map, runs of 64 texels for an NCHW one (BtsFieldCfg.tile_blocks: what each
  // layout is faster with); the step's own flag arrays never leave the two calls, so the step decides for itself
  v.cfg.tile_blocks = q.feat_channels_last != 0;
  const CamBlock cam = split_cams(st->cams, st->cfg.n, st->cfg.nv);
  v.t.proj_nhwc = q.proj_nhwc, v.t.K_enc = cam.K_enc, v.t.w2c_enc = cam.w2c_enc, v.t.imgs_nhwc4 = st->imgs_nhwc4, v.t.K_r = cam.K_r, v.t.w2c_r = cam.w2c_r;
  v.t.empty_feature = st->cfg.learn_empty ? st->empty_feature : nullptr, v.t.mlp_params = st->mlp_params;
  v.a.rays_per_sample = st->P * st->ph * st->pw, v.a.K = st->K, v.a.hard_alpha_cap = st->hard_alpha_cap, v.a.white_bkgd = 0;
  v.a.rays = st->rays, v.a.lindisp = st->lindisp;
  return v;
}

int train_step_fwd_impl(const BtsTrainStep* st, hipStream_t main_stream) {
  hipStream_t stream = main_stream;
  const BtsFieldCfg& c = st->cfg;
  const int n = c.n, nv = c.nv, Bp = st->P * st->ph * st->pw;
  unsigned char* zero[BTS_MAX_SCALES];
  long zero_bytes[BTS_MAX_SCALES];
  for (int s = 0; s < st->n_scales; ++s) zero[s] = st->scale[s].sampled_tiles, zero_bytes[s] = (long)n * map_tiles(c.H, c.W, st->scale[s].feat_shift);
  int rc = handover_launch(st->Ks, st->poses_c2w, st->images, st->patch_v, st->patch_y, st->patch_x, n, st->v, st->id_encoder, nv, st->ids_render, st->n_loss,
                           st->ids_loss, c.H, c.W, st->P, st->ph, st->pw, st->z_near, st->z_far, st->img_scale, st->img_shift, st->cams, st->imgs_nhwc4,
                           st->rays, st->rgb_gt, st->n_scales, zero, zero_bytes, stream);
  if (rc) {
    set_error("%s: the hand-over kernel launch failed", "bts_train_step_fwd");
    return rc;
  }
  FinishParams fin;
  memset(&fin, 0, sizeof(fin));
  SideQueues* sq = (st->concurrent_scales && st->n_scales > 1) ? side_queues() : nullptr;
  if (sq) {
    if (hipEventRecord(sq->fork, main_stream) != hipSuccess) return BTS_E_LAUNCH;
    for (int s = 1; s < st->n_scales; ++s)
      if (hipStreamWaitEvent(sq->q[s - 1], sq->fork, 0) != hipSuccess) return BTS_E_LAUNCH;
  }
  // one slice of the (idle) backward workspace per scale for the projection's tile list
  const size_t fwd_ws = st->bwd_workspace ? (st->bwd_workspace_bytes / (size_t)st->n_scales) & ~(size_t)255 : 0;
  for (int s = 0; s < st->n_scales; ++s) {
    hipStream_t stream = (sq && s > 0) ? sq->q[s - 1] : main_stream;
    const BtsTrainScale& q = st->scale[s];
    ScaleView v = scale_view(st, s);
    const long texels = map_texels(st, s);
    rc = mark_tiles_impl(st->rays, nullptr, q.jitter, v.t.w2c_enc, v.t.K_enc, (long)n * Bp, Bp, st->K, st->lindisp, c.H, c.W, q.feat_shift, q.sampled_tiles,
                         stream, v.cfg.tile_blocks);
    if (!rc) rc = project_features_impl(c.C, c.d_hidden, q.feat_nchw, st->mlp_params, n, (int)texels, q.proj_nhwc, q.sampled_tiles, stream, q.feat_channels_last != 0,
                                        tile_geometry_width(&v.cfg),
                                        // the backward's workspace is idle during the forward: the scale's slice of it holds the tile list
                                        fwd_ws ? static_cast<char*>(st->bwd_workspace) + fwd_ws * (size_t)s : nullptr, fwd_ws);
    if (rc) {
      set_error("%s: projection launch failed at scale %ld", "bts_train_step_fwd", s);
      return rc;
    }
    v.a.jitter = q.jitter, v.a.z_samp_out = q.z_samp;
    v.a.rgb = q.rgb, v.a.depth = q.depth, v.a.rgb_samps = q.rgb_samps, v.a.sigma_raw = q.sigma_raw, v.a.trans = q.trans;
    v.a.invalid_wsum = q.invalid_wsum, v.a.invalid_any = q.invalid_any;
    rc = render_fwd_impl(&v.cfg, &v.t, &v.a, stream);
    if (rc) return rc;
    // the invalid-ray mask of EVERY scale's term comes from scale 0's render (loss.py:100-118 reads data["coarse"][0]): the side chains'
    // loss passes wait for it
    if (sq && s == 0 && hipEventRecord(sq->first, main_stream) != hipSuccess) return BTS_E_LAUNCH;
    if (sq && s > 0 && st->invalid_policy != 0 && hipStreamWaitEvent(stream, sq->first, 0) != hipSuccess) return BTS_E_LAUNCH;
    BtsLossArgs la;
    memset(&la, 0, sizeof(la));
    la.rgb = q.rgb, la.depth = st->edge_aware_smoothness ? q.depth : nullptr, la.rgb_gt = st->rgb_gt, la.parts = q.loss_parts;
    la.g_rgb = q.g_rgb, la.g_depth = st->edge_aware_smoothness ? q.g_depth : nullptr;
    la.n_patches = n * st->P, la.patch_h = st->ph, la.patch_w = st->pw, la.nv = nv, la.K = 0;
    la.invalid_policy = st->invalid_policy, la.edge_aware_smoothness = st->edge_aware_smoothness, la.scale_rgb = 1.0f, la.scale_eas = 1.0f;
    la.invalid_wsum = st->invalid_policy == 2 ? st->scale[0].invalid_wsum : nullptr;
    la.invalid_any = st->invalid_policy == 1 ? st->scale[0].invalid_any : nullptr;
    rc = photometric_loss_impl(&la, stream);
    if (rc) return rc;
    fin.parts[s] = q.loss_parts;
    if (sq && s > 0 && (hipEventRecord(sq->join[s - 1], stream) != hipSuccess || hipStreamWaitEvent(main_stream, sq->join[s - 1], 0) != hipSuccess))
      return BTS_E_LAUNCH;
  }
  stream = main_stream;
  fin.n_scales = st->n_scales, fin.n_patches = n * st->P, fin.out = st->loss_vals;
  memcpy(fin.M, st->loss_matrix, sizeof(float) * 9 * 3 * st->n_scales);
  loss_finish_kernel<<<1, 256, 0, stream>>>(fin);
  return launch_check("%s: loss reduction launch failed", "bts_train_step_fwd");
}

int train_step_bwd_impl(const BtsTrainStep* st, const float* g_loss, hipStream_t main_stream) {
  hipStream_t stream = main_stream;
  const BtsFieldCfg& c = st->cfg;
  const int n = c.n, nv = c.nv, Bp = st->P * st->ph * st->pw;
  const int cols = 3 * st->n_scales;
  const long n_params = MlpLayout{c.C + 3 + 6 * c.num_freqs, c.d_hidden, c.n_blocks}.total();
  ScaleGradParams sg;
  memset(&sg, 0, sizeof(sg));
  for (int s = 0; s < st->n_scales; ++s) {
    const BtsTrainScale& q = st->scale[s];
    sg.g_rgb[s] = q.g_rgb, sg.g_depth[s] = st->edge_aware_smoothness ? q.g_depth : nullptr, sg.gs_rgb[s] = q.gs_rgb, sg.gs_depth[s] = q.gs_depth;
    sg.c_rgb[s] = st->loss_matrix[8 * cols + 3 * s], sg.c_eas[s] = st->loss_matrix[8 * cols + 3 * s + 1];
  }
  sg.g_loss = g_loss, sg.n_scales = st->n_scales, sg.n_rgb = (long)n * Bp * nv * 3, sg.n_depth = (long)n * Bp;
  // one workspace slice per scale when the scales run side by side (the passes of a scale hand each other its contents)
  size_t ws_each = 0;
  ScaleView v0 = scale_view(st, 0);
  ws_each = (render_bwd_workspace_impl(&v0.cfg, &v0.a) + 255) & ~(size_t)255;
  if (ws_each > st->bwd_workspace_bytes || (ws_each && !st->bwd_workspace)) {
    set_error("%s: bwd_workspace too small (%ld bytes needed)", "bts_train_step_bwd", (long)ws_each);
    return BTS_E_WORKSPACE;
  }
  SideQueues* sq = (st->concurrent_scales && st->n_scales > 1 && st->bwd_workspace_bytes >= ws_each * (size_t)st->n_scales) ? side_queues() : nullptr;
  const bool want_empty = c.learn_empty && st->d_empty_proj && (st->d_mlp_params || st->d_empty_feature);
  if (st->d_mlp_params) sg.zero[sg.n_zero] = st->d_mlp_params, sg.zero_n[sg.n_zero++] = n_params;
  if (want_empty) sg.zero[sg.n_zero] = st->d_empty_proj, sg.zero_n[sg.n_zero++] = c.d_hidden;
  for (int s = 0; s < (sq ? st->n_scales : 1); ++s) {     // pass C's slot copies: the reduce kernel leaves them zero again, one fill serves every scale
    float* fp;
    size_t fb;
    render_bwd_flush_region(&v0.cfg, &v0.a, static_cast<char*>(st->bwd_workspace) + ws_each * (size_t)s, &fp, &fb);
    sg.zero[sg.n_zero] = fp, sg.zero_n[sg.n_zero++] = (long)(fb / sizeof(float));
  }
  const long want = (sg.n_rgb + 255) / 256;
  scale_grads_kernel<<<dim3((unsigned)(want < 1024 ? want : 1024), (unsigned)st->n_scales), 256, 0, stream>>>(sg);
  if (int rc = launch_check("%s: gradient scaling launch failed", "bts_train_step_bwd")) return rc;
  if (sq) {
    if (hipEventRecord(sq->fork, main_stream) != hipSuccess) return BTS_E_LAUNCH;
    for (int s = 1; s < st->n_scales; ++s)
      if (hipStreamWaitEvent(sq->q[s - 1], sq->fork, 0) != hipSuccess) return BTS_E_LAUNCH;
  }
  for (int s = 0; s < st->n_scales; ++s) {
    stream = (sq && s > 0) ? sq->q[s - 1] : main_stream;
    const BtsTrainScale& q = st->scale[s];
    ScaleView v = scale_view(st, s);
    v.a.z_samp = q.z_samp, v.a.sigma_raw = q.sigma_raw, v.a.trans = q.trans, v.a.rgb_samps = q.rgb_samps;
    BtsRenderGrads g;
    memset(&g, 0, sizeof(g));
    g.g_rgb = q.gs_rgb, g.g_depth = st->edge_aware_smoothness ? q.gs_depth : nullptr;
    const bool need_map = q.d_feat_nchw != nullptr || st->d_mlp_params != nullptr;
    g.d_proj_nhwc = need_map ? q.d_proj_nhwc : nullptr, g.d_proj_tiles = need_map ? q.d_proj_tiles : nullptr;
    g.d_mlp_params = st->d_mlp_params, g.d_empty_proj = want_empty ? st->d_empty_proj : nullptr;
    const size_t need = render_bwd_workspace_impl(&v.cfg, &v.a);
    void* ws = sq ? static_cast<void*>(static_cast<char*>(st->bwd_workspace) + ws_each * (size_t)s) : st->bwd_workspace;
    const size_t ws_bytes = sq ? ws_each : st->bwd_workspace_bytes;
    if (need > ws_bytes || (need && !st->bwd_workspace)) {
      set_error("%s: bwd_workspace too small (%ld bytes needed)", "bts_train_step_bwd", (long)need);
      return BTS_E_WORKSPACE;
    }
    int rc = render_bwd_impl(&v.cfg, &v.t, &v.a, &g, ws, stream, true);
    if (rc) return rc;
    if (need_map) {
      float* slots;
      size_t slot_bytes;
      render_bwd_flush_region(&v.cfg, &v.a, ws, &slots, &slot_bytes);   // (pass C's slot copies at the END of the slice stay zero between the scales)
      rc = project_features_bwd_tiles_impl(c.C, c.d_hidden, q.feat_nchw, q.d_proj_nhwc, q.d_proj_tiles, st->mlp_params, n, (int)map_texels(st, s),
                                           q.d_feat_nchw, st->d_mlp_params, 1, stream, q.feat_channels_last != 0, tile_geometry_width(&v.cfg),
                                           // the scale's slice of the backward workspace is dead by now (everything bts_render_bwd parked there was
                                           // read by its own passes, enqueued above on this stream) except pass C's slot copies at its END
                                           ws, need > slot_bytes ? need - slot_bytes : 0);
      if (rc) {
        set_error("%s: projection backward launch failed at scale %ld", "bts_train_step_bwd", s);
        return rc;
      }
    }
    if (sq && s > 0 && (hipEventRecord(sq->join[s - 1], stream) != hipSuccess || hipStreamWaitEvent(main_stream, sq->join[s - 1], 0) != hipSuccess))
      return BTS_E_LAUNCH;
  }
  stream = main_stream;
  if (want_empty) {
    empty_grad_kernel<<<1, 256, 0, stream>>>(st->mlp_params, st->empty_feature, st->d_empty_proj, c.C, c.d_hidden, c.C + 3 + 6 * c.num_freqs, st->d_mlp_params,
                                             st->d_empty_feature);
    if (int rc = launch_check("%s: empty-feature gradient launch failed", "bts_train_step_bwd")) return rc;
  }
  return BTS_OK;
}

// prep (bts_eval_frame_prep): the parameter tensors and the scratch of the launch that packs and stages the MLP under the projection;
// NULL: the projection alone, on the caller's packed vector f->mlp_params
struct EvalPrep {
  const BtsMlpTensors* params;
  float *packed, *image;
};
// pin: the render launch may take the kernel with the frame's switches compiled in (PinnedSet); false: the kernel it took without one
int eval_frame_impl(const BtsEvalFrame* f, float* rgb_gt, unsigned* sched, hipStream_t stream, const EvalPrep* prep = nullptr, bool pin = true) {
  const BtsFieldCfg& c = f->cfg;
  const int n = c.n, nv = c.nv;
  // cameras, inverse intrinsics (for distance_to_z behind the render), rgb0 packing, rays and rgb_gt: one launch (it also zeroes `sched`,
  // the render's ticket counter)
  int rc = eval_handover_launch(f->Ks, f->poses_c2w, f->images, n, f->v, f->id_encoder, nv, f->ids_render, c.H, c.W, f->z_near, f->z_far, f->norm_dir,
                                f->img_scale, f->img_shift, f->cams, f->depth_z ? f->inv_K : nullptr, f->imgs_nhwc4, f->rays, rgb_gt, sched, stream);
  // the projection -- with `prep` on lin_in's own weight, and in the same launch the MLP: packed for the render, and staged once for all of
  // its work-groups
  if (!rc && prep)
    rc = eval_prep_launch(c.C, c.d_hidden, c.n_blocks, f->feat_nchw, f->feat_channels_last != 0, f->proj_nhwc, prep->params->tensor,
                          c.learn_empty ? f->empty_feature : nullptr, prep->packed, prep->image, n, c.H * c.W, stream);
  else if (!rc)
    rc = project_features_impl(c.C, c.d_hidden, f->feat_nchw, f->mlp_params, n, c.H * c.W, f->proj_nhwc, nullptr, stream, f->feat_channels_last != 0);
  if (rc) {
    set_error("%s: a hand-over kernel launch failed", "bts_eval_frame");
    return rc;
  }
  BtsFieldCfg cfg = c;
  cfg.feat_shift = 0;
  BtsFieldTensors t;
  memset(&t, 0, sizeof(t));
  const CamBlock cam = split_cams(f->cams, n, nv);
  t.proj_nhwc = f->proj_nhwc, t.K_enc = cam.K_enc, t.w2c_enc = cam.w2c_enc, t.imgs_nhwc4 = f->imgs_nhwc4, t.K_r = cam.K_r, t.w2c_r = cam.w2c_r;
  t.empty_feature = c.learn_empty ? f->empty_feature : nullptr, t.mlp_params = prep ? prep->packed : f->mlp_params;
  BtsRenderArgs a;
  memset(&a, 0, sizeof(a));
  a.rays_per_sample = f->v * c.H * c.W, a.K = f->K, a.hard_alpha_cap = f->hard_alpha_cap, a.rays = f->rays, a.jitter = f->jitter, a.lindisp = f->lindisp;
  a.rgb = f->rgb, a.depth = f->depth, a.weights = f->weights, a.alphas = f->alphas, a.invalid = f->invalid;
  rc = render_fwd_sched_impl(&cfg, &t, &a, sched, stream, prep ? prep->image : nullptr, pin);
  if (rc) return rc;
  if (f->depth_z) {
    rc = distance_to_z_launch(f->depth, f->inv_K, n * f->v, c.H, c.W, f->depth_z, stream);
    if (rc) {
      set_error("%s: distance_to_z launch failed", "bts_eval_frame");
      return rc;
    }
  }
  return BTS_OK;
}

}  // namespace bts

using namespace bts;

extern "C" {

// the argument checks of the eval-frame entry points; packed: the caller hands f->mlp_params over (every entry but bts_eval_frame_prep)
static int check_eval_frame(const BtsEvalFrame* f, const char* who, bool packed) {
  if (!f) {
    set_error("%s: NULL frame", who);
    return BTS_E_INVALID;
  }
  const BtsFieldCfg& c = f->cfg;
  if (c.n <= 0 || c.H <= 0 || c.W <= 0 || f->v <= 0 || f->K <= 0 || c.nv < 0 || c.nv > BTS_MAX_VIEWS) {
    set_error("%s: non-positive size or more than 8 render views (n=%ld, v=%ld, K=%ld)", who, c.n, f->v, f->K);
    return BTS_E_INVALID;
  }
  if (!shape_supported(c.C, c.d_hidden, c.n_blocks) || c.num_freqs != kNumFreqs) {
    set_error("%s: configuration outside the compiled envelope (C=%ld d_hidden=%ld n_blocks=%ld)", who, c.C, c.d_hidden, c.n_blocks);
    return BTS_E_UNSUPPORTED;
  }
  bool ids_ok = f->id_encoder >= 0 && f->id_encoder < f->v;
  for (int j = 0; j < c.nv; ++j) ids_ok = ids_ok && f->ids_render[j] >= 0 && f->ids_render[j] < f->v;
  if (!ids_ok || c.enc_render_view < -1 || c.enc_render_view >= c.nv) {
    set_error("%s: a frame id outside [0, v=%ld) or enc_render_view out of range", who, f->v);
    return BTS_E_INVALID;
  }
  if (!f->images || !f->Ks || !f->poses_c2w || !f->feat_nchw || (packed && !f->mlp_params) || !f->jitter || !f->cams || !f->proj_nhwc || !f->rays ||
      !f->rgb || !f->depth || (c.nv > 0 && !f->imgs_nhwc4) || (f->depth_z && !f->inv_K) || (c.learn_empty && !f->empty_feature)) {
    set_error("%s: NULL input / output / scratch pointer", who);
    return BTS_E_INVALID;
  }
  if ((long)c.n * f->v * c.H * c.W > 0x7FF00000L) {
    set_error("%s: too many rays in one call (%ld)", who, (long)c.n * f->v * c.H * c.W);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}

int bts_eval_frame_sched(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, void* stream) {
  if (int rc = check_eval_frame(f, "bts_eval_frame", true)) return rc;
  return eval_frame_impl(f, rgb_gt, sched, (hipStream_t)stream);
}

int64_t bts_mlp_image_floats(const BtsFieldCfg* cfg) { return cfg ? mlp_image_floats(cfg->C, cfg->d_hidden, cfg->n_blocks) : 0; }

static int eval_frame_prep(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, const BtsMlpTensors* params, float* mlp_packed, float* mlp_image,
                           void* stream, bool pin) {
  const char* who = "bts_eval_frame_prep";
  if (int rc = check_eval_frame(f, who, false)) return rc;
  if (!params || !mlp_packed) {
    set_error("%s: NULL input / output / scratch pointer", who);
    return BTS_E_INVALID;
  }
  const int want = 4 + 4 * f->cfg.n_blocks;
  if (params->n_tensors != want || want > BTS_MLP_MAX_TENSORS) {
    set_error("%s: n_tensors=%ld, the MLP has %ld parameter tensors (4 + 4 * n_blocks)", who, params->n_tensors, want);
    return BTS_E_INVALID;
  }
  for (int i = 0; i < want; ++i)
    if (!params->tensor[i]) {
      set_error("%s: NULL input / output / scratch pointer", who);
      return BTS_E_INVALID;
    }
  if ((reinterpret_cast<uintptr_t>(mlp_image) & 15) != 0) {
    set_error("%s: mlp_image must be 16-byte aligned (the render's work-groups copy it with 16-byte loads)", who);
    return BTS_E_INVALID;
  }
  const EvalPrep prep{params, mlp_packed, mlp_image};
  return eval_frame_impl(f, rgb_gt, sched, (hipStream_t)stream, &prep, pin);
}
int bts_eval_frame_prep(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, const BtsMlpTensors* params, float* mlp_packed, float* mlp_image,
                        void* stream) {
  return eval_frame_prep(f, rgb_gt, sched, params, mlp_packed, mlp_image, stream, true);
}
int bts_eval_frame_prep_unpinned(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, const BtsMlpTensors* params, float* mlp_packed,
                                 float* mlp_image, void* stream) {
  return eval_frame_prep(f, rgb_gt, sched, params, mlp_packed, mlp_image, stream, false);
}

int bts_eval_frame_gt(const BtsEvalFrame* f, float* rgb_gt, void* stream) { return bts_eval_frame_sched(f, rgb_gt, nullptr, stream); }
int bts_eval_frame(const BtsEvalFrame* f, void* stream) { return bts_eval_frame_sched(f, nullptr, nullptr, stream); }

// the host's split of a render launch into static lists and a claimed tail, for tests: grid work-groups, `groups` ray groups -> the
// first claimed group (= groups: no tail); *chunk_log2 (may be NULL) receives the chunk size the split is aligned to
int64_t bts_render_dyn_first(int32_t grid, int64_t groups, int32_t* chunk_log2) {
  const int l = render_chunk_log2(grid, groups);
  if (chunk_log2) *chunk_log2 = l;
  return render_dyn_first(grid, l, groups, 0);
}

// whether a render launch of these arguments matches the pinned set (bts_field_kernel.h: PinnedSet, on the parameters bts_render_fwd fills), for
// tests: 1 / 0, -1 for a NULL argument.  Host only; no pointer is dereferenced.  The launch takes the pinned kernel where, besides, it has
// a claimed tail and a staged MLP (bts_eval_frame_prep)
int32_t bts_render_pinned(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a) {
  if (!cfg || !t || !a) return -1;
  return render_args_pinned(cfg, t, a) ? 1 : 0;
}

int bts_train_step_fwd(const BtsTrainStep* st, void* stream) {
  if (int rc = check_step(st, "bts_train_step_fwd", false)) return rc;
  return train_step_fwd_impl(st, (hipStream_t)stream);
}

int bts_train_step_bwd(const BtsTrainStep* st, const float* g_loss, void* stream) {
  if (int rc = check_step(st, "bts_train_step_bwd", true)) return rc;
  return train_step_bwd_impl(st, g_loss, (hipStream_t)stream);
}

}  // extern "C"
