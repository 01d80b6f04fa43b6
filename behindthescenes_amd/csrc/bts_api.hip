// extern "C" entry points of libbts_render.so (declared in include/bts_render.h): argument validation and launch
// geometry only -- no allocation, no synchronisation, no exceptions.
#include "bts_host.h"

#include <cstdio>
#include <cstring>

using namespace bts;

// feat_shift: 0 .. 6, H and W multiples of 2^feat_shift (the small map then IS the nearest-neighbour source of the H x W one)
static int check_shift(const BtsFieldCfg* cfg, const char* who) {
  const int fs = cfg->feat_shift;
  if (fs < 0 || fs > 6 || (cfg->H & ((1 << fs) - 1)) != 0 || (cfg->W & ((1 << fs) - 1)) != 0) {
    set_error("%s: feat_shift=%ld needs 0 <= feat_shift <= 6 and H=%ld, W=%ld multiples of 2^feat_shift", who, (long)fs, (long)cfg->H, (long)cfg->W);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}
static long feat_texels(const BtsFieldCfg* cfg) { return (long)(cfg->H >> cfg->feat_shift) * (cfg->W >> cfg->feat_shift); }

static int check_cfg(const BtsFieldCfg* cfg, const BtsFieldTensors* t, bool need_imgs) {
  if (!cfg || !t) {
    set_error("%s: NULL cfg/tensors", "bts");
    return BTS_E_INVALID;
  }
  if (cfg->n <= 0 || cfg->H <= 0 || cfg->W <= 0 || cfg->nv < 0) {
    set_error("%s: non-positive size n=%ld H=%ld W=%ld", "bts", cfg->n, cfg->H, cfg->W);
    return BTS_E_INVALID;
  }
  if (!bts_supported(cfg)) {
    set_error("%s: configuration outside the compiled envelope (C=%ld d_hidden=%ld n_blocks=%ld; also needs num_freqs=6, nv<=8)",
              "bts", cfg->C, cfg->d_hidden, cfg->n_blocks);
    return BTS_E_UNSUPPORTED;
  }
  if (int rc = check_shift(cfg, "bts")) return rc;
  if (cfg->feat_shift && !t->proj_nhwc) {
    set_error("%s: feat_shift > 0 needs the projected map (proj_nhwc)", "bts");
    return BTS_E_INVALID;
  }
  if ((!t->feat_nhwc && !t->proj_nhwc) || !t->K_enc || !t->w2c_enc || !t->mlp_params) {
    set_error("%s: NULL field tensor", "bts");
    return BTS_E_INVALID;
  }
  if (need_imgs && cfg->nv > 0 && (!t->imgs_nhwc4 || !t->K_r || !t->w2c_r)) {
    set_error("%s: NULL colour-view tensor with nv=%ld", "bts", cfg->nv);
    return BTS_E_INVALID;
  }
  if (cfg->learn_empty && !t->empty_feature) {
    set_error("%s: learn_empty set but empty_feature is NULL", "bts");
    return BTS_E_INVALID;
  }
  if (cfg->enc_render_view < -1 || cfg->enc_render_view >= cfg->nv) {
    set_error("%s: enc_render_view=%ld must be -1 or a render view index below nv=%ld", "bts", cfg->enc_render_view, cfg->nv);
    return BTS_E_INVALID;
  }
  if (cfg->code_mode != 0 && cfg->code_mode != 1) {
    set_error("%s: unknown code_mode %ld", "bts", cfg->code_mode);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}

// The render arguments of the forward (rays, z_samp or jitter, rgb, depth) or backward form (rays, z_samp, the forward's sigma_raw and
// trans), then the sizes.  rest_ok: what else the entry requires under the same message; null_fmt: that message in the entry's wording.
static const char kFwdArgsNull[] = "%s: NULL render argument (rays, z_samp or jitter, rgb and depth are required)";
static int check_render_args(const BtsRenderArgs* a, const char* who, bool bwd, bool rest_ok, const char* null_fmt) {
  if (!a || !rest_ok || !a->rays || (bwd ? (!a->z_samp || !a->sigma_raw || !a->trans) : ((!a->z_samp && !a->jitter) || !a->rgb || !a->depth))) {
    set_error(null_fmt, who);
    return BTS_E_INVALID;
  }
  if (a->rays_per_sample <= 0 || a->K <= 0) {
    set_error("%s: non-positive rays_per_sample=%ld K=%ld", who, (long)a->rays_per_sample, (long)a->K);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}

// What the five bts_project_features* entries check before they launch: the entry's own pointers (ptrs_ok) and the sizes, the compiled
// envelope, feat_shift.  launched(): the launch's code with the entry's message.
static int check_projection(const BtsFieldCfg* cfg, bool ptrs_ok, int N, const char* who) {
  if (!cfg || !ptrs_ok || N <= 0 || cfg->H <= 0 || cfg->W <= 0) {
    set_error("%s: NULL pointer or non-positive size", who);
    return BTS_E_INVALID;
  }
  if (!bts_supported(cfg)) {
    set_error("%s: configuration outside the compiled envelope (C=%ld d_hidden=%ld n_blocks=%ld)", who, cfg->C, cfg->d_hidden, cfg->n_blocks);
    return BTS_E_UNSUPPORTED;
  }
  return check_shift(cfg, who);
}
static int launched(int rc, const char* who) {
  if (rc) set_error("%s: kernel launch failed", who);
  return rc;
}

extern "C" {

int bts_abi_version(void) { return BTS_ABI_VERSION; }
const char* bts_last_error(void) { return last_error(); }

int bts_supported(const BtsFieldCfg* cfg) {
  if (!cfg) return 0;
  return shape_supported(cfg->C, cfg->d_hidden, cfg->n_blocks) && cfg->num_freqs == kNumFreqs && cfg->nv <= BTS_MAX_VIEWS ? 1 : 0;
}

int64_t bts_mlp_param_count(const BtsFieldCfg* cfg) {
  if (!cfg) return -1;
  return MlpLayout{cfg->C + 3 + 6 * cfg->num_freqs, cfg->d_hidden, cfg->n_blocks}.total();
}

int bts_render_fwd(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, void* stream) {
  if (int rc = check_cfg(cfg, t, true)) return rc;
  if (int rc = check_render_args(a, "bts_render_fwd", false, true, kFwdArgsNull)) return rc;
  return render_fwd_impl(cfg, t, a, (hipStream_t)stream);
}

size_t bts_render_bwd_workspace(const BtsFieldCfg* cfg, const BtsRenderArgs* a) {
  if (!cfg || !a) return 0;
  return render_bwd_workspace_impl(cfg, a);
}

int bts_render_bwd(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_cfg(cfg, t, true)) return rc;
  // (this entry names its gradient struct and the map in the same breath as the render arguments)
  if (int rc = check_render_args(a, "bts_render_bwd", true, g && t->proj_nhwc,
                                 "%s: NULL argument (rays, z_samp, the forward's sigma_raw + trans and proj_nhwc are required)"))
    return rc;
  const size_t need = render_bwd_workspace_impl(cfg, a);
  if (workspace_bytes < need || (!workspace && need > 0)) {
    set_error("%s: workspace too small (%ld bytes needed)", "bts_render_bwd", (long)need);
    return BTS_E_WORKSPACE;
  }
  return render_bwd_impl(cfg, t, a, g, workspace, (hipStream_t)stream);
}

int bts_project_features(const BtsFieldCfg* cfg, const float* feat_nchw, const float* mlp_params, int32_t N, float* proj_nhwc,
                         void* stream) {
  const char* who = "bts_project_features";
  if (int rc = check_projection(cfg, feat_nchw && mlp_params && proj_nhwc, N, who)) return rc;
  return launched(project_features_impl(cfg->C, cfg->d_hidden, feat_nchw, mlp_params, N, (int)feat_texels(cfg), proj_nhwc, nullptr, (hipStream_t)stream),
                  who);
}

int bts_project_features_tiles(const BtsFieldCfg* cfg, const float* feat_nchw, const float* mlp_params, int32_t N, const uint8_t* tiles, float* proj_nhwc,
                               void* stream) {
  const char* who = "bts_project_features_tiles";
  if (int rc = check_projection(cfg, feat_nchw && mlp_params && proj_nhwc && tiles, N, who)) return rc;
  return launched(project_features_impl(cfg->C, cfg->d_hidden, feat_nchw, mlp_params, N, (int)feat_texels(cfg), proj_nhwc, tiles, (hipStream_t)stream,
                                        false, tile_geometry_width(cfg)),
                  who);
}

int bts_mark_sampled_tiles(const BtsFieldCfg* cfg, const float* K_enc, const float* w2c_enc, const BtsRenderArgs* a, uint8_t* tiles, void* stream) {
  if (!cfg || !K_enc || !w2c_enc || !a || !tiles || !a->rays || (!a->z_samp && !a->jitter) || cfg->n <= 0 || cfg->H <= 0 || cfg->W <= 0 ||
      a->rays_per_sample <= 0 || a->K <= 0) {
    set_error("%s: NULL pointer, non-positive size, or neither z_samp nor jitter", "bts_mark_sampled_tiles");
    return BTS_E_INVALID;
  }
  if (int rc = check_shift(cfg, "bts_mark_sampled_tiles")) return rc;
  return launched(mark_tiles_impl(a->rays, a->z_samp, a->z_samp ? nullptr : a->jitter, w2c_enc, K_enc, (long)cfg->n * a->rays_per_sample,
                                  a->rays_per_sample, a->K, a->lindisp, cfg->H, cfg->W, cfg->feat_shift, tiles, (hipStream_t)stream, cfg->tile_blocks),
                  "bts_mark_sampled_tiles");
}

int bts_project_features_bwd(const BtsFieldCfg* cfg, const float* feat_nchw, const float* d_proj_nhwc, const float* mlp_params,
                             int32_t N, float* d_feat_nchw, float* d_mlp_params, void* stream) {
  const char* who = "bts_project_features_bwd";
  if (int rc = check_projection(cfg, d_proj_nhwc && mlp_params && !(d_mlp_params && !feat_nchw), N, who)) return rc;
  return launched(project_features_bwd_impl(cfg->C, cfg->d_hidden, feat_nchw, d_proj_nhwc, mlp_params, N, (int)feat_texels(cfg), d_feat_nchw,
                                            d_mlp_params, (hipStream_t)stream),
                  who);
}

int64_t bts_proj_tile_count(const BtsFieldCfg* cfg) {
  // the same bound every entry point that takes the flags checks (check_shift: 0 .. 6, H and W multiples of 2^feat_shift); an invalid
  // configuration answers -1 with a message, never 0 -- a caller that sized its flag array with 0 would hand the kernels no flags at all
  if (!cfg || cfg->H <= 0 || cfg->W <= 0) {
    set_error("%s: NULL cfg or non-positive size", "bts_proj_tile_count");
    return -1;
  }
  if (check_shift(cfg, "bts_proj_tile_count")) return -1;
  return map_tiles(cfg->H, cfg->W, cfg->feat_shift);
}

int bts_project_features_bwd_tiles(const BtsFieldCfg* cfg, const float* feat_nchw, float* d_proj_nhwc, uint8_t* tiles, const float* mlp_params,
                                   int32_t N, float* d_feat_nchw, float* d_mlp_params, int32_t clear_after, void* stream) {
  const char* who = "bts_project_features_bwd_tiles";
  if (int rc = check_projection(cfg, d_proj_nhwc && tiles && mlp_params && !(d_mlp_params && !feat_nchw), N, who)) return rc;
  return launched(project_features_bwd_tiles_impl(cfg->C, cfg->d_hidden, feat_nchw, d_proj_nhwc, tiles, mlp_params, N, (int)feat_texels(cfg), d_feat_nchw,
                                                  d_mlp_params, clear_after, (hipStream_t)stream, false, tile_geometry_width(cfg)),
                  who);
}

int bts_project_features_cl(const BtsFieldCfg* cfg, const float* feat_nhwc, const float* mlp_params, int32_t N, const uint8_t* tiles, float* proj_nhwc,
                            void* stream) {
  const char* who = "bts_project_features_cl";
  if (int rc = check_projection(cfg, feat_nhwc && mlp_params && proj_nhwc, N, who)) return rc;
  return launched(project_features_impl(cfg->C, cfg->d_hidden, feat_nhwc, mlp_params, N, (int)feat_texels(cfg), proj_nhwc, tiles, (hipStream_t)stream,
                                        true, tile_geometry_width(cfg)),
                  who);
}

int bts_project_features_bwd_cl(const BtsFieldCfg* cfg, const float* feat_nhwc, float* d_proj_nhwc, uint8_t* tiles, const float* mlp_params, int32_t N,
                                float* d_feat_nhwc, float* d_mlp_params, int32_t clear_after, void* stream) {
  const char* who = "bts_project_features_bwd_cl";
  if (int rc = check_projection(cfg, d_proj_nhwc && mlp_params && !(d_mlp_params && !feat_nhwc), N, who)) return rc;
  return launched(project_features_bwd_tiles_impl(cfg->C, cfg->d_hidden, feat_nhwc, d_proj_nhwc, tiles, mlp_params, N, (int)feat_texels(cfg), d_feat_nhwc,
                                                  d_mlp_params, clear_after, (hipStream_t)stream, true, tile_geometry_width(cfg)),
                  who);
}

int bts_field_query(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t P, int32_t only_density,
                    float* rgb, float* invalid, float* sigma, void* stream) {
  int rc = check_cfg(cfg, t, !only_density);
  if (rc) return rc;
  if (!xyz || !sigma || P <= 0 || (!only_density && cfg->nv > 0 && !rgb)) {
    set_error("%s: NULL/empty query argument (P=%ld)", "bts_field_query", P);
    return BTS_E_INVALID;
  }
  return field_query_impl(cfg, t, xyz, P, only_density, rgb, invalid, sigma, (hipStream_t)stream);
}

int bts_occupancy_profile(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t Y, int32_t columns, float threshold,
                          int32_t only_density, float* profile, float* sigma, void* stream) {
  int rc = check_cfg(cfg, t, !only_density);
  if (rc) return rc;
  if (!xyz || !profile || Y <= 0 || columns <= 0) {
    set_error("%s: NULL/empty argument (Y=%ld, columns=%ld)", "bts_occupancy_profile", Y, columns);
    return BTS_E_INVALID;
  }
  if (Y > 64 || !t->proj_nhwc || (long)Y * columns > 0x7FFFFFFFL) {
    set_error("%s: needs Y <= 64 levels (got %ld), the projected feature map and fewer than 2^31 points", "bts_occupancy_profile", Y);
    return BTS_E_UNSUPPORTED;
  }
  return occupancy_profile_impl(cfg, t, xyz, Y, columns, threshold, only_density, profile, sigma, (hipStream_t)stream);
}

#define BTS_CHECK_LAYOUT(cond, name)                      \
  if (!(cond)) {                                          \
    set_error("%s: NULL pointer or non-positive size", name); \
    return BTS_E_INVALID;                                 \
  }

int bts_nchw_to_nhwc(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, void* stream) {
  BTS_CHECK_LAYOUT(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "bts_nchw_to_nhwc");
  return launched(transpose_launch(src, dst, N, C, H, W, true, (hipStream_t)stream), "bts_nchw_to_nhwc");
}
int bts_nhwc_to_nchw(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, void* stream) {
  BTS_CHECK_LAYOUT(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "bts_nhwc_to_nchw");
  return launched(transpose_launch(src, dst, N, C, H, W, false, (hipStream_t)stream), "bts_nhwc_to_nchw");
}
int bts_pack_rgb(const float* src, float* dst, int32_t N, int32_t H, int32_t W, float scale, float shift, void* stream) {
  BTS_CHECK_LAYOUT(src && dst && N > 0 && H > 0 && W > 0, "bts_pack_rgb");
  return launched(pack_rgb_launch(src, dst, N, H, W, scale, shift, (hipStream_t)stream), "bts_pack_rgb");
}
int bts_gen_rays(const float* poses, const float* projs, int32_t V, int32_t H, int32_t W, float z_near, float z_far,
                 int32_t norm_dir, float* rays, void* stream) {
  BTS_CHECK_LAYOUT(poses && projs && rays && V > 0 && H > 0 && W > 0, "bts_gen_rays");
  return launched(gen_rays_launch(poses, projs, V, H, W, z_near, z_far, norm_dir, rays, (hipStream_t)stream), "bts_gen_rays");
}
int bts_patch_rays(const float* poses, const float* projs, const float* images, const int32_t* patch_v, const int32_t* patch_y,
                   const int32_t* patch_x, int32_t n, int32_t v, int32_t c, int32_t H, int32_t W, int32_t P, int32_t ph, int32_t pw,
                   float z_near, float z_far, int32_t norm_dir, float* rays, float* rgb_gt, void* stream) {
  BTS_CHECK_LAYOUT(poses && projs && patch_v && patch_y && patch_x && rays && n > 0 && v > 0 && H > 0 && W > 0 && P >= 0 && ph > 0 && pw > 0 &&
                       ph <= H && pw <= W && (!images || (rgb_gt && c > 0)),
                   "bts_patch_rays");
  return launched(patch_rays_launch(poses, projs, images, patch_v, patch_y, patch_x, n, v, c, H, W, P, ph, pw, z_near, z_far, norm_dir, rays,
                                    rgb_gt, (hipStream_t)stream),
                  "bts_patch_rays");
}
// bts_photometric_loss and its _automask form: one set of checks, one launch
static int photometric_loss_entry(const BtsLossArgs* a, const float* thresh, void* stream, const char* who) {
  BTS_CHECK_LAYOUT(a && a->rgb && a->rgb_gt && a->parts && a->n_patches >= 0 && a->patch_h > 0 && a->patch_w > 0 &&
                       a->patch_h * a->patch_w <= 64 && a->nv > 0 && a->invalid_policy >= 0 && a->invalid_policy <= 2 &&
                       (a->invalid_policy != 1 || a->invalid_any || (a->invalid && a->K > 0)) &&
                       (a->invalid_policy != 2 || a->invalid_wsum || (a->invalid && a->weights && a->K > 0)) &&
                       (!a->edge_aware_smoothness || a->depth),
                   who);
  return launched(photometric_loss_impl(a, (hipStream_t)stream, thresh), who);
}
// thresh == NULL: BTS_E_INVALID before anything else of an _automask entry
static int check_thresh(const float* thresh, const char* who) {
  if (thresh) return BTS_OK;
  set_error("%s: thresh is NULL (the per-ray bound, (B) floats; without one call the entry point without _automask)", who);
  return BTS_E_INVALID;
}
int bts_photometric_loss(const BtsLossArgs* a, void* stream) { return photometric_loss_entry(a, nullptr, stream, "bts_photometric_loss"); }
int bts_photometric_loss_automask(const BtsLossArgs* a, const float* thresh, void* stream) {
  static const char who[] = "bts_photometric_loss_automask";
  if (int rc = check_thresh(thresh, who)) return rc;
  return photometric_loss_entry(a, thresh, stream, who);
}
size_t bts_photometric_loss_tiled_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv) {
  return loss_tiled_bytes(n_patches, patch_h, patch_w, nv);
}
size_t bts_photometric_loss_tiled_automask_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv) {
  return loss_tiled_bytes(n_patches, patch_h, patch_w, nv, true);
}
// policies strict / weight_guided (BtsLossArgs, BtsPixelLossArgs): the renderer's per-ray reduction or the per-sample rows it stands for
static int check_policy_inputs(int policy, const float* invalid_any, const float* invalid_wsum, const float* invalid, const float* weights, int K,
                               const char* who) {
  if ((policy == 1 && !invalid_any && !(invalid && K > 0)) || (policy == 2 && !invalid_wsum && !(invalid && weights && K > 0))) {
    set_error("%s: invalid_policy %ld needs invalid_any / invalid_wsum, or invalid (and weights) with K > 0", who, (long)policy);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}
static int photometric_loss_tiled_entry(const BtsLossArgs* a, const float* thresh, void* workspace, size_t workspace_bytes, void* stream,
                                        const char* who) {
  BTS_CHECK_LAYOUT(a && a->rgb && a->rgb_gt && a->parts && a->n_patches >= 0 && a->patch_h > 0 && a->patch_w > 0 && a->nv > 0 &&
                       a->invalid_policy >= 0 && a->invalid_policy <= 2 && (!a->edge_aware_smoothness || a->depth),
                   who);
  if (int rc = check_policy_inputs(a->invalid_policy, a->invalid_any, a->invalid_wsum, a->invalid, a->weights, a->K, who)) return rc;
  if ((long)a->n_patches * a->patch_h * a->patch_w > 2147483647L) {
    set_error("%s: %ld patches of %ld x %ld pixels are more than 2^31 - 1 rays", who, (long)a->n_patches, (long)a->patch_h, (long)a->patch_w);
    return BTS_E_INVALID;
  }
  const size_t need = loss_tiled_bytes(a->n_patches, a->patch_h, a->patch_w, a->nv, thresh != nullptr);
  if (!workspace || workspace_bytes < need) {
    set_error(thresh ? "%s: workspace too small (%ld bytes needed, see bts_photometric_loss_tiled_automask_workspace)"
                     : "%s: workspace too small (%ld bytes needed, see bts_photometric_loss_tiled_workspace)",
              who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(photometric_loss_tiled_impl(a, workspace, (hipStream_t)stream, thresh), who);
}
int bts_photometric_loss_tiled(const BtsLossArgs* a, void* workspace, size_t workspace_bytes, void* stream) {
  return photometric_loss_tiled_entry(a, nullptr, workspace, workspace_bytes, stream, "bts_photometric_loss_tiled");
}
int bts_photometric_loss_tiled_automask(const BtsLossArgs* a, const float* thresh, void* workspace, size_t workspace_bytes, void* stream) {
  static const char who[] = "bts_photometric_loss_tiled_automask";
  if (int rc = check_thresh(thresh, who)) return rc;
  return photometric_loss_tiled_entry(a, thresh, workspace, workspace_bytes, stream, who);
}
size_t bts_photometric_loss_median_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv, int32_t n) {
  return loss_median_bytes(n_patches, patch_h, patch_w, nv, n);
}
int bts_photometric_loss_median(const BtsLossArgs* a, int32_t n, const float* thresh, float* out, float* thresholds, int64_t* kept, void* workspace,
                                size_t workspace_bytes, void* stream) {
  static const char who[] = "bts_photometric_loss_median";
  if (!a || !a->rgb || !a->rgb_gt || !a->parts || !out || (a->edge_aware_smoothness && !a->depth)) {
    set_error("%s: NULL required pointer (args, rgb, rgb_gt, parts, out; depth with edge_aware_smoothness)", who);
    return BTS_E_INVALID;
  }
  if (n <= 0 || a->n_patches <= 0 || a->patch_h <= 0 || a->patch_w <= 0 || a->nv <= 0) {
    set_error("%s: non-positive size (n, n_patches, patch_h, patch_w, nv)", who);
    return BTS_E_INVALID;
  }
  if (a->n_patches % n != 0) {
    set_error("%s: %ld patches are not a multiple of n = %ld batch samples", who, (long)a->n_patches, (long)n);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy < 0 || a->invalid_policy > 2) {
    set_error("%s: unknown invalid_policy %ld (0 none, 1 strict, 2 weight_guided)", who, (long)a->invalid_policy);
    return BTS_E_INVALID;
  }
  if (int rc = check_policy_inputs(a->invalid_policy, a->invalid_any, a->invalid_wsum, a->invalid, a->weights, a->K, who)) return rc;
  if ((long)a->n_patches * a->patch_h * a->patch_w > 2147483647L) {
    set_error("%s: %ld patches of %ld x %ld pixels are more than 2^31 - 1 rays", who, (long)a->n_patches, (long)a->patch_h, (long)a->patch_w);
    return BTS_E_INVALID;
  }
  const size_t need = loss_median_bytes(a->n_patches, a->patch_h, a->patch_w, a->nv, n);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace too small (%ld bytes needed, see bts_photometric_loss_median_workspace)", who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(photometric_loss_median_impl(a, n, thresh, out, thresholds, kept, workspace, (hipStream_t)stream), who);
}
size_t bts_pixel_loss_workspace(int64_t B, int32_t n, int32_t patch_h, int32_t patch_w) { return pixel_loss_bytes((long)B, n, patch_h, patch_w); }
static int pixel_loss_entry(const BtsPixelLossArgs* a, const float* thresh, void* workspace, size_t workspace_bytes, void* stream, const char* who) {
  if (!a || !a->rgb || !a->rgb_gt || !a->out || (a->edge_aware_smoothness && !a->depth)) {
    set_error("%s: NULL required pointer (args, rgb, rgb_gt, out; depth with edge_aware_smoothness)", who);
    return BTS_E_INVALID;
  }
  if (a->B <= 0 || a->n <= 0 || a->patch_h <= 0 || a->patch_w <= 0 || a->nv <= 0) {
    set_error("%s: non-positive size (B, n, patch_h, patch_w, nv)", who);
    return BTS_E_INVALID;
  }
  if (a->B > (1L << 29)) {
    set_error("%s: %ld rays are more than 2^29", who, (long)a->B);
    return BTS_E_INVALID;
  }
  if (a->B % ((long)a->n * a->patch_h * a->patch_w) != 0) {
    set_error("%s: B = %ld rays are not a multiple of n * patch_h * patch_w = %ld", who, (long)a->B, (long)a->n * a->patch_h * a->patch_w);
    return BTS_E_INVALID;
  }
  if (a->criterion != 1 && a->criterion != 2) {
    set_error("%s: unknown criterion %ld (1 = l1, 2 = l2)", who, (long)a->criterion);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy < 0 || a->invalid_policy > 3) {
    set_error("%s: unknown invalid_policy %ld", who, (long)a->invalid_policy);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy == 3 && !(a->rgb_samps && a->weights && a->invalid && a->K > 0)) {
    set_error("%s: weight_guided_diverse needs rgb_samps, weights and invalid with K > 0", who);
    return BTS_E_INVALID;
  }
  if (int rc = check_policy_inputs(a->invalid_policy, a->invalid_any, a->invalid_wsum, a->invalid, a->weights, a->K, who)) return rc;
  const size_t need = pixel_loss_bytes((long)a->B, a->n, a->patch_h, a->patch_w);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace too small (%ld bytes needed, see bts_pixel_loss_workspace)", who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(pixel_loss_impl(a, workspace, (hipStream_t)stream, thresh), who);
}
int bts_pixel_loss(const BtsPixelLossArgs* a, void* workspace, size_t workspace_bytes, void* stream) {
  return pixel_loss_entry(a, nullptr, workspace, workspace_bytes, stream, "bts_pixel_loss");
}
int bts_pixel_loss_automask(const BtsPixelLossArgs* a, const float* thresh, void* workspace, size_t workspace_bytes, void* stream) {
  static const char who[] = "bts_pixel_loss_automask";
  if (int rc = check_thresh(thresh, who)) return rc;
  return pixel_loss_entry(a, thresh, workspace, workspace_bytes, stream, who);
}
size_t bts_pixel_loss_channels_workspace(int64_t B) { return B > 0 && B <= (1L << 29) ? pixel_loss_channels_bytes((long)B) : 0; }
int bts_pixel_loss_channels(const BtsPixelLossArgs* a, int32_t channels, void* workspace, size_t workspace_bytes, void* stream) {
  static const char who[] = "bts_pixel_loss_channels";
  if (!a || !a->rgb || !a->rgb_gt || !a->out) {
    set_error("%s: NULL required pointer (args, rgb, rgb_gt, out)", who);
    return BTS_E_INVALID;
  }
  if (a->B <= 0 || a->nv <= 0) {
    set_error("%s: non-positive size (B, nv)", who);
    return BTS_E_INVALID;
  }
  if (a->B > (1L << 29)) {
    set_error("%s: %ld rays are more than 2^29", who, (long)a->B);
    return BTS_E_INVALID;
  }
  if (channels < 1 || channels > BTS_PIXEL_LOSS_MAX_CHANNELS) {
    set_error("%s: %ld channels are outside [1, %ld]", who, (long)channels, (long)BTS_PIXEL_LOSS_MAX_CHANNELS);
    return BTS_E_INVALID;
  }
  if (a->criterion != 1 && a->criterion != 2) {
    set_error("%s: unknown criterion %ld (1 = l1, 2 = l2)", who, (long)a->criterion);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy < 0 || a->invalid_policy > 3) {
    set_error("%s: unknown invalid_policy %ld", who, (long)a->invalid_policy);
    return BTS_E_INVALID;
  }
  if (a->median_thresholding || a->invalid_policy == 3 || a->edge_aware_smoothness) {
    set_error("%s: median_thresholding, weight_guided_diverse and edge_aware_smoothness are served for 3 channels only (bts_pixel_loss)", who);
    return BTS_E_UNSUPPORTED;
  }
  if (int rc = check_policy_inputs(a->invalid_policy, a->invalid_any, a->invalid_wsum, a->invalid, a->weights, a->K, who)) return rc;
  const size_t need = pixel_loss_channels_bytes((long)a->B);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace too small (%ld bytes needed, see bts_pixel_loss_channels_workspace)", who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(pixel_loss_channels_impl(a, channels, workspace, (hipStream_t)stream), who);
}
size_t bts_loss_regularisers_workspace(int64_t B, int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t K) {
  if (K < 2 || K > 256 || B > (1L << 29)) return 0;
  return loss_reg_bytes((long)B, n_patches, patch_h, patch_w, K);
}
int bts_loss_regularisers(const BtsLossRegArgs* a, void* workspace, size_t workspace_bytes, void* stream) {
  static const char who[] = "bts_loss_regularisers";
  const bool depth_on = a && a->coef_depth > 0.0f;
  const bool alpha_on = a && (a->coef_alpha_reg > 0.0f || a->coef_surfaceness > 0.0f || a->coef_entropy > 0.0f);
  if (!a || (alpha_on && !a->alphas) || !a->terms || !a->reg || (depth_on && !a->depth)) {
    set_error("%s: NULL required pointer (args, terms, reg; alphas with an alpha term, depth with the depth term)", who);
    return BTS_E_INVALID;
  }
  if (a->B <= 0 || a->n_patches <= 0 || a->patch_h <= 0 || a->patch_w <= 0 || a->K <= 0 || (a->invalid_policy != 0 && a->nv <= 0)) {
    set_error("%s: non-positive size (B, n_patches, patch_h, patch_w, K; nv with an invalid policy)", who);
    return BTS_E_INVALID;
  }
  if (a->K < 2 || a->K > 256) {
    set_error("%s: K = %ld samples per ray are outside [2, 256]", who, (long)a->K);
    return BTS_E_UNSUPPORTED;
  }
  if (depth_on && (a->patch_h < 2 || a->patch_w < 2)) {
    set_error("%s: the depth term needs patch_h >= 2 and patch_w >= 2, got %ld x %ld (the reference's mean of an empty tensor is NaN)", who,
              (long)a->patch_h, (long)a->patch_w);
    return BTS_E_UNSUPPORTED;
  }
  if (a->B != (int64_t)a->n_patches * a->patch_h * a->patch_w) {
    set_error("%s: B = %ld rays are not n_patches * patch_h * patch_w = %ld", who, (long)a->B, (long)a->n_patches * a->patch_h * a->patch_w);
    return BTS_E_INVALID;
  }
  if (a->B > (1L << 29)) {
    set_error("%s: %ld rays are more than 2^29", who, (long)a->B);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy < 0 || a->invalid_policy > 3) {
    set_error("%s: unknown invalid_policy %ld", who, (long)a->invalid_policy);
    return BTS_E_INVALID;
  }
  if (a->invalid_policy == 3 && !(a->rgb_samps && a->weights && a->invalid && a->K_invalid > 0)) {
    set_error("%s: weight_guided_diverse needs rgb_samps, weights and invalid with K_invalid > 0", who);
    return BTS_E_INVALID;
  }
  if (int rc = check_policy_inputs(a->invalid_policy, a->invalid_any, a->invalid_wsum, a->invalid, a->weights, a->K_invalid, who)) return rc;
  if ((a->g_alphas && !alpha_on) || (a->g_depth && !depth_on)) {
    set_error("%s: g_alphas needs an alpha term (alpha_reg, surfaceness, entropy) and g_depth the depth term with a coefficient > 0", who);
    return BTS_E_INVALID;
  }
  const size_t need = loss_reg_bytes((long)a->B, a->n_patches, a->patch_h, a->patch_w, a->K);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace too small (%ld bytes needed, see bts_loss_regularisers_workspace)", who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(loss_reg_impl(a, workspace, (hipStream_t)stream), who);
}
int bts_automask_errors(const float* images, int32_t n, int32_t v, int32_t H, int32_t W, const int32_t* ids_loss, int32_t n_loss, float scale,
                        float* errors, float* images4, void* stream) {
  static const char who[] = "bts_automask_errors";
  if (!images || !ids_loss) {
    set_error("%s: NULL images or ids_loss", who);
    return BTS_E_INVALID;
  }
  if (!errors && !images4) {
    set_error("%s: both outputs (errors, images4) are NULL", who);
    return BTS_E_INVALID;
  }
  if (n <= 0 || v <= 0 || H <= 0 || W <= 0) {
    set_error("%s: non-positive size (n, v, H, W)", who);
    return BTS_E_INVALID;
  }
  if (n_loss < 1 || n_loss > BTS_MAX_VIEWS) {
    set_error("%s: %ld loss frames are outside [1, BTS_MAX_VIEWS = %ld]", who, (long)n_loss, (long)BTS_MAX_VIEWS);
    return BTS_E_INVALID;
  }
  for (int j = 0; j < n_loss; ++j)
    if (ids_loss[j] < 0 || ids_loss[j] >= v) {
      set_error("%s: ids_loss[%ld] = %ld is outside [0, v = %ld)", who, (long)j, (long)ids_loss[j], (long)v);
      return BTS_E_INVALID;
    }
  if (automask_tiles(n, H, W) > 2147483647L) {
    set_error("%s: %ld frames of %ld x %ld pixels are more than 2^31 - 1 tiles", who, (long)n, (long)H, (long)W);
    return BTS_E_INVALID;
  }
  return launched(automask_errors_launch(images, n, v, H, W, ids_loss, n_loss, scale, errors, images4, (hipStream_t)stream), who);
}
int bts_loss_diverse_flags(const float* rgb_samps, const float* weights, const float* invalid, int64_t B, int32_t K, int32_t nv, float* flags,
                           void* stream) {
  BTS_CHECK_LAYOUT(rgb_samps && weights && invalid && flags && B > 0 && B <= (1L << 29) && K > 0 && nv > 0, "bts_loss_diverse_flags");
  return launched(diverse_flags_launch(rgb_samps, weights, invalid, (long)B, K, nv, flags, (hipStream_t)stream), "bts_loss_diverse_flags");
}
int bts_sample_coarse(const float* rays, const float* u, int64_t B, int32_t K, int32_t lindisp, float* z_samp, void* stream) {
  BTS_CHECK_LAYOUT(rays && u && z_samp && B > 0 && K > 0, "bts_sample_coarse");
  return launched(sample_coarse_launch(rays, u, (long)B, K, lindisp, z_samp, (hipStream_t)stream), "bts_sample_coarse");
}
int bts_sample_fine(const BtsSampleFineArgs* a, void* stream) {
  static const char who[] = "bts_sample_fine";
  if (!a) {
    set_error("%s: NULL args", who);
    return BTS_E_INVALID;
  }
  if (a->mode != BTS_SAMPLE_FINE && a->mode != BTS_SAMPLE_FROM_DIST) {
    set_error("%s: unknown mode %ld (BTS_SAMPLE_FINE = 0, BTS_SAMPLE_FROM_DIST = 1)", who, (long)a->mode);
    return BTS_E_INVALID;
  }
  const bool from_dist = a->mode == BTS_SAMPLE_FROM_DIST;
  if (a->B <= 0 || a->Kc <= 0 || (from_dist ? a->n_coarse <= 0 : (a->Kf <= 0 || a->Kfd < 0))) {
    set_error(from_dist ? "%s: non-positive size (B, ns, n_coarse)" : "%s: non-positive size (B, Kc, Kf; Kfd < 0)", who);
    return BTS_E_INVALID;
  }
  if (!from_dist && a->Kfd > a->Kf) {
    set_error("%s: Kfd = %ld depth draws are more than the Kf = %ld fine samples", who, (long)a->Kfd, (long)a->Kf);
    return BTS_E_INVALID;
  }
  if (from_dist && a->n_coarse > a->Kc) {
    set_error("%s: n_coarse = %ld samples from ns = %ld bins would index past the borders (the reference raises)", who, (long)a->n_coarse,
              (long)a->Kc);
    return BTS_E_INVALID;
  }
  const bool imp = from_dist || a->Kf > a->Kfd, dep = !from_dist && a->Kfd > 0, pieces = !from_dist && !a->z_coarse;
  if ((from_dist && !a->z_coarse) || (!from_dist && !a->rays) || (imp && (!a->weights || !a->u || !a->t)) || (dep && (!a->depth || !a->noise)) ||
      ((!pieces || imp) && !a->z_out) || (pieces && dep && !a->z_depth_out)) {
    set_error("%s: NULL required pointer (rays; weights, u, t with importance draws; depth, noise with depth draws; z_samp in from-dist mode; "
              "the outputs)", who);
    return BTS_E_INVALID;
  }
  if (a->Kc < 2 || (from_dist ? a->Kc : a->Kc + a->Kf) > 256) {
    set_error("%s: Kc = %ld, Kf = %ld are outside 2 <= Kc, Kc + Kf <= 256", who, (long)a->Kc, from_dist ? 0L : (long)a->Kf);
    return BTS_E_UNSUPPORTED;
  }
  if (a->B > (1L << 29)) {
    set_error("%s: %ld rays are more than 2^29", who, (long)a->B);
    return BTS_E_UNSUPPORTED;
  }
  return launched(sample_fine_launch(a, (hipStream_t)stream), who);
}
int bts_distance_to_z(const float* depths, const float* inv_K, int32_t N, int32_t H, int32_t W, float* out, void* stream) {
  BTS_CHECK_LAYOUT(depths && inv_K && out && N > 0 && H > 0 && W > 0, "bts_distance_to_z");
  return launched(distance_to_z_launch(depths, inv_K, N, H, W, out, (hipStream_t)stream), "bts_distance_to_z");
}

int bts_invert_small(const float* src, float* dst, int32_t N, int32_t dim, void* stream) {
  BTS_CHECK_LAYOUT(src && dst && N > 0 && (dim == 3 || dim == 4), "bts_invert_small");
  return launched(invert_small_launch(src, dst, N, dim, (hipStream_t)stream), "bts_invert_small");
}

// ---- MLP-predicted colour (sample_color=False): the field checks of check_cfg plus this head's own (nv = 1, no render view, G required)
static int check_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const char* who) {
  if (!cfg || !t) {
    set_error("%s: NULL cfg/tensors", who);
    return BTS_E_INVALID;
  }
  if (cfg->nv != 1) {
    set_error("%s: nv=%ld, but MLP-predicted colour has exactly one colour output (nv = 1, models_bts.py:321)", who, (long)cfg->nv);
    return BTS_E_INVALID;
  }
  if (cfg->enc_render_view != -1) {
    set_error("%s: enc_render_view=%ld must be -1 (this head has no render views)", who, (long)cfg->enc_render_view);
    return BTS_E_INVALID;
  }
  if (int rc = check_cfg(cfg, t, false)) return rc;
  if (!t->proj_nhwc) {
    set_error("%s: the projected feature map (proj_nhwc) is required", who);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}

// The render arguments of the two lane = sample families (bts_mc_field.h).  kernels, family: how the texts name the caller's ("this head's" /
// "MLP-predicted colour", "the merged-view" / "merged encoder views")
static int check_lane_sample_args(const BtsRenderArgs* a, const char* who, bool bwd, const char* kernels, const char* family) {
  if (int rc = check_render_args(a, who, bwd, true, bwd ? "%s: NULL argument (rays, z_samp and the forward's sigma_raw + trans are required)" : kFwdArgsNull))
    return rc;
  // set_error takes one string and up to three longs, so the family's words go into the format itself (they are literals of this file,
  // without a '%', and the longest format stays well inside the buffer); the compiler does not check these two formats
  char fmt[192];
  if (a->K > 256) {
    snprintf(fmt, sizeof(fmt), "%%s: K=%%ld samples per ray; %s kernels take whole rays of at most 256 samples per work-group", kernels);
    set_error(fmt, who, (long)a->K);
    return BTS_E_UNSUPPORTED;
  }
  if (!bwd && (a->invalid_wsum || a->invalid_any)) {
    snprintf(fmt, sizeof(fmt), "%%s: invalid_wsum / invalid_any are not produced for %s (request weights and invalid)", family);
    set_error(fmt, who);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}
static int check_mlp_color_args(const BtsRenderArgs* a, const char* who, bool bwd) {
  return check_lane_sample_args(a, who, bwd, "this head's", "MLP-predicted colour");
}

// what a backward entry of the two families checks behind its field and arguments: the gradient struct and the workspace (need bytes)
static int check_bwd_call(const BtsRenderGrads* g, const void* workspace, size_t workspace_bytes, size_t need, const char* who) {
  if (!g) {
    set_error("%s: NULL gradient struct", who);
    return BTS_E_INVALID;
  }
  if (workspace_bytes < need || !workspace) {
    set_error("%s: workspace too small (%ld bytes needed)", who, (long)need);
    return BTS_E_WORKSPACE;
  }
  return BTS_OK;
}

int64_t bts_mlp_color_param_count(const BtsFieldCfg* cfg) {
  if (!cfg) {
    set_error("%s: NULL cfg", "bts_mlp_color_param_count");
    return -1;
  }
  return bts_mlp_param_count(cfg) + 3 * (int64_t)cfg->d_hidden + 3;
}

int bts_render_fwd_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, void* stream) {
  if (int rc = check_mlp_color(cfg, t, "bts_render_fwd_mlp_color")) return rc;
  if (int rc = check_mlp_color_args(a, "bts_render_fwd_mlp_color", false)) return rc;
  return mlp_color_render_fwd_impl(cfg, t, a, (hipStream_t)stream);
}

size_t bts_render_bwd_mlp_color_workspace(const BtsFieldCfg* cfg, const BtsRenderArgs* a) {
  if (!cfg || !a || cfg->n <= 0 || a->rays_per_sample <= 0 || a->K <= 0 || cfg->d_hidden <= 0) return 0;
  return mlp_color_bwd_workspace_impl(cfg, a);
}

int bts_render_bwd_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_mlp_color(cfg, t, "bts_render_bwd_mlp_color")) return rc;
  if (int rc = check_mlp_color_args(a, "bts_render_bwd_mlp_color", true)) return rc;
  if (int rc = check_bwd_call(g, workspace, workspace_bytes, mlp_color_bwd_workspace_impl(cfg, a), "bts_render_bwd_mlp_color")) return rc;
  return mlp_color_render_bwd_impl(cfg, t, a, g, workspace, (hipStream_t)stream);
}

int bts_field_query_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t P, int32_t only_density,
                              float* rgb, float* invalid, float* sigma, void* stream) {
  if (int rc = check_mlp_color(cfg, t, "bts_field_query_mlp_color")) return rc;
  if (!xyz || !sigma || P <= 0 || (!only_density && !rgb)) {
    set_error("%s: NULL/empty query argument (P=%ld)", "bts_field_query_mlp_color", (long)P);
    return BTS_E_INVALID;
  }
  return mlp_color_field_query_impl(cfg, t, xyz, P, only_density, rgb, invalid, sigma, (hipStream_t)stream);
}

// ---- merged encoder views: everything bts_multi_view.hip's kernels index with is checked here; a bad table never reaches a launch
static int check_group_table(const int32_t* start, const int32_t* member, int n_groups, int n_views, const char* who) {
  if (n_groups < 1 || n_groups > BTS_MV_MAX_VIEWS) {
    set_error("%s: %ld groups; 1 .. 8 are supported", who, (long)n_groups);
    return BTS_E_INVALID;
  }
  if (start[0] != 0) {
    set_error("%s: a group table must start at member 0 (got %ld)", who, (long)start[0]);
    return BTS_E_INVALID;
  }
  unsigned seen = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (start[g + 1] <= start[g]) {
      set_error("%s: group %ld is empty (or the table runs backwards)", who, (long)g);
      return BTS_E_INVALID;
    }
    if (start[g + 1] > BTS_MV_MAX_VIEWS) {
      set_error("%s: group %ld runs past the table's 8 members", who, (long)g);
      return BTS_E_INVALID;
    }
    for (int m = start[g]; m < start[g + 1]; ++m) {
      if (member[m] < 0 || member[m] >= n_views) {
        set_error("%s: member %ld of group %ld is not one of the %ld views", who, (long)member[m], (long)g, (long)n_views);
        return BTS_E_INVALID;
      }
      if (seen & (1u << member[m])) {
        set_error("%s: view %ld is a member of two groups", who, (long)member[m]);
        return BTS_E_INVALID;
      }
      seen |= 1u << member[m];
    }
  }
  return BTS_OK;
}

static int check_multi_view(const BtsMultiViewField* mv, const char* who) {
  if (!mv) {
    set_error("%s: NULL field", who);
    return BTS_E_INVALID;
  }
  if (mv->V < 1 || mv->V > BTS_MV_MAX_VIEWS) {
    set_error("%s: V=%ld encoder views; 1 .. 8 are supported", who, (long)mv->V);
    return BTS_E_INVALID;
  }
  const BtsFieldCfg* c0 = &mv->cfg[0];
  if (c0->nv < 1 || c0->nv > BTS_MAX_VIEWS) {
    set_error("%s: nv=%ld render views; 1 .. 8 are supported", who, (long)c0->nv);
    return BTS_E_INVALID;
  }
  if (int rc = check_group_table(mv->enc_group_start, mv->enc_member, mv->n_enc_groups, mv->V, who)) return rc;
  if (int rc = check_group_table(mv->ren_group_start, mv->ren_member, mv->n_ren_groups, c0->nv, who)) return rc;
  for (int g = 0; g < mv->n_enc_groups; ++g)
    if (mv->enc_mult[g] != 1 && mv->enc_mult[g] != 2) {
      set_error("%s: encoder group %ld has multiplicity %ld; 1 or 2 expected", who, (long)g, (long)mv->enc_mult[g]);
      return BTS_E_INVALID;
    }
  for (int v = 1; v < mv->V; ++v) {
    const BtsFieldCfg* c = &mv->cfg[v];
    if (c->n != c0->n || c->C != c0->C || c->d_hidden != c0->d_hidden || c->n_blocks != c0->n_blocks || c->H != c0->H || c->W != c0->W ||
        c->feat_shift != c0->feat_shift || c->tile_blocks != c0->tile_blocks) {
      set_error("%s: encoder view %ld differs from view 0 in n / C / d_hidden / n_blocks / H / W / feat_shift / tile_blocks", who, (long)v);
      return BTS_E_UNSUPPORTED;
    }
  }
  if (int rc = check_cfg(c0, &mv->view[0], true)) return rc;
  for (int v = 0; v < mv->V; ++v)
    if (!mv->view[v].proj_nhwc || !mv->view[v].K_enc || !mv->view[v].w2c_enc) {
      set_error("%s: encoder view %ld: proj_nhwc, K_enc and w2c_enc are required", who, (long)v);
      return BTS_E_INVALID;
    }
  return BTS_OK;
}

static int check_multi_view_args(const BtsRenderArgs* a, const char* who, bool bwd) {
  return check_lane_sample_args(a, who, bwd, "the merged-view", "merged encoder views");
}

int bts_render_fwd_multi_view(const BtsMultiViewField* mv, const BtsRenderArgs* a, void* stream) {
  if (int rc = check_multi_view(mv, "bts_render_fwd_multi_view")) return rc;
  if (int rc = check_multi_view_args(a, "bts_render_fwd_multi_view", false)) return rc;
  return multi_view_render_fwd_impl(mv, a, (hipStream_t)stream);
}

size_t bts_render_bwd_multi_view_workspace(const BtsMultiViewField* mv, const BtsRenderArgs* a) {
  if (!mv || !a || mv->V < 1 || mv->V > BTS_MV_MAX_VIEWS || mv->cfg[0].n <= 0 || a->rays_per_sample <= 0 || a->K <= 0 || mv->cfg[0].d_hidden <= 0)
    return 0;
  return multi_view_bwd_workspace_impl(mv, a);
}

int bts_render_bwd_multi_view(const BtsMultiViewField* mv, const BtsRenderArgs* a, const BtsRenderGrads* g, float* const* d_proj_views,
                              unsigned char* const* d_proj_tiles_views, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_multi_view(mv, "bts_render_bwd_multi_view")) return rc;
  if (int rc = check_multi_view_args(a, "bts_render_bwd_multi_view", true)) return rc;
  if (int rc = check_bwd_call(g, workspace, workspace_bytes, multi_view_bwd_workspace_impl(mv, a), "bts_render_bwd_multi_view")) return rc;
  return multi_view_render_bwd_impl(mv, a, g, d_proj_views, d_proj_tiles_views, workspace, (hipStream_t)stream);
}

int bts_field_query_multi_view(const BtsMultiViewField* mv, const float* xyz, int32_t P, float* rgb, float* invalid, float* sigma,
                               void* stream) {
  if (int rc = check_multi_view(mv, "bts_field_query_multi_view")) return rc;
  if (!xyz || !sigma || P <= 0) {
    set_error("%s: NULL/empty query argument (P=%ld)", "bts_field_query_multi_view", (long)P);
    return BTS_E_INVALID;
  }
  return multi_view_field_query_impl(mv, xyz, P, rgb, invalid, sigma, (hipStream_t)stream);
}

// ---- LiDAR occupancy evaluation (evaluator_lidar.py): limits and host-side checks shared by the three entry points
static int check_lidar_limits(int T, int y_res, const char* who) {
  if (T <= 0 || y_res <= 0) {
    set_error("%s: non-positive T=%ld / y_res=%ld", who, (long)T, (long)y_res);
    return BTS_E_INVALID;
  }
  if (T > BTS_LIDAR_MAX_CLOUDS || y_res > BTS_LIDAR_MAX_SLICES) {
    set_error("%s: T=%ld clouds / y_res=%ld slices; at most 32 clouds and 16 slices are supported", who, (long)T, (long)y_res);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}

static int check_lidar_clouds(const float* points, const int32_t* offsets, int T, const char* who) {
  if (((uintptr_t)points & 15) != 0) {
    set_error("%s: points must be 16-byte aligned", who);
    return BTS_E_INVALID;
  }
  if (offsets[0] != 0) {
    set_error("%s: offsets[0]=%ld must be 0", who, (long)offsets[0]);
    return BTS_E_INVALID;
  }
  for (int t = 0; t < T; ++t)
    if (offsets[t + 1] < offsets[t]) {
      set_error("%s: offsets are not monotone at cloud %ld (%ld after %ld)", who, (long)t, (long)offsets[t + 1], (long)offsets[t]);
      return BTS_E_INVALID;
    }
  for (int t = 0; t < T; ++t)
    if (offsets[t + 1] - offsets[t] < 360) {
      set_error("%s: cloud %ld has %ld points; the reference's tables need at least 360 selected points per slice and cloud", who, (long)t,
                (long)(offsets[t + 1] - offsets[t]));
      return BTS_E_UNSUPPORTED;
    }
  return BTS_OK;
}

size_t bts_lidar_slices_workspace(int32_t T, int32_t y_res) {
  if (T <= 0 || y_res <= 0 || T > BTS_LIDAR_MAX_CLOUDS || y_res > BTS_LIDAR_MAX_SLICES) return 0;
  return lidar_bins_bytes(T, y_res);
}

int bts_lidar_slices(const float* points, const int32_t* offsets, int32_t T, const float* velo_poses, const float* borders361, float y_lo,
                     float y_hi, int32_t y_res, float max_dist, void* bins_workspace, float* tables, void* stream) {
  BTS_CHECK_LAYOUT(points && offsets && velo_poses && borders361 && bins_workspace && tables, "bts_lidar_slices");
  if (int rc = check_lidar_limits(T, y_res, "bts_lidar_slices")) return rc;
  if (int rc = check_lidar_clouds(points, offsets, T, "bts_lidar_slices")) return rc;
  return launched(lidar_slices_launch(points, offsets, T, velo_poses, borders361, y_lo, y_hi, y_res, max_dist, bins_workspace, tables,
                                      (hipStream_t)stream),
                  "bts_lidar_slices");
}

int bts_lidar_occupancy(const float* q_pts, int32_t P, const float* tables, int32_t y_res, int32_t T, const float* world_to_velo,
                        float min_dist, uint8_t* is_occupied, uint8_t* is_visible, void* stream) {
  BTS_CHECK_LAYOUT(q_pts && tables && world_to_velo && is_occupied && is_visible && P > 0, "bts_lidar_occupancy");
  if (int rc = check_lidar_limits(T, y_res, "bts_lidar_occupancy")) return rc;
  return launched(lidar_occupancy_launch(q_pts, P, tables, y_res, T, world_to_velo, min_dist, is_occupied, is_visible, (hipStream_t)stream),
                  "bts_lidar_occupancy");
}

// workspace of bts_occupancy_eval: bts_occ.hip's occ_eval_layout
size_t bts_occupancy_eval_workspace(int32_t P, int32_t T, int32_t y_res) {
  if (P <= 0 || T <= 0 || y_res <= 0 || T > BTS_LIDAR_MAX_CLOUDS || y_res > BTS_LIDAR_MAX_SLICES) return 0;
  Carver count(nullptr);
  occ_eval_layout(count, P, T, y_res);
  return count.bytes();
}

int bts_occupancy_eval(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsOccupancyEval* a, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (int rc = check_cfg(cfg, t, false)) return rc;
  BTS_CHECK_LAYOUT(a && a->q_pts && a->points && a->offsets && a->velo_poses && a->borders361 && a->pred_depth_z && a->proj && a->cam_pose &&
                       a->counts && a->P > 0 && a->H > 0 && a->W > 0,
                   "bts_occupancy_eval");
  if (cfg->n != 1) {
    set_error("%s: n=%ld; the evaluator queries one encoded sample (n = 1)", "bts_occupancy_eval", (long)cfg->n);
    return BTS_E_INVALID;
  }
  if (int rc = check_lidar_limits(a->T, a->y_res, "bts_occupancy_eval")) return rc;
  if (int rc = check_lidar_clouds(a->points, a->offsets, a->T, "bts_occupancy_eval")) return rc;
  const size_t need = bts_occupancy_eval_workspace(a->P, a->T, a->y_res);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace too small or not 16-byte aligned (%ld bytes needed)", "bts_occupancy_eval", (long)need);
    return BTS_E_WORKSPACE;
  }
  const int P = a->P, T = a->T, y_res = a->y_res;
  hipStream_t s = (hipStream_t)stream;
  Carver carve(workspace);
  const OccEvalWs w = occ_eval_layout(carve, P, T, y_res);
  float* tables = a->tables ? a->tables : w.tables;
  float* sigma = a->sigma ? a->sigma : w.sigma;

  if (int rc = field_query_impl(cfg, t, a->q_pts, P, 1, nullptr, nullptr, sigma, s)) return rc;
  int rc = invert_small_launch(a->velo_poses, w.w2v, T, 4, s);
  if (!rc) rc = invert_small_launch(a->cam_pose, w.w2c, 1, 4, s);
  if (!rc) rc = lidar_slices_launch(a->points, a->offsets, T, a->velo_poses, a->borders361, a->y_lo, a->y_hi, y_res, a->max_dist, w.bins, tables, s);
  if (!rc) rc = lidar_occupancy_launch(a->q_pts, P, tables, y_res, T, w.w2v, a->min_dist, w.is_occ, w.is_vis, s);
  if (!rc) rc = occ_metrics_launch(a->q_pts, P, sigma, w.is_occ, w.is_vis, a->pred_depth_z, a->H, a->W, a->proj, w.w2c, a->occ_threshold, a->counts, a->masks, s);
  if (rc) set_error("%s: kernel launch failed", "bts_occupancy_eval");
  return rc;
}

// ---- depth evaluation metrics (evaluator.py:96-151)
static bool depth_metrics_sizes_ok(long B, long H, long W, long Hg, long Wg, int mode) {
  const long max_px = 1L << 30;
  return B > 0 && B <= BTS_DEPTH_METRICS_MAX_FRAMES && H > 0 && W > 0 && Hg > 0 && Wg > 0 && H * W <= max_px && Hg * Wg <= max_px && mode >= 0 &&
         mode <= 2;
}

size_t bts_depth_metrics_workspace(int32_t B, int32_t Hg, int32_t Wg, int32_t mode) {
  if (!depth_metrics_sizes_ok(B, 1, 1, Hg, Wg, mode)) return 0;
  return depth_metrics_bytes(B, Hg, Wg);
}

int bts_depth_metrics(const BtsDepthMetrics* a, void* workspace, size_t workspace_bytes, void* stream) {
  BTS_CHECK_LAYOUT(a && a->pred && a->gt && a->metrics && a->B > 0 && a->H > 0 && a->W > 0 && a->Hg > 0 && a->Wg > 0, "bts_depth_metrics");
  if (a->B > BTS_DEPTH_METRICS_MAX_FRAMES) {
    set_error("%s: B=%ld frames; at most 64 per call", "bts_depth_metrics", (long)a->B);
    return BTS_E_INVALID;
  }
  if (a->mode < 0 || a->mode > 2) {
    set_error("%s: unknown mode %ld (0 none, 1 median, 2 l2)", "bts_depth_metrics", (long)a->mode);
    return BTS_E_INVALID;
  }
  if (!depth_metrics_sizes_ok(a->B, a->H, a->W, a->Hg, a->Wg, a->mode)) {
    set_error("%s: more than 2^30 pixels per frame (pred %ld, gt %ld)", "bts_depth_metrics", (long)a->H * a->W, (long)a->Hg * a->Wg);
    return BTS_E_INVALID;
  }
  const size_t need = depth_metrics_bytes(a->B, a->Hg, a->Wg);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace NULL, too small or not 16-byte aligned (%ld bytes needed)", "bts_depth_metrics", (long)need);
    return BTS_E_INVALID;
  }
  return launched(depth_metrics_launch(a, workspace, (hipStream_t)stream), "bts_depth_metrics");
}

// ---- NVS evaluation metrics (evaluator_nvs.py:141-178 without LPIPS)
static bool nvs_metrics_sizes_ok(long B, long H, long W, long He, long We) {
  const long max_px = 1L << 30;
  return B > 0 && B <= BTS_NVS_METRICS_MAX_FRAMES && H > 0 && W > 0 && He > 0 && We > 0 && H * W <= max_px && He * We <= max_px;
}

size_t bts_nvs_metrics_workspace(int32_t B, int32_t He, int32_t We) {
  if (!nvs_metrics_sizes_ok(B, 1, 1, He, We)) return 0;
  return nvs_metrics_bytes(B, He, We);
}

int bts_nvs_metrics(const BtsNvsMetrics* a, void* workspace, size_t workspace_bytes, void* stream) {
  BTS_CHECK_LAYOUT(a && a->pred && a->gt && a->metrics && a->B > 0 && a->H > 0 && a->W > 0 && a->He > 0 && a->We > 0, "bts_nvs_metrics");
  if (a->B > BTS_NVS_METRICS_MAX_FRAMES) {
    set_error("%s: B=%ld frames; at most 64 per call", "bts_nvs_metrics", (long)a->B);
    return BTS_E_INVALID;
  }
  if (!nvs_metrics_sizes_ok(a->B, a->H, a->W, a->He, a->We)) {
    set_error("%s: more than 2^30 pixels per frame (source %ld, eval_resolution %ld)", "bts_nvs_metrics", (long)a->H * a->W, (long)a->He * a->We);
    return BTS_E_INVALID;
  }
  if (a->y0 < 0 || a->x0 < 0 || a->y1 > a->He || a->x1 > a->We || a->y1 < a->y0 || a->x1 < a->x0) {
    set_error("%s: the crop box leaves eval_resolution (%ld x %ld)", "bts_nvs_metrics", (long)a->He, (long)a->We);
    return BTS_E_INVALID;
  }
  if (a->y1 - a->y0 < 7 || a->x1 - a->x0 < 7) {
    set_error("%s: crop of %ld x %ld pixels; a side below the 7-pixel window", "bts_nvs_metrics", (long)(a->y1 - a->y0), (long)(a->x1 - a->x0));
    return BTS_E_INVALID;
  }
  if (!(a->data_range > 0.0)) {
    set_error("%s: data_range must be positive", "bts_nvs_metrics");
    return BTS_E_INVALID;
  }
  const size_t need = nvs_metrics_bytes(a->B, a->He, a->We);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace NULL, too small or not 16-byte aligned (%ld bytes needed)", "bts_nvs_metrics", (long)need);
    return BTS_E_INVALID;
  }
  return launched(nvs_metrics_launch(a, workspace, (hipStream_t)stream), "bts_nvs_metrics");
}

// ---- 3D-bounding-box occupancy evaluation (evaluator_3dbb.py): limits and host-side checks shared by the entry points
static int check_bbox_boxes(const int32_t* v_offsets, const int32_t* f_offsets, int B, const char* who) {
  if (B > BTS_BBOX_MAX_BOXES) {
    set_error("%s: B=%ld boxes; at most 4096 are supported", who, (long)B);
    return BTS_E_UNSUPPORTED;
  }
  if (v_offsets[0] != 0 || f_offsets[0] != 0) {
    set_error("%s: offsets[0] must be 0 (vertices %ld, faces %ld)", who, (long)v_offsets[0], (long)f_offsets[0]);
    return BTS_E_INVALID;
  }
  for (int b = 0; b < B; ++b)
    if (v_offsets[b + 1] <= v_offsets[b] || f_offsets[b + 1] <= f_offsets[b]) {
      set_error("%s: offsets are not monotone at box %ld (a box needs at least one vertex and one face)", who, (long)b);
      return BTS_E_INVALID;
    }
  for (int b = 0; b < B; ++b)
    if (v_offsets[b + 1] - v_offsets[b] > BTS_BBOX_MAX_VERTS || f_offsets[b + 1] - f_offsets[b] > BTS_BBOX_MAX_FACES) {
      set_error("%s: box %ld has %ld vertices / %ld faces; at most 64 vertices and 32 faces per box are supported", who, (long)b,
                (long)(v_offsets[b + 1] - v_offsets[b]), (long)(f_offsets[b + 1] - f_offsets[b]));
      return BTS_E_UNSUPPORTED;
    }
  return BTS_OK;
}

static bool bbox_grid_ok(long ph, long pw, long hs, long ws) {
  const long max_px = 1L << 27;   // ray r reads floats 8 r + 3 .. 8 r + 5
  return ph > 0 && pw > 0 && hs > 0 && ws > 0 && ph * pw <= max_px && hs * ws <= (1L << 30);
}

int bts_bbox_bounds(const float* vertices, const int32_t* faces, const int32_t* v_offsets, const int32_t* f_offsets, int32_t B,
                    const float* to_keyframe, const float* proj, float max_d, float* tables, int32_t* n_faces, uint8_t* active, void* stream) {
  BTS_CHECK_LAYOUT(vertices && faces && v_offsets && f_offsets && to_keyframe && proj && tables && n_faces && active && B > 0, "bts_bbox_bounds");
  if (int rc = check_bbox_boxes(v_offsets, f_offsets, B, "bts_bbox_bounds")) return rc;
  return launched(bbox_bounds_launch(vertices, faces, v_offsets, f_offsets, B, to_keyframe, proj, max_d, tables, n_faces, active, nullptr,
                                     (hipStream_t)stream),
                  "bts_bbox_bounds");
}

int bts_bbox_pseudo_depth(const float* rays, int32_t ph, int32_t pw, const float* seg, int32_t hs, int32_t ws, const float* tables,
                          const int32_t* n_faces, const uint8_t* active, const float* semantic_id, int32_t B, float* pseudo_depth, void* stream) {
  BTS_CHECK_LAYOUT(rays && seg && tables && n_faces && active && semantic_id && pseudo_depth && B > 0 && ph > 0 && pw > 0 && hs > 0 && ws > 0,
                   "bts_bbox_pseudo_depth");
  if (B > BTS_BBOX_MAX_BOXES) {
    set_error("%s: B=%ld boxes; at most 4096 are supported", "bts_bbox_pseudo_depth", (long)B);
    return BTS_E_UNSUPPORTED;
  }
  if (!bbox_grid_ok(ph, pw, hs, ws)) {
    set_error("%s: more than 2^27 rays or 2^30 label pixels (%ld, %ld)", "bts_bbox_pseudo_depth", (long)ph * pw, (long)hs * ws);
    return BTS_E_INVALID;
  }
  return launched(bbox_pseudo_depth_launch(rays, ph, pw, seg, hs, ws, tables, n_faces, active, semantic_id, B, pseudo_depth, (hipStream_t)stream),
                  "bts_bbox_pseudo_depth");
}

// workspace of bts_bbox_occupancy_eval: bts_bbox_occ.hip's bbox_eval_layout
size_t bts_bbox_occupancy_eval_workspace(int32_t P, int32_t B, int32_t ph, int32_t pw) {
  if (P <= 0 || B <= 0 || B > BTS_BBOX_MAX_BOXES || !bbox_grid_ok(ph, pw, 1, 1)) return 0;
  Carver count(nullptr);
  bbox_eval_layout(count, P, B, ph, pw);
  return count.bytes();
}

int bts_bbox_occupancy_eval(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsBBoxOccupancyEval* a, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (int rc = check_cfg(cfg, t, false)) return rc;
  BTS_CHECK_LAYOUT(a && a->q_pts && a->vertices && a->faces && a->v_offsets && a->f_offsets && a->semantic_id && a->rays && a->seg &&
                       a->pred_depth_z && a->proj && a->cam_pose && a->counts && a->P > 0 && a->B > 0 && a->ph > 0 && a->pw > 0 && a->hs > 0 &&
                       a->ws > 0,
                   "bts_bbox_occupancy_eval");
  if (cfg->n != 1) {
    set_error("%s: n=%ld; the evaluator queries one encoded sample (n = 1)", "bts_bbox_occupancy_eval", (long)cfg->n);
    return BTS_E_INVALID;
  }
  if (int rc = check_bbox_boxes(a->v_offsets, a->f_offsets, a->B, "bts_bbox_occupancy_eval")) return rc;
  if (!bbox_grid_ok(a->ph, a->pw, a->hs, a->ws)) {
    set_error("%s: more than 2^27 rays or 2^30 label pixels (%ld, %ld)", "bts_bbox_occupancy_eval", (long)a->ph * a->pw, (long)a->hs * a->ws);
    return BTS_E_INVALID;
  }
  const size_t need = bts_bbox_occupancy_eval_workspace(a->P, a->B, a->ph, a->pw);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace too small or not 16-byte aligned (%ld bytes needed)", "bts_bbox_occupancy_eval", (long)need);
    return BTS_E_WORKSPACE;
  }
  const int P = a->P, B = a->B;
  hipStream_t s = (hipStream_t)stream;
  Carver carve(workspace);
  const BBoxEvalWs w = bbox_eval_layout(carve, P, B, a->ph, a->pw);
  float* tables = a->tables ? a->tables : w.tables;
  float* pseudo = a->pseudo_depth ? a->pseudo_depth : w.pseudo;
  float* sigma = a->sigma ? a->sigma : w.sigma;

  if (int rc = field_query_impl(cfg, t, a->q_pts, P, 1, nullptr, nullptr, sigma, s)) return rc;
  if (hipMemsetAsync(a->counts, 0, 7 * sizeof(int32_t), s) != hipSuccess) {
    (void)launch_code();
    set_error("%s: kernel launch failed", "bts_bbox_occupancy_eval");
    return BTS_E_LAUNCH;
  }
  int rc = invert_small_launch(a->cam_pose, w.to_key, 1, 4, s);
  if (!rc) rc = bbox_bounds_launch(a->vertices, a->faces, a->v_offsets, a->f_offsets, B, w.to_key, a->proj, a->max_d, tables, w.n_faces, w.active,
                                   a->counts + 6, s);
  if (!rc) rc = bbox_pseudo_depth_launch(a->rays, a->ph, a->pw, a->seg, a->hs, a->ws, tables, w.n_faces, w.active, a->semantic_id, B, pseudo, s);
  if (!rc) rc = bbox_metrics_launch(a->q_pts, P, sigma, pseudo, a->pred_depth_z, a->ph, a->pw, a->proj, tables, w.n_faces, w.active, B,
                                    a->occ_threshold, a->counts, a->masks, s);
  if (rc) set_error("%s: kernel launch failed", "bts_bbox_occupancy_eval");
  return rc;
}

// ---- novel-view frames and colour-mapped depth (scripts/inference_setup.py:182-198, utils/plotting.py:41-46)
static int check_panel(const char* who, int depth_panel, long h, long w, long Hc, long Wc, long row0, long col0) {
  if (row0 < 0 || col0 < 0 || row0 + h > Hc || col0 + w > Wc) {
    set_error(depth_panel ? "%s: the depth panel at (%ld, %ld) leaves the canvas" : "%s: the panel at (%ld, %ld) leaves the canvas", who, row0, col0);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}
static bool frames_sizes_ok(long B, long h, long w) { return B > 0 && B <= 65535 && h > 0 && w > 0 && h * w <= (1L << 30); }

int bts_colorize(const float* x, int32_t B, int32_t h, int32_t w, int32_t norm, int32_t N, const double* lut_f64, const uint8_t* lut_u8,
                 float* minmax_scratch, double* out, uint8_t* canvas, int32_t Hc, int32_t Wc, int32_t row0, int32_t col0, void* stream) {
  BTS_CHECK_LAYOUT(x && B > 0 && h > 0 && w > 0 && (out || canvas) && (!out || lut_f64) && (!canvas || lut_u8) && (!norm || minmax_scratch),
                   "bts_colorize");
  if (!frames_sizes_ok(B, h, w) || N < 1 || N > BTS_CMAP_MAX_N) {
    set_error("%s: more than 65535 images, more than 2^30 pixels per image, or a table of N=%ld outside [1, 65536]", "bts_colorize", (long)N);
    return BTS_E_INVALID;
  }
  if (canvas)
    if (int rc = check_panel("bts_colorize", 0, h, w, Hc, Wc, row0, col0)) return rc;
  return launched(colorize_launch(x, B, h, w, norm, N, lut_f64, lut_u8, minmax_scratch, out, canvas, Hc, Wc, row0, col0, (hipStream_t)stream),
                  "bts_colorize");
}

int bts_pack_u8(const float* x, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t h, int32_t w, float scale, float shift,
                uint8_t* canvas, int32_t Hc, int32_t Wc, int32_t row0, int32_t col0, void* stream) {
  BTS_CHECK_LAYOUT(x && canvas && B > 0 && h > 0 && w > 0, "bts_pack_u8");
  if (!frames_sizes_ok(B, h, w)) {
    set_error("%s: more than 65535 images or more than 2^30 pixels per image", "bts_pack_u8");
    return BTS_E_INVALID;
  }
  if (int rc = check_panel("bts_pack_u8", 0, h, w, Hc, Wc, row0, col0)) return rc;
  return launched(pack_u8_launch(x, (long)sb, (long)sy, (long)sx, (long)sc, B, h, w, scale, shift, canvas, Hc, Wc, row0, col0, (hipStream_t)stream),
                  "bts_pack_u8");
}

int bts_novel_views(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsNovelViews* a, void* stream) {
  const char* who = "bts_novel_views";
  BTS_CHECK_LAYOUT(a && a->P > 0 && a->h > 0 && a->w > 0 && a->rgb && a->depth && a->invalid_wsum, who);
  if (!frames_sizes_ok(a->P, a->h, a->w) || (long)a->P * a->h * a->w > (1L << 30)) {
    set_error("%s: more than 65535 poses or more than 2^30 rays per chunk", who);
    return BTS_E_INVALID;
  }
  if (a->black_invalid && !a->frame_max) {
    set_error("%s: black_invalid needs the frame_max scratch", who);
    return BTS_E_INVALID;
  }
  const bool img = a->canvas && a->img_row0 >= 0, dep = a->canvas && a->depth_row0 >= 0;
  if (img)
    if (int rc = check_panel(who, 0, a->h, a->w, a->Hc, a->Wc, a->img_row0, a->img_col0)) return rc;
  if (dep) {
    if (int rc = check_panel(who, 1, a->h, a->w, a->Hc, a->Wc, a->depth_row0, a->depth_col0)) return rc;
    if (!a->lut_u8 || !a->norm_range || a->lut_N < 1 || a->lut_N > BTS_CMAP_MAX_N) {
      set_error("%s: the depth panel needs lut_u8, norm_range and 1 <= lut_N <= 65536 (got %ld)", who, (long)a->lut_N);
      return BTS_E_INVALID;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (!a->finish_only) {
    if (int rc = check_cfg(cfg, t, true)) return rc;
    if (cfg->n != 1 || cfg->nv != 1) {
      set_error("%s: n=%ld, nv=%ld; a chunk of novel views renders from ONE encoded sample with ONE colour view (ids_encoder=[0], ids_render=[0])",
                who, (long)cfg->n, (long)cfg->nv);
      return BTS_E_UNSUPPORTED;
    }
    if (!t->proj_nhwc) {
      set_error("%s: the projected feature map (proj_nhwc) is required (sampling inside the kernel, the invalid_wsum epilogue)", who);
      return BTS_E_UNSUPPORTED;
    }
    if (!a->poses_c2w || !a->Ks || !a->near_far || !a->jitter || !a->rays || a->K <= 0) {
      set_error("%s: NULL pointer or non-positive K (poses_c2w, Ks, near_far, jitter and the rays scratch are required)", who);
      return BTS_E_INVALID;
    }
    if (gen_rays_nf_launch(a->poses_c2w, a->Ks, a->near_far, a->P, a->h, a->w, a->norm_dir, a->rays, s)) {
      set_error("%s: kernel launch failed", who);
      return BTS_E_LAUNCH;
    }
    BtsRenderArgs r;
    memset(&r, 0, sizeof(r));
    r.rays_per_sample = a->P * a->h * a->w, r.K = a->K, r.hard_alpha_cap = a->hard_alpha_cap, r.white_bkgd = 0, r.lindisp = a->lindisp;
    r.rays = a->rays, r.jitter = a->jitter, r.rgb = a->rgb, r.depth = a->depth, r.invalid_wsum = a->invalid_wsum;
    if (int rc = render_fwd_impl(cfg, t, &r, s)) return rc;
  }
  return launched(novel_view_finish_launch(a, s), who);
}

// ---- training visualisation panels (models/bts/trainer.py:430-506)
static bool train_vis_counts_ok(long T, long K) { return T >= 1 && T <= BTS_TRAIN_VIS_MAX_FRAMES && K >= 2 && K <= 256; }

size_t bts_train_vis_workspace(int32_t T, int32_t h, int32_t w, int32_t K) {
  if (!train_vis_counts_ok(T, K) || !train_vis_sizes_ok(h, w)) return 0;
  return train_vis_bytes(T, w);
}

int bts_train_vis(const BtsTrainVis* a, void* stream) {
  const char* who = "bts_train_vis";
  if (!a) {
    set_error("%s: NULL argument struct", who);
    return BTS_E_INVALID;
  }
  if (a->T < 1 || a->T > BTS_TRAIN_VIS_MAX_FRAMES || a->T > a->v) {
    set_error("%s: T=%ld frames are outside [1, min(v = %ld, 6)]", who, (long)a->T, (long)a->v);
    return BTS_E_INVALID;
  }
  if (a->K < 2 || a->K > 256) {
    set_error("%s: K=%ld samples are outside [2, 256]", who, (long)a->K);
    return BTS_E_INVALID;
  }
  if (a->nv < 1 || a->nv > BTS_MAX_VIEWS) {
    set_error("%s: nv=%ld render views are outside [1, BTS_MAX_VIEWS = %ld]", who, (long)a->nv, (long)BTS_MAX_VIEWS);
    return BTS_E_INVALID;
  }
  if (a->S < 1 || a->S > BTS_MAX_SCALES) {
    set_error("%s: S=%ld depth scales are outside [1, BTS_MAX_SCALES = %ld]", who, (long)a->S, (long)BTS_MAX_SCALES);
    return BTS_E_INVALID;
  }
  if (!train_vis_sizes_ok(a->h, a->w)) {
    set_error("%s: the frame size h=%ld, w=%ld is outside [1, 8192]", who, (long)a->h, (long)a->w);
    return BTS_E_INVALID;
  }
  if (!a->lut || a->lut_N < 1 || a->lut_N > BTS_CMAP_MAX_N) {
    set_error("%s: an empty colour table: lut is NULL or lut_N=%ld is outside [1, 65536]", who, (long)a->lut_N);
    return BTS_E_INVALID;
  }
  for (int i = 0; i < a->T; ++i)
    if (!a->imgs[i]) {
      set_error("%s: NULL pointer: imgs[%ld]", who, (long)i);
      return BTS_E_INVALID;
    }
  for (int i = 0; i < a->S; ++i)
    if (!a->depth[i]) {
      set_error("%s: NULL pointer: depth[%ld]", who, (long)i);
      return BTS_E_INVALID;
    }
  if (!a->rgb || !a->alphas || !a->invalid) {
    set_error("%s: NULL pointer among the inputs rgb, alphas, invalid", who);
    return BTS_E_INVALID;
  }
  if (!a->input_im || !a->recon_im || !a->recon_depth || !a->depth_profile || !a->ray_entropy || !a->alpha_sum || !a->recon_mse || !a->invalids) {
    set_error("%s: NULL pointer among the eight output panels", who);
    return BTS_E_INVALID;
  }
  const size_t need = train_vis_bytes(a->T, a->w);
  if (!a->workspace || a->workspace_bytes < need || ((uintptr_t)a->workspace & 15) != 0) {
    set_error("%s: workspace too small or not 16-byte aligned (%ld bytes needed)", who, (long)need);
    return BTS_E_WORKSPACE;
  }
  return launched(train_vis_launch(a, (hipStream_t)stream), who);
}

// ---- patch colours (image_processor {type: patch}): what the three entries share -- the struct, the frames and cameras, the sizes, the
// compiled patch size; rays: the entry reads rays, z_samp, K and rays_per_sample
static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
static int check_patch_color(const BtsPatchColor* a, bool rays, const char* who) {
  if (!a) {
    set_error("%s: NULL argument struct", who);
    return BTS_E_INVALID;
  }
  if (!a->imgs_nhwc4 || !a->K_r || !a->w2c_r || (rays && (!a->rays || !a->z_samp))) {
    set_error("%s: NULL pointer among imgs_nhwc4, K_r, w2c_r (and rays, z_samp where the entry reads them)", who);
    return BTS_E_INVALID;
  }
  if (misaligned(a->imgs_nhwc4, 16) || misaligned(a->K_r, 4) || misaligned(a->w2c_r, 4) || (rays && (misaligned(a->rays, 4) || misaligned(a->z_samp, 4)))) {
    set_error("%s: misaligned pointer (imgs_nhwc4 needs 16 bytes, every other tensor 4)", who);
    return BTS_E_INVALID;
  }
  if (a->n <= 0 || a->nv <= 0 || a->H <= 0 || a->W <= 0 || (rays && (a->K <= 0 || a->rays_per_sample <= 0))) {
    set_error("%s: non-positive size (n, nv, H, W; K and rays_per_sample where the entry reads them)", who);
    return BTS_E_INVALID;
  }
  if (a->nv > BTS_MAX_VIEWS) {
    set_error("%s: nv=%ld render views exceed BTS_MAX_VIEWS = %ld", who, (long)a->nv, (long)BTS_MAX_VIEWS);
    return BTS_E_INVALID;
  }
  if ((long)a->H * a->W > (1L << 30)) {
    set_error("%s: a frame of H=%ld x W=%ld texels is more than 2^30", who, (long)a->H, (long)a->W);
    return BTS_E_INVALID;
  }
  if (!patch_color_size_ok(a->patch)) {
    set_error("%s: patch=%ld, but the compiled patch size is %ld (27 channels)", who, (long)a->patch, (long)BTS_PATCH_COLOR_SIZE);
    return BTS_E_UNSUPPORTED;
  }
  return BTS_OK;
}
static int check_patch_color_io(const void* in, const void* out, const char* names, const char* who) {
  char fmt[128];
  if (!in || !out) {
    snprintf(fmt, sizeof(fmt), "%%s: NULL pointer among %s", names);
    set_error(fmt, who);
    return BTS_E_INVALID;
  }
  if (misaligned(in, 4) || misaligned(out, 4)) {
    snprintf(fmt, sizeof(fmt), "%%s: misaligned pointer among %s (4 bytes)", names);
    set_error(fmt, who);
    return BTS_E_INVALID;
  }
  return BTS_OK;
}

int bts_patch_color_fwd(const BtsPatchColor* a, void* stream) {
  const char* who = "bts_patch_color_fwd";
  if (int rc = check_patch_color(a, true, who)) return rc;
  if (int rc = check_patch_color_io(a->weights, a->rgb, "weights, rgb", who)) return rc;
  if (misaligned(a->rgb_samps, 4)) {
    set_error("%s: misaligned pointer rgb_samps (4 bytes)", who);
    return BTS_E_INVALID;
  }
  return patch_color_fwd_impl(a, (hipStream_t)stream);
}

int bts_patch_color_bwd(const BtsPatchColor* a, const float* g_rgb, float* g_weights, void* stream) {
  const char* who = "bts_patch_color_bwd";
  if (int rc = check_patch_color(a, true, who)) return rc;
  if (int rc = check_patch_color_io(g_rgb, g_weights, "g_rgb, g_weights", who)) return rc;
  return patch_color_bwd_impl(a, g_rgb, g_weights, (hipStream_t)stream);
}

int bts_patch_color_query(const BtsPatchColor* a, const float* xyz, int32_t P, float* rgb, void* stream) {
  const char* who = "bts_patch_color_query";
  if (int rc = check_patch_color(a, false, who)) return rc;
  if (int rc = check_patch_color_io(xyz, rgb, "xyz, rgb", who)) return rc;
  if (P <= 0) {
    set_error("%s: non-positive point count P=%ld", who, (long)P);
    return BTS_E_INVALID;
  }
  return patch_color_query_impl(a, xyz, P, rgb, (hipStream_t)stream);
}

// ---- LiDAR ground-truth depth maps (kitti_raw_dataset.py:256-302, kitti_360_dataset.py:505-539)
// 0: served; BTS_E_INVALID / BTS_E_UNSUPPORTED: which of the two the sizes are (no message)
static int lidar_depth_sizes(long B, long H, long W) {
  if (B <= 0 || B > BTS_LIDAR_DEPTH_MAX_FRAMES || H <= 0 || W <= 0) return BTS_E_INVALID;
  if (W < 2 || H * W >= (1L << 24)) return BTS_E_UNSUPPORTED;
  return BTS_OK;
}

size_t bts_lidar_depth_workspace(int32_t B, int32_t H, int32_t W, int32_t p_fp64) {
  if (lidar_depth_sizes(B, H, W) != BTS_OK) return 0;
  return lidar_depth_bytes(B, H, W, p_fp64 != 0);
}

int bts_lidar_depth(const BtsLidarDepth* a, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "bts_lidar_depth";
  BTS_CHECK_LAYOUT(a && a->offsets && a->P && a->depth && a->H > 0 && a->W > 0, who);
  if (a->B <= 0 || a->B > BTS_LIDAR_DEPTH_MAX_FRAMES) {
    set_error("%s: B=%ld frames; between 1 and 32 per call", who, (long)a->B);
    return BTS_E_INVALID;
  }
  if (a->convention != BTS_LIDAR_DEPTH_KITTI_RAW && a->convention != BTS_LIDAR_DEPTH_KITTI_360) {
    set_error("%s: unknown convention %ld (0 kitti_raw, 1 kitti_360)", who, (long)a->convention);
    return BTS_E_INVALID;
  }
  if (a->eigen_depth && a->convention != BTS_LIDAR_DEPTH_KITTI_RAW) {
    set_error("%s: eigen_depth is kitti_raw's; kitti_360's load_depth has no crop", who);
    return BTS_E_INVALID;
  }
  if (a->offsets[0] != 0) {
    set_error("%s: offsets[0] = %ld, expected 0", who, (long)a->offsets[0]);
    return BTS_E_INVALID;
  }
  for (int f = 0; f < a->B; ++f) {
    if (a->offsets[f + 1] < a->offsets[f]) {
      set_error("%s: offsets decrease at frame %ld (%ld after %ld)", who, (long)f, (long)a->offsets[f + 1], (long)a->offsets[f]);
      return BTS_E_INVALID;
    }
  }
  const int64_t N = a->offsets[a->B];
  if (N > 0 && (!a->points || ((uintptr_t)a->points & 15) != 0)) {
    set_error("%s: points NULL or not 16-byte aligned", who);
    return BTS_E_INVALID;
  }
  if (a->W < 2) {
    set_error("%s: W=%ld; with one column every pixel shares one key of the reference's duplicate search", who, (long)a->W);
    return BTS_E_UNSUPPORTED;
  }
  if (lidar_depth_sizes(a->B, a->H, a->W) != BTS_OK) {
    set_error("%s: H * W = %ld pixels; from 2^24 the reference's float32 key stops being exact", who, (long)a->H * a->W);
    return BTS_E_UNSUPPORTED;
  }
  if (N >= (1LL << 31)) {
    set_error("%s: N=%ld points; fewer than 2^31 per call", who, (long)N);
    return BTS_E_UNSUPPORTED;
  }
  const size_t need = lidar_depth_bytes(a->B, a->H, a->W, a->p_fp64 != 0);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    set_error("%s: workspace NULL, too small or not 16-byte aligned (%ld bytes needed, see bts_lidar_depth_workspace)", who, (long)need);
    return BTS_E_INVALID;
  }
  return launched(lidar_depth_launch(a, workspace, (hipStream_t)stream), who);
}

}  // extern "C"
