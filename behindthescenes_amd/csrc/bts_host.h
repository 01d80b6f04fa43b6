// Host functions of libbts_render.so that one translation unit defines and another calls: each is declared HERE and nowhere else,
// with its default arguments.  Every .hip file that defines or calls one includes this header, so the compiler sees declaration and
// definition together (a changed parameter is a compile error at the definition, not a link error -- or, for a default, nothing at all).
// Behind them: the small inline helpers of the host layer and the kernel dispatch (the compiled shapes, the view-count rungs, the launch
// check).  No device code.
#pragma once
#include "bts_common.h"

#include <type_traits>

namespace bts {

struct FwdParams;   // bts_field_kernel.h
struct BwdParams;   // bts_bwd.h

// ---- bts_fwd.hip: the error text of bts_last_error() (thread-local; printf-style, one string and up to three longs), the compiled
// envelope, the persistent grids' geometry, the render forward and the field queries
void set_error(const char* fmt, const char* a = "", long b = 0, long c = 0, long d = 0);
const char* last_error();
bool shape_supported(int C, int HD, int NB);
FwdParams make_params(const BtsFieldCfg* cfg, const BtsFieldTensors* t);
int device_cu_count();
int render_grid(const FwdParams& p);
int render_chunk_log2(int grid, long groups);
long render_dyn_first(int grid, int chunk_log2, long groups, int tail_div);
int render_fwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, hipStream_t s);
// mlp_image: the staged MLP of bts_eval_frame_prep (bts_render_kernel.h: MlpImage) or NULL; pin: the launch may take the kernel with the
// evaluation frame's switches compiled in where its parameters match them (bts_field_kernel.h: PinnedSet)
int render_fwd_sched_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, unsigned* sched, hipStream_t s,
                          const float* mlp_image = nullptr, bool pin = false);
// PinnedSet::matches on the parameters render_fwd_sched_impl fills from these arguments (no launch, nothing dereferenced)
bool render_args_pinned(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a);
int field_query_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int P, int only_density, float* rgb,
                     float* invalid, float* sigma, hipStream_t s);
int occupancy_profile_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int Y, int cols, float threshold,
                           int only_density, float* profile, float* sigma, hipStream_t s);
// bts_fwd_proj.hip, bts_fwd_epi.hip: the pipelined render kernel without / with the loss epilogue
int launch_render_pipelined(const FwdParams& p, int C, int HD, int NB, int grid, hipStream_t s, bool pin = false);
int launch_render_pipelined_epi(const FwdParams& p, int C, int HD, int NB, int grid, hipStream_t s);
// bts_query.hip.  Plain query: cols = 0; profile: cols = columns per sample, col_len = Y, P = Y * cols
int query_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int P, int only_density, float* rgb, float* invalid,
               float* sigma, int cols, int col_len, float threshold, float* profile, hipStream_t s);

// ---- bts_bwd.hip: the render backward; render_bwd_flush_region: where pass C's slot copies sit inside a workspace
size_t render_bwd_workspace_impl(const BtsFieldCfg* cfg, const BtsRenderArgs* a);
void render_bwd_flush_region(const BtsFieldCfg* cfg, const BtsRenderArgs* a, void* workspace, float** ptr, size_t* bytes);
int render_bwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g, void* workspace,
                    hipStream_t s, bool flush_clean = false);   // flush_clean: the caller zeroed the slot copies on this stream
// bts_bwd_rows.hip (gate-bit passes; the row forms of passes B and C), bts_bwd_blocks.hip (row passes)
int launch_bwd_rows(const BwdParams& bp, int C, int HD, int n, int grid, hipStream_t s);
int launch_scatter_rows(const BwdParams& bp, const float* u0_ws, int HD, int n, hipStream_t s);
int launch_dwpe_rows(const FwdParams& p, const float* u0_ws, float* d_mlp, float* flush_ws, int C, int HD, int NB, int n, int grid, hipStream_t s,
                     bool flush_clean);
int launch_bwd_blocks(const BwdParams& bp, float* u0_ws, int C, int HD, int NB, int n, int grid, hipStream_t s);

// ---- bts_prep.hip: the projection G = F . w_in[:, :C]^T, its backward and the tile flags.  Wm: the map's width when `tiles` are
// 16 x 4 blocks (BtsFieldCfg.tile_blocks), 0 = runs of 64 texels; list_ws: scratch for the balanced (list-driven) form
int project_features_impl(int C, int HD, const float* feat, const float* mlp, int N, int HW, float* proj, const unsigned char* tiles, hipStream_t s,
                          bool feat_cl = false, int Wm = 0, void* list_ws = nullptr, size_t list_ws_bytes = 0);
int mark_tiles_impl(const float* rays, const float* z_samp, const float* jitter, const float* w2c_enc, const float* K_enc, long B, int Bp, int K, int lindisp,
                    int H, int W, int fs, unsigned char* tiles, hipStream_t s, int blocks);
int project_features_bwd_impl(int C, int HD, const float* feat, const float* dproj, const float* mlp, int N, int HW, float* dfeat,
                              float* d_mlp, hipStream_t s);
int project_features_bwd_tiles_impl(int C, int HD, const float* feat, float* dproj, unsigned char* tiles, const float* mlp, int N, int HW, float* dfeat,
                                    float* d_mlp, int clear, hipStream_t s, bool feat_cl = false, int Wm = 0, void* list_ws = nullptr,
                                    size_t list_ws_bytes = 0);

// ---- bts_aux.hip: layout changes, rays, sampling, the hand-over kernels of the training step and the eval frame
int transpose_launch(const float* src, float* dst, int N, int C, int H, int W, bool to_nhwc, hipStream_t s);
int pack_rgb_launch(const float* src, float* dst, int N, int H, int W, float scale, float shift, hipStream_t s);
int gen_rays_launch(const float* poses, const float* projs, int V, int H, int W, float zn, float zf, int norm_dir, float* rays,
                    hipStream_t s);
int gen_rays_nf_launch(const float* poses, const float* projs, const float* near_far, int V, int H, int W, int norm_dir, float* rays,
                       hipStream_t s);
int patch_rays_launch(const float* poses, const float* projs, const float* images, const int* pv, const int* py, const int* px, int n, int v,
                      int c, int H, int W, int P, int ph, int pw, float zn, float zf, int norm_dir, float* rays, float* gt, hipStream_t s);
int sample_coarse_launch(const float* rays, const float* u, long B, int K, int lindisp, float* z, hipStream_t s);
int distance_to_z_launch(const float* depths, const float* invK, int N, int H, int W, float* out, hipStream_t s);
// the evaluation frame's prep launch (MLP | projection); mlp_image_floats: the size of its `image`, 0 = no such shape
long mlp_image_floats(int C, int HD, int NB);
int eval_prep_launch(int C, int HD, int NB, const float* feat, bool feat_cl, float* proj, const float* const* tensors, const float* empty, float* packed,
                     float* image, int n, int HW, hipStream_t s);
int invert_small_launch(const float* src, float* dst, int N, int dim, hipStream_t s);
int handover_launch(const float* Ks, const float* poses, const float* images, const int* pv, const int* py, const int* px, int n, int v, int id_enc, int nv,
                    const int* ids_render, int n_loss, const int* ids_loss, int H, int W, int P, int ph, int pw, float z_near, float z_far, float scale,
                    float shift, float* cams, float* imgs, float* rays, float* gt, int n_zero, unsigned char* const* zero, const long* zero_bytes,
                    hipStream_t s);
int eval_handover_launch(const float* Ks, const float* poses, const float* images, int n, int v, int id_enc, int nv, const int* ids_render, int H, int W,
                         float z_near, float z_far, int norm_dir, float scale, float shift, float* cams, float* inv_K, float* imgs, float* rays,
                         float* rgb_gt, unsigned* sched, hipStream_t s);

// ---- bts_loss.hip (patches of at most 64 pixels), bts_loss_tiled.hip (patches of any size)
// thresh (B) or NULL: the automasking bound on every pixel's error -- a compile-time variant of the kernels, the forms without it are untouched
int photometric_loss_impl(const BtsLossArgs* a, hipStream_t s, const float* thresh = nullptr);
size_t loss_tiled_bytes(int n_patches, int ph, int pw, int nv, bool with_thresh = false);
int photometric_loss_tiled_impl(const BtsLossArgs* a, void* workspace, hipStream_t s, const float* thresh = nullptr);
// ... with median thresholding over n batch samples (bts_loss_tiled.hip's median variant of the passes); thresh may be NULL
size_t loss_median_bytes(int n_patches, int ph, int pw, int nv, int n);
int photometric_loss_median_impl(const BtsLossArgs* a, int n, const float* thresh, float* out, float* thresholds, int64_t* kept, void* workspace,
                                 hipStream_t s);
// ---- bts_loss_pixel.hip: criteria l1 / l2, median thresholding, the diverse flags
size_t pixel_loss_bytes(long B, int n, int ph, int pw);
int pixel_loss_impl(const BtsPixelLossArgs* a, void* workspace, hipStream_t s, const float* thresh = nullptr);
// ---- bts_loss_pixel_c.hip: criteria l1 / l2 for a run-time channel count
size_t pixel_loss_channels_bytes(long B);
int pixel_loss_channels_impl(const BtsPixelLossArgs* a, int channels, void* workspace, hipStream_t s);
// ---- bts_loss_reg.hip: the alpha / surfaceness / entropy / depth regularisers
size_t loss_reg_bytes(long B, int n_patches, int ph, int pw, int K);
int loss_reg_impl(const BtsLossRegArgs* a, void* workspace, hipStream_t s);
// ---- bts_sample_fine.hip: importance / depth draws and their merge with the coarse depths; from-dist sampling
int sample_fine_launch(const BtsSampleFineArgs* a, hipStream_t s);
// ---- bts_automask.hip: the error map of use_automasking
long automask_tiles(int n, int H, int W);
int automask_errors_launch(const float* images, int n, int v, int H, int W, const int* ids_loss, int L, float scale, float* errors,
                           float* images4, hipStream_t s);
int diverse_flags_launch(const float* rgb_samps, const float* weights, const float* invalid, long B, int K, int nv, float* flags, hipStream_t s);

// ---- bts_mlp_color.hip: MLP-predicted colour
int mlp_color_render_fwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, hipStream_t s);
int mlp_color_field_query_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int P, int only_density, float* rgb,
                               float* invalid, float* sigma, hipStream_t s);
size_t mlp_color_bwd_workspace_impl(const BtsFieldCfg* cfg, const BtsRenderArgs* a);
int mlp_color_render_bwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g, void* workspace,
                              hipStream_t s);

// ---- bts_patch_color.hip: 27-channel patch colours from the render's weights
bool patch_color_size_ok(int patch);
int patch_color_fwd_impl(const BtsPatchColor* a, hipStream_t s);
int patch_color_bwd_impl(const BtsPatchColor* a, const float* g_rgb, float* g_weights, hipStream_t s);
int patch_color_query_impl(const BtsPatchColor* a, const float* xyz, int P, float* rgb, hipStream_t s);

// ---- bts_multi_view.hip: merged encoder views (the field is checked by bts_api.hip before any of these runs)
int multi_view_render_fwd_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a, hipStream_t s);
int multi_view_field_query_impl(const BtsMultiViewField* mv, const float* xyz, int P, float* rgb, float* invalid, float* sigma, hipStream_t s);
size_t multi_view_bwd_workspace_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a);
int multi_view_render_bwd_impl(const BtsMultiViewField* mv, const BtsRenderArgs* a, const BtsRenderGrads* g, float* const* d_proj_views,
                               unsigned char* const* d_proj_tiles_views, void* workspace, hipStream_t s);

// ---- bts_occ.hip: LiDAR occupancy evaluation.  *_layout: the ONE statement of a workspace's layout, run over a Carver (below) once to
// count the bytes and once to hand out the pointers
class Carver;
struct LidarBins {
  unsigned* bins;
  unsigned long long* first;
};
LidarBins lidar_bins_layout(Carver& w, int T, int y_res);
size_t lidar_bins_bytes(int T, int y_res);
struct OccEvalWs {
  char* bins;   // lidar_bins_layout's
  float *tables, *w2v, *w2c;
  unsigned char *is_occ, *is_vis;
  float* sigma;
};
OccEvalWs occ_eval_layout(Carver& w, int P, int T, int y_res);
int lidar_slices_launch(const float* points, const int* offsets, int T, const float* velo_poses, const float* borders, float y_lo, float y_hi,
                        int y_res, float max_dist, void* bins_ws, float* tables, hipStream_t s);
int lidar_occupancy_launch(const float* q_pts, int P, const float* tables, int y_res, int T, const float* world_to_velo, float min_dist,
                           unsigned char* is_occupied, unsigned char* is_visible, hipStream_t s);
int occ_metrics_launch(const float* q_pts, int P, const float* sigma, const unsigned char* is_occupied, const unsigned char* is_visible,
                       const float* depth_z, int H, int W, const float* proj, const float* w2c, float occ_threshold, int* counts,
                       unsigned char* masks, hipStream_t s);

// ---- bts_depth_metrics.hip, bts_nvs_metrics.hip: depth and NVS evaluation metrics
size_t depth_metrics_bytes(int B, int Hg, int Wg);
int depth_metrics_launch(const BtsDepthMetrics* a, void* workspace, hipStream_t s);
size_t nvs_metrics_bytes(int B, int He, int We);
int nvs_metrics_launch(const BtsNvsMetrics* a, void* workspace, hipStream_t s);

// ---- bts_lidar_depth.hip: LiDAR ground-truth depth maps (both KITTI load_depth)
size_t lidar_depth_bytes(int B, int H, int W, bool p_fp64);
int lidar_depth_launch(const BtsLidarDepth* a, void* workspace, hipStream_t s);

// ---- bts_bbox_occ.hip: 3D-bounding-box occupancy evaluation
struct BBoxEvalWs {
  float *to_key, *tables;
  int* n_faces;
  unsigned char* active;
  float *pseudo, *sigma;
};
BBoxEvalWs bbox_eval_layout(Carver& w, int P, int B, int ph, int pw);
int bbox_bounds_launch(const float* vertices, const int* faces, const int* v_offsets, const int* f_offsets, int B, const float* to_key,
                       const float* proj, float max_d, float* tables, int* n_faces, unsigned char* active, int* n_active, hipStream_t s);
int bbox_pseudo_depth_launch(const float* rays, int ph, int pw, const float* seg, int hs, int ws, const float* tables, const int* n_faces,
                             const unsigned char* active, const float* semantic_id, int B, float* pseudo_depth, hipStream_t s);
int bbox_metrics_launch(const float* q_pts, int P, const float* sigma, const float* pseudo, const float* depth_z, int H, int W, const float* proj,
                        const float* tables, const int* n_faces, const unsigned char* active, int B, float occ_threshold, int* counts,
                        unsigned char* masks, hipStream_t s);

// ---- bts_frames.hip: novel-view frames and colour-mapped depth
int colorize_launch(const float* x, int B, int h, int w, int norm, int N, const double* lut, const unsigned char* lut_u8, float* partials,
                    double* out, unsigned char* canvas, int Hc, int Wc, int row0, int col0, hipStream_t s);
int pack_u8_launch(const float* x, long sb, long sy, long sx, long sc, int B, int h, int w, float scale, float shift, unsigned char* canvas,
                   int Hc, int Wc, int row0, int col0, hipStream_t s);
int novel_view_finish_launch(const BtsNovelViews* a, hipStream_t s);

// ---- bts_train_vis.hip: the trainer's visualisation panels
bool train_vis_sizes_ok(int h, int w);
size_t train_vis_bytes(int T, int w);
int train_vis_launch(const BtsTrainVis* a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// small helpers of the host layer
// ---------------------------------------------------------------------------------------------------------------
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// A workspace's layout, written ONCE as a sequence of take<T>(count) calls: run over Carver(nullptr) it counts the bytes, run over
// Carver(workspace) it hands out the pointers.  Every buffer starts on a 256-byte boundary behind the (rounded-up) workspace pointer;
// bytes() includes the 256 that rounding may cost
constexpr size_t kAlign = 256;
inline size_t up256(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }
class Carver {
 public:
  explicit Carver(void* workspace) : base_(reinterpret_cast<char*>(up256((size_t)(uintptr_t)workspace))) {}
  template <class T>
  T* take(size_t count) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += up256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return kAlign + off_; }

 private:
  char* base_;
  size_t off_ = 0;
};

// tiles (64 texels each, either geometry: bts_common.h) of the map of an H x W frame at feat_shift fs
inline long map_tiles(int H, int W, int fs) { return ((long)(H >> fs) * (W >> fs) + 63) / 64; }

// the `Wm` of the projection passes: the map's width where the cfg's tile flags are 16 x 4 blocks, 0 where they are runs of 64 texels
inline int tile_geometry_width(const BtsFieldCfg* cfg) { return cfg->tile_blocks ? cfg->W >> cfg->feat_shift : 0; }

// the cameras the hand-over kernels leave in one block: K_enc (n, 9) | w2c_enc (n, 16) | K_r (n, nv, 9) | w2c_r (n, nv, 16)
struct CamBlock {
  float *K_enc, *w2c_enc, *K_r, *w2c_r;
};
inline CamBlock split_cams(float* cams, int n, int nv) {
  CamBlock c;
  c.K_enc = cams;
  c.w2c_enc = c.K_enc + (long)n * 9;
  c.K_r = c.w2c_enc + (long)n * 16;
  c.w2c_r = c.K_r + (long)n * nv * 9;
  return c;
}

// ---------------------------------------------------------------------------------------------------------------
// kernel dispatch: the compiled field shapes, the view-count rungs, the launch check
// ---------------------------------------------------------------------------------------------------------------
// The field shapes (C, d_hidden, n_blocks) the kernels are compiled for: THE list -- bts_supported (shape_supported) and every dispatch
// read it, nothing else names a shape.
template <int C_, int HD_, int NB_>
struct Shape {
  static constexpr int C = C_, HD = HD_, NB = NB_;
  static bool is(int c, int hd, int nb) { return c == C && hd == HD && nb == NB; }
};
// what a (C, HD)-only dispatch is handed: a shape without its n_blocks
template <int C_, int HD_>
struct Width {
  static constexpr int C = C_, HD = HD_;
};
template <class... S>
struct ShapeList {
  // rc = f(S{}) for the shape S that is (C, HD, NB) / rc = f(Width{}) for the first shape with these C and HD; false: there is none
  template <class F>
  static bool shape(int C, int HD, int NB, int& rc, F&& f) {
    return ((S::is(C, HD, NB) && (rc = f(S{}), true)) || ...);
  }
  template <class F>
  static bool width(int C, int HD, int& rc, F&& f) {
    return ((C == S::C && HD == S::HD && (rc = f(Width<S::C, S::HD>{}), true)) || ...);
  }
};
using Re10kShape = Shape<32, 32, 1>;   // exp_re10k.yaml: the one shape with a ResnetBlockFC, and with 48-lane modes
using Shapes = ShapeList<Shape<64, 64, 0>, Re10kShape, Shape<32, 32, 0>>;

// f(S{}) for the compiled shape S that is (C, HD, NB); no such shape: BTS_E_UNSUPPORTED and the text below.  (Every entry point rejects
// such a shape with its own envelope message before anything gets here.)
template <class F>
int with_shape(int C, int HD, int NB, F&& f) {
  int rc = BTS_E_UNSUPPORTED;
  if (!Shapes::shape(C, HD, NB, rc, f)) set_error("%s: unsupported MLP shape C=%ld d_hidden=%ld n_blocks=%ld", "bts", C, HD, NB);
  return rc;
}
// f(Width<C, HD>{}) where a compiled shape has these C and HD (the projection and the gate-bit passes do not depend on n_blocks),
// BTS_E_UNSUPPORTED otherwise
template <class F>
int with_width(int C, int HD, F&& f) {
  int rc = BTS_E_UNSUPPORTED;
  (void)Shapes::width(C, HD, rc, f);
  return rc;
}

// f(std::integral_constant<int, NVMAX>{}): the size of a kernel's per-view arrays for nv render views (nv <= BTS_MAX_VIEWS = 8)
template <class F>
int with_nvmax(int nv, F&& f) {
  if (nv <= 1) return f(std::integral_constant<int, 1>{});
  if (nv <= 2) return f(std::integral_constant<int, 2>{});
  if (nv <= 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

// The status of the launches issued so far, read ONCE (reading clears it): the only place csrc asks HIP for it.  A failure is
// BTS_E_LAUNCH with set_error(fmt, who, code), who = the HIP error string unless the caller names itself; fmt = NULL leaves the message
// to the caller (bts_api.hip's launched(rc, who))
inline int launch_check(const char* fmt = "%s: kernel launch failed (%ld)", const char* who = nullptr) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return BTS_OK;
  if (fmt) set_error(fmt, who ? who : hipGetErrorString(e), (long)e);
  return BTS_E_LAUNCH;
}
inline int launch_code() { return launch_check(nullptr); }

// kern<<<grid, 256, dyn, s>>>(args...) for a kernel whose dynamic LDS (dyn bytes) may exceed the 64 KB a launch gets without asking
template <class K, class... A>
void launch_dyn_lds(K kern, int grid, int dyn, hipStream_t s, const A&... args) {
  if (dyn) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
  kern<<<grid, 256, dyn, s>>>(args...);
}

}  // namespace bts
