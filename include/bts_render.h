/*
 * bts_render.h -- C ABI of the MI355X-native BehindTheScenes density-field renderer (libbts_render.so).
 *
 * The reference (Brummi/BehindTheScenes @ 2024_10_08) is pure Python/PyTorch and has no FFI of its own; its seam for
 * this path is a Python object protocol.  The entry points below are what a binding for that seam
 * needs and nothing more; each one names the reference function(s) it replaces.  Plain pointers and sizes only: no torch
 * types, no allocation inside, no exceptions -- every function returns 0 on success or a negative BTS_E_* code and
 * leaves a message retrievable with bts_last_error().  All pointers are DEVICE pointers to fp32 data unless noted; all
 * work is enqueued on the caller's HIP stream (`stream` is a hipStream_t passed as void*; NULL = default stream) and the
 * functions are re-entrant (autograd may call the backward from another thread).
 *
 * Data layout in HBM:
 *   proj_nhwc   (n, H, W, Hd)       "projected" feature map G = F . w_in[:, :C]^T, channels-last: bilinear interpolation and
 *                                   lin_in are both linear, so lin_in(bilinear(F)) == bilinear(G) + w_in[:, C:] . PE + b_in;
 *                                   bts_project_features builds G from the encoder's NCHW output in one pass (it replaces the
 *                                   NCHW->NHWC hand-over), the render kernels gather G straight into the MFMA accumulators.
 *   feat_nhwc   (n, H, W, C)        alternative: raw channels-last F, lin_in evaluated per point (forward / query only)
 *   imgs_nhwc4  (n, nv, H, W, 4)    rgb0-packed colour frames in [0,1]                 -> one 16-byte load per tap
 *   rays        (n*Bp, 8)           [origin(3), direction(3), near, far]   (reference layout, util.py:270-273)
 *   z_samp      (n*Bp, K)           sample depths per ray                  (reference layout, nerf.py:210-218)
 *   mlp_params  packed fp32: w_in (Hd x d_in, row-major = nn.Linear.weight), b_in (Hd),
 *               n_blocks x [fc_0.weight (Hd x Hd), fc_0.bias (Hd), fc_1.weight (Hd x Hd), fc_1.bias (Hd)],
 *               w_out (Hd), b_out (1);  d_in = C + 3 + 6*num_freqs.
 */
#ifndef BTS_RENDER_H
#define BTS_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BTS_ABI_VERSION 9

enum {
  BTS_OK = 0,
  BTS_E_INVALID = -1,     /* NULL pointer / non-positive size / inconsistent arguments */
  BTS_E_UNSUPPORTED = -2, /* configuration outside the compiled envelope (see bts_supported) */
  BTS_E_LAUNCH = -3,      /* HIP runtime reported an error at launch */
  BTS_E_WORKSPACE = -4    /* workspace too small (see bts_render_bwd_workspace) */
};

/* Scalar configuration of the field: BTSNet.__init__ (models/bts/model/models_bts.py:18-54),
 * PositionalEncoding (models/common/model/code.py:11-28), ResnetFC shape (models/common/model/resnetfc.py:65-130).
 *
 * Precision of lin_in's inputs (resnetfc.py:147, models_bts.py:150-171).  The 36 trigonometric inputs AND the three raw ones -- the
 * projected x, y and the depth code -- enter the f16 matrix pipe as two round-to-nearest halves each: v = hi + lo + r with
 * |r| <= 2^-22 |v| in the worst case (each half rounds to 11 significand bits; 2^-23 |v| typical), the weights likewise after an exact
 * power-of-two scaling; the products hi.hi + lo.hi + hi.lo are exact in the fp32 accumulator, the dropped lo.lo term is <= 2^-22 |w v|.
 * That is up to four fp32 rounding units (2^-24) per product.  For the sines (|v| <= 1) it vanishes in the accumulation's own rounding.
 * x and y are NOT bounded by 1: a point beside or behind the encoder camera projects to |x|, |y| of hundreds (the perspective divide
 * clamps z at 1e-3), and the split then costs up to 2^-22 |x| ABSOLUTE per product.  It stays invisible next to what the reference's own
 * fp32 arithmetic does there: the twelve encoding inputs sin(f x [+ pi/2]), f = 1.5 .. 48, are evaluated on fp32 arguments whose rounding
 * alone is 2^-24 f |x| -- 12 to 48 times the split's error on the raw row, through weights of the same size.  Beyond |x|, |y| = 2083
 * (encoding arguments past the fast sines' range) a wave takes the exact fp32 routine.  Pinned by
 * tests/test_gpu_parity.py::test_raw_rows_worst_case_vs_fp64: |x|, |y| log-uniform up to 2000, the code at both ends of [-1, 1] and
 * clamped, learn_empty on and off -- never further from an fp64 evaluation than 1.5 x the fp32 reference's own distance. */
typedef struct BtsFieldCfg {
  int32_t n;           /* batch ("super-batch") size */
  int32_t H, W;        /* feature-map and colour-frame size */
  int32_t C;           /* feature channels (encoder.latent_size) */
  int32_t d_hidden;    /* MLP hidden width */
  int32_t n_blocks;    /* number of ResnetBlockFC */
  int32_t nv;          /* number of render (colour) views, 0..BTS_MAX_VIEWS */
  int32_t num_freqs;   /* PE octaves (6 in every shipped config) */
  int32_t code_mode;   /* 0 = "z", 1 = "distance"  (models_bts.py:157-171) */
  int32_t inv_z;       /* 1 = inverse-depth normalisation */
  int32_t learn_empty; /* 1 = replace features of out-of-frustum points by empty_feature (models_bts.py:176-182) */
  int32_t empty_empty; /* 1 = sigma := 0 for out-of-frustum points (models_bts.py:323-324) */
  float freq_factor;   /* PE base frequency (1.5) */
  float d_min, d_max;  /* z_near, z_far of the field */
  /* ABI 4: the feature map of decoder scale s handed over at ITS OWN size.  BTSNet.encode resizes every scale's map to scale 0's
   * size with F.interpolate(mode="nearest") (models_bts.py:115-117) before the renderer samples it; for sizes that differ by 2^s that
   * map is texel (y >> s, x >> s) of the small one, so the kernels index the small map directly: feat / proj / d_proj are
   * (n, H >> feat_shift, W >> feat_shift, .) and every result is bit-identical to the resized map's.  H and W (the colour frames'
   * size, and the size the bilinear taps are computed for) must be multiples of 2^feat_shift.  0 = a full-size map. */
  int32_t feat_shift;
  /* ABI 5: index j of a render view whose camera IS the encoder camera of every batch element -- K_r[:, j] == K_enc and
   * w2c_r[:, j] == w2c_enc bit for bit, i.e. ids_render[j] == ids_encoder[0] in BTSNet.encode (models_bts.py:84-97; the eval_depth
   * configuration renders its colours from the encoder frame) -- or -1.  The forward and query kernels then take that view's
   * projection, frustum flag and bilinear weights from the encoder view's instead of evaluating them a second time: same inputs, same
   * instruction sequence, bit-identical results (tests/test_gpu_abi5.py).  A hint: -1 is always correct. */
  int32_t enc_render_view;
  /* ABI 9: the geometry of this map's tile flags (BtsRenderGrads.d_proj_tiles, every `tiles` argument).  0: tile t = texels 64 t .. 64 t + 63
   * of the row-major map (ABI 6 - 8).  1: tile t = the block of 4 rows x 16 texels at rows 4 (t / (W' / 16)) .., columns 16 (t % (W' / 16)) ..
   * of the (H', W') = (H >> feat_shift, W >> feat_shift) map -- honoured where H' is a multiple of 4 and W' of 16, otherwise the
   * linear form is used as with 0 (bts_proj_tile_count is ceil(H' W' / 64) either way).  A training step's samples lie on streaks along
   * the epipolar lines: they touch 38 % of the 64 x 1 runs and 26 % of the 16 x 4 blocks of exp_kitti_360.yaml's maps.  Blocks pay with a
   * CHANNELS-LAST feature map (a block = four 4 KB pieces of F, dF, G, dG each: train step -3 %); with an NCHW map its rows come
   * apart into 64-byte pieces and the projection backward is 2 % SLOWER than with runs (profiles/r06f) -- so: 1 for channels-last maps, 0
   * for NCHW ones.  Every call that produces or consumes one flag array must see the same value. */
  int32_t tile_blocks;
} BtsFieldCfg;

#define BTS_MAX_VIEWS 8

/* State left behind by BTSNet.encode (models_bts.py:128-136), in the layouts above. */
typedef struct BtsFieldTensors {
  const float* feat_nhwc;     /* (n, H, W, C)   raw features; may be NULL when proj_nhwc is given */
  const float* proj_nhwc;     /* (n, H, W, Hd)  projected features (preferred; required by the backward) or NULL */
  const float* K_enc;         /* (n, 3, 3)   normalised intrinsics of the encoder view */
  const float* w2c_enc;       /* (n, 4, 4)   world -> encoder camera */
  const float* imgs_nhwc4;    /* (n, nv, H, W, 4), may be NULL iff nv == 0 */
  const float* K_r;           /* (n, nv, 3, 3) */
  const float* w2c_r;         /* (n, nv, 4, 4) */
  const float* empty_feature; /* (C) or NULL */
  const float* mlp_params;    /* packed, see above */
} BtsFieldTensors;

/* One call of NeRFRenderer.composite (models/common/render/nerf.py:210-313) on n*Bp rays. */
typedef struct BtsRenderArgs {
  int32_t rays_per_sample; /* Bp */
  int32_t K;               /* samples per ray */
  int32_t hard_alpha_cap;  /* nerf.py:285-286 */
  int32_t white_bkgd;      /* nerf.py:301-304: rgb += 1 - sum(weights); honoured by the forward AND the backward */
  const float* rays;       /* (n*Bp, 8) */
  const float* z_samp;     /* (n*Bp, K), or NULL with `jitter` below */
  /* outputs; the per-sample ones may be NULL when not wanted */
  float* rgb;              /* (n*Bp, nv*3) */
  float* depth;            /* (n*Bp) */
  float* weights;          /* (n*Bp, K)        or NULL */
  float* alphas;           /* (n*Bp, K)        or NULL */
  float* invalid;          /* (n*Bp, K, nv)    or NULL   1.0 = sample outside a frustum */
  float* rgb_samps;        /* (n*Bp, K, nv*3)  or NULL */
  float* sigma_raw;        /* (n*Bp, K)        or NULL   pre-softplus MLP output  } the two per-sample activations the  */
  float* trans;            /* (n*Bp, K)        or NULL   transmittance before sample } backward needs (8 B per sample)     */
  /* ABI 2: what the photometric loss' invalid-ray policies (loss.py:100-118) need of `weights` and `invalid`, reduced over the samples
   * in the kernel's epilogue -- a training step then stores 8 B per ray and view instead of (1 + nv) * 4 * K B per ray */
  float* invalid_wsum;     /* (n*Bp, nv)       or NULL   sum_k weights_k * invalid_k,v   (policy weight_guided: > 0.9) */
  float* invalid_any;      /* (n*Bp, nv)       or NULL   max_k invalid_k,v               (policy strict) */
  /* ABI 3: the density noise of a training step (nerf.py:279-280: sigmas + randn_like(sigmas) * noise_std, drawn by the caller),
   * added to softplus(s) before relu / alpha -- INPUT of the forward and of the backward (which needs the sign of the sum) */
  const float* sigma_noise;/* (n*Bp, K)        or NULL */
  /* ABI 5: NeRFRenderer.sample_coarse (nerf.py:103-123) inside the forward kernel.  With z_samp == NULL the sample depths are computed
   * from every ray's [near, far] and the stratified jitter `jitter` in [0, 1) (the caller's torch.rand_like draw, nerf.py:112) by the
   * routine bts_sample_coarse runs -- bit-identical depths, one launch and 8 bytes per sample of HBM traffic less; `lindisp` selects
   * disparity- (nerf.py:117) or depth-linear (:115) spacing; z_samp_out, when given, receives the depths (a training step hands them
   * to bts_render_bwd as z_samp).  Ignored when z_samp is given.  Needs proj_nhwc. */
  const float* jitter;     /* (n*Bp, K)        or NULL */
  float* z_samp_out;       /* (n*Bp, K)        or NULL */
  int32_t lindisp;
  int32_t reserved_;       /* 0 */
} BtsRenderArgs;

/* Gradients flowing into / out of the renderer (what torch.autograd would compute through nerf.py:283-299,
 * models_bts.py:266-338 and resnetfc.py:132-184).  No gradient is produced for rays, z_samp, poses or colours. */
typedef struct BtsRenderGrads {
  const float* g_rgb;      /* (n*Bp, nv*3) or NULL */
  const float* g_depth;    /* (n*Bp)       or NULL */
  const float* g_weights;  /* (n*Bp, K)    or NULL */
  const float* g_alphas;   /* (n*Bp, K)    or NULL */
  float* d_proj_nhwc;      /* (n, H, W, Hd) gradient w.r.t. proj_nhwc, ACCUMULATED into (caller zero-fills), or NULL to skip */
  float* d_mlp_params;     /* packed like mlp_params, ACCUMULATED into (caller zero-fills), or NULL to skip */
  float* d_empty_proj;     /* (Hd) gradient w.r.t. the PROJECTED empty feature (w_in[:, :C] . empty_feature), accumulated, or NULL */
  /* ABI 6: which parts of d_proj_nhwc received anything.  (n, bts_proj_tile_count(cfg)) bytes, one per tile of 64 texels of an image's
   * map: the backward SETS the byte of every tile it adds into (it never clears one), or NULL.  A training step's rays touch 8-15 % of
   * the texels; bts_project_features_bwd_tiles reads only the flagged tiles.
   * TILE GEOMETRY (ABI 9; the same for every `tiles` argument of this header): BtsFieldCfg.tile_blocks -- runs of 64 consecutive texels
   * (0; ABI 6 - 8: always) or blocks of 4 rows x 16 texels (1).  Flags are produced and consumed by this library (bts_render_bwd,
   * bts_mark_sampled_tiles -> bts_project_features_tiles / _bwd_tiles / _cl); a caller that writes its own needs the mapping
   * (behindthescenes_amd.native.proj_tile_map). */
  uint8_t* d_proj_tiles;
} BtsRenderGrads;

int bts_abi_version(void);
const char* bts_last_error(void);

/* 1 if (C, d_hidden, n_blocks, nv, num_freqs) is inside the compiled envelope, else 0. */
int bts_supported(const BtsFieldCfg* cfg);
/* number of floats in mlp_params for cfg */
int64_t bts_mlp_param_count(const BtsFieldCfg* cfg);

/* Fused sample -> project -> bilinear(F) -> PE -> MLP -> softplus -> colour taps -> alpha-composite.
 * Replaces NeRFRenderer.composite + BTSNet.forward + sample_features + sample_colors + ResnetFC.forward +
 * PositionalEncoding.forward (nerf.py:210-313, models_bts.py:138-338, resnetfc.py:132-184, code.py:30-42). */
int bts_render_fwd(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, void* stream);

/* Backward of bts_render_fwd.  `a` must carry sigma_raw and trans written by the forward (weights/alphas are not needed).  When
 * a->rgb_samps is non-NULL it is READ here: the forward's per-sample colours, which spare the backward one projection + four taps
 * per view and sample (training requests rgb_samps anyway); NULL = recompute them.
 * workspace: bts_render_bwd_workspace(cfg, a) bytes of device scratch -- what the backward's passes hand each other: for the plain
 * MLP (n_blocks = 0) with K <= 64, 20 bytes per sample at d_hidden = 64 (the gradient at the pre-softplus density + the relu gates
 * as bits, per sample and per channel); with ResnetBlockFC layers or K > 64, 4 (d_hidden + 1) bytes per sample (the gradient row at
 * lin_in's output + the gradient at the pre-softplus density).  Contents need no initialisation. */
size_t bts_render_bwd_workspace(const BtsFieldCfg* cfg, const BtsRenderArgs* a);
int bts_render_bwd(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Hand-over from the (PyTorch) encoder, fused with the feature part of lin_in (resnetfc.py:147 restricted to the first C
 * inputs): feat_nchw (N, C, H, W) -> proj_nhwc (N, H, W, Hd) = F . w_in[:, :C]^T.  Uses cfg->C, d_hidden, n_blocks, num_freqs. */
int bts_project_features(const BtsFieldCfg* cfg, const float* feat_nchw, const float* mlp_params, int32_t N, float* proj_nhwc,
                         void* stream);
/* Its backward: d_feat_nchw (N, C, H, W) = d_proj . w_in[:, :C] (written, not accumulated; may be NULL) and
 * d_mlp_params[w_in[:, :C]] += d_proj^T . F (accumulated; may be NULL).  empty_feature handling: d_empty_proj (Hd) is the
 * gradient the render backward accumulated for the projected empty feature; d_empty_feature (C) += w_in[:, :C]^T d_empty_proj. */
int bts_project_features_bwd(const BtsFieldCfg* cfg, const float* feat_nchw, const float* d_proj_nhwc, const float* mlp_params,
                             int32_t N, float* d_feat_nchw, float* d_mlp_params, void* stream);

/* ABI 6: the same backward over a SPARSE d_proj.  `tiles` (N, bts_proj_tile_count(cfg)) is the flag array bts_render_bwd filled
 * (BtsRenderGrads.d_proj_tiles): only flagged tiles of d_proj_nhwc are read, every other texel is taken as zero (it must BE zero if
 * clear_after is set, see below).  d_feat_nchw is written densely (zeros where nothing arrived), d_mlp_params accumulated.  With
 * clear_after != 0 the call also writes zeros over the flagged tiles of d_proj_nhwc and resets their flags: a caller that keeps one
 * (d_proj, tiles) pair per map shape zero-fills it once and never again (the fill of a training step's d_proj is as large as the
 * gradient's whole HBM traffic otherwise: 503 MB at exp_kitti_360.yaml's batch). */
/* tiles per image of cfg's map ((H >> feat_shift) * (W >> feat_shift) texels, 64 per tile, rounded up); -1 for an invalid cfg (feat_shift
 * outside 0 .. 6, H or W not a multiple of 2^feat_shift, non-positive sizes) */
int64_t bts_proj_tile_count(const BtsFieldCfg* cfg);
/* ABI 6: the forward side of the same observation -- a render reads only the tiles its samples' taps land in.
 * bts_mark_sampled_tiles: for every sample of every ray of `a` (rays, rays_per_sample, K, and z_samp or jitter + lindisp exactly as
 * bts_render_fwd takes them; cfg->n, H, W, feat_shift; the encoder cameras) the flags (n, bts_proj_tile_count(cfg)) of the four tap
 * texels' tiles are SET (caller zero-fills) -- computed with the render kernels' own depth / projection / tap routines, i.e. the same
 * texels bit for bit.  bts_project_features_tiles then evaluates the flagged tiles of proj_nhwc only and leaves the rest of the buffer
 * untouched (uninitialised memory stays uninitialised): such a map is good for bts_render_fwd / bts_render_bwd on THAT sample set and
 * for nothing else (no field queries). */
int bts_mark_sampled_tiles(const BtsFieldCfg* cfg, const float* K_enc, const float* w2c_enc, const BtsRenderArgs* a, uint8_t* tiles,
                           void* stream);
int bts_project_features_tiles(const BtsFieldCfg* cfg, const float* feat_nchw, const float* mlp_params, int32_t N, const uint8_t* tiles,
                               float* proj_nhwc, void* stream);
int bts_project_features_bwd_tiles(const BtsFieldCfg* cfg, const float* feat_nchw, float* d_proj_nhwc, uint8_t* tiles,
                                   const float* mlp_params, int32_t N, float* d_feat_nchw, float* d_mlp_params, int32_t clear_after,
                                   void* stream);
/* ABI 8: the encoder's map handed over CHANNELS-LAST -- (N, H >> s, W >> s, C) in memory, i.e. a torch tensor of shape (N, C, h, w) in
 * channels_last format: what MIOpen's NHWC convolutions and bts_conv3x3_fwd (out_nchw = 0) write.  The same products as the NCHW entry
 * points; the forward sums them in another order (G agrees to fp32 rounding), d_feat of a given d_proj is bit-identical.  A 64-texel
 * tile of F / dF is ONE contiguous 64 * C * 4 byte piece instead of C row pieces of 256 bytes, and the sparse backward is traffic-bound
 * (profiles/r05u, r05v).
 * `tiles`: NULL = the whole map (dense forward / backward, nothing cleared); otherwise the flags of bts_mark_sampled_tiles (forward) or of
 * bts_render_bwd's kept pair (backward, with clear_after as in bts_project_features_bwd_tiles). */
int bts_project_features_cl(const BtsFieldCfg* cfg, const float* feat_nhwc, const float* mlp_params, int32_t N, const uint8_t* tiles,
                            float* proj_nhwc, void* stream);
int bts_project_features_bwd_cl(const BtsFieldCfg* cfg, const float* feat_nhwc, float* d_proj_nhwc, uint8_t* tiles, const float* mlp_params,
                                int32_t N, float* d_feat_nhwc, float* d_mlp_params, int32_t clear_after, void* stream);

/* BTSNet.forward on raw points (models_bts.py:266-338): xyz (n, P, 3) -> rgb (n, P, nv*3), invalid (n, P, max(nv,1)),
 * sigma (n, P).  only_density != 0 skips the colour taps: rgb may be NULL and invalid is (n, P, 1). */
int bts_field_query(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t P, int32_t only_density,
                    float* rgb, float* invalid, float* sigma, void* stream);

/* The occupancy profile of scripts/inference_setup.py:201-229 (render_profile) in one pass: xyz (n, Y * columns, 3) is a dense grid
 * of query points with the vertical level y SLOWEST (get_pts' order, :169-187: point (y, c) at index y * columns + c).  Per column
 * c: sigma := 1 where any view flags the point invalid (:219), running sum over the levels y = 0 .. Y-1 (:224), profile (n, columns)
 * = (number of levels whose running sum is <= threshold) / Y (:225; threshold 8 in the reference).  only_density != 0: only the
 * encoder view's frustum test counts as invalid (the LiDAR / 3D-bbox evaluators' query mode, evaluator_lidar.py:300-308).
 * sigma (n, Y * columns), when given, also receives the raw densities.  Y <= 64 (the reference uses 64); needs proj_nhwc.  ABI 3.
 * Rounding: the running sum is a wave-wide parallel scan, the reference's a sequential fp32 cumsum -- on a column whose running sum
 * passes within ~2e-4 of the threshold the `<=` test can fall the other way and move that column's value by 1 / Y (the parity tests
 * compare the columns that are decided by a wider margin, tests/_cases.py: decided_columns). */
int bts_occupancy_profile(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t Y, int32_t columns, float threshold,
                          int32_t only_density, float* profile, float* sigma, void* stream);

/* Layout changes at the hand-off from the (PyTorch) encoder: F (N, C, H, W) <-> (N, H, W, C); frames (N, 3, H, W) ->
 * (N, H, W, 4) with `scale`*x + `shift` applied (encode's x*0.5+0.5, models_bts.py:82). */
int bts_nchw_to_nhwc(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int bts_nhwc_to_nchw(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int bts_pack_rgb(const float* src_nchw, float* dst_nhwc4, int32_t N, int32_t H, int32_t W, float scale, float shift,
                 void* stream);

/* gen_rays (models/common/util/util.py:244-273 + unproj_map :113-149) for full images:
 * poses_c2w (V, 4, 4), projs (V, 3, 3) -> rays (V, H, W, 8). */
int bts_gen_rays(const float* poses_c2w, const float* projs, int32_t V, int32_t H, int32_t W, float z_near, float z_far,
                 int32_t norm_dir, float* rays, void* stream);

/* Photometric loss on the renderer's patch outputs, forward AND backward in one pass.  Replaces, for criterion "l1+ssim",
 * ReconstructionLoss.__call__ (models/bts/model/loss.py:83-293): compute_errors_l1ssim (:10-18) with SSIM
 * (models/common/model/layers.py:79-150: 3x3 Gaussian window, zero padding, comp_mode), the minimum over the nv render views,
 * the invalid-ray policy (:100-118) and edge_aware_smoothness (:21-40, masked as in :262-266).
 * Rays are in PatchRaySampler order: B = n_patches * patch_h * patch_w, patch-major, then row, then column; patch_h*patch_w <= 64.
 * parts (n_patches, 4) receives per patch [sum of the rgb term, sum of the smoothness term, number of invalid rays, 0]: the caller
 * forms  loss = scale_rgb * sum(parts[:,0]) + scale_eas * sum(parts[:,1])  (scale_rgb = (lambda_coarse + lambda_fine) / B ...).
 * g_rgb (B, nv, 3) / g_depth (B), when given, receive d loss / d rgb and d loss / d depth for exactly that loss. */
typedef struct {
  const float* rgb;      /* (B, nv, 3) rendered colours per view */
  const float* depth;    /* (B) expected ray termination depth (may be NULL without edge_aware_smoothness) */
  const float* weights;  /* (B, K)      needed by invalid_policy 2   } unless invalid_wsum / invalid_any */
  const float* invalid;  /* (B, K, nv)  needed by invalid_policy 1, 2 } below are given                  */
  const float* rgb_gt;   /* (B, 3) */
  float* parts;          /* (n_patches, 4) */
  float* g_rgb;          /* (B, nv, 3) or NULL */
  float* g_depth;        /* (B) or NULL */
  int32_t n_patches, patch_h, patch_w, nv, K;
  int32_t invalid_policy;          /* 0 none, 1 strict, 2 weight_guided */
  int32_t edge_aware_smoothness;   /* 0 / 1 */
  float scale_rgb, scale_eas;
  /* ABI 2: the renderer's per-ray reductions (BtsRenderArgs.invalid_wsum / invalid_any); when given they replace weights / invalid */
  const float* invalid_wsum;   /* (B, nv) or NULL   policy 2 */
  const float* invalid_any;    /* (B, nv) or NULL   policy 1 */
} BtsLossArgs;
int bts_photometric_loss(const BtsLossArgs* args, void* stream);

/* The same loss for patches of ANY size (the trainer's default patch_size 16, sample_mode "image", the validation loss on whole frames,
 * where the "patch" of ImageRaySampler.reconstruct is the 192 x 640 frame): same BtsLossArgs, same meaning of parts (n_patches, 4),
 * same scale_rgb / scale_eas semantics of g_rgb / g_depth; every patch_h, patch_w >= 1 is accepted (areas of 64 and below too: the
 * cross-check against bts_photometric_loss, which keeps its patch_h * patch_w <= 64 limit and stays the path of the shipped
 * patch_size 8 steps).  A patch is cut into 16 x 16 tiles over up to four launches (csrc/bts_loss_tiled.hip): no float atomics, reruns
 * are bit-identical; with g_rgb == NULL and g_depth == NULL (validation under no_grad) only the forward runs.  `workspace`: at least
 * bts_photometric_loss_tiled_workspace(n_patches, patch_h, patch_w, nv) bytes of device memory (about 45 bytes per ray; any
 * alignment; contents need not be initialised or kept).  BTS_E_INVALID with a bts_last_error text, nothing launched, for: a NULL
 * required pointer or non-positive size, a workspace that is NULL or too small, more than 2^31 - 1 rays, an invalid_policy without the
 * tensors it reads (the combinations bts_photometric_loss checks). */
size_t bts_photometric_loss_tiled_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv);
int bts_photometric_loss_tiled(const BtsLossArgs* args, void* workspace, size_t workspace_bytes, void* stream);

/* The PER-PIXEL criteria of ReconstructionLoss (loss.py:43-293): criterion "l1" / "l2" (the reference's default), with or without
 * median_thresholding, under invalid_policy none / strict / weight_guided / weight_guided_diverse, plus the edge-aware smoothness term
 * of bts_photometric_loss_tiled (same formulas, its own passes: csrc/bts_loss_pixel.hip).  Rays in the flat layout of BtsLossArgs:
 * B = n * (rays per batch sample), every sample a whole number of patch_h x patch_w patches (patch-major, then row, then column).
 * The reference's quirks, kept on purpose:
 *   - e[ray, c] = min_v crit(rgb[ray, v, c] - gt[ray, c]) * keep[ray]: the minimum over the views is taken PER CHANNEL (:154-155), three
 *     channels of one pixel may pick three different views;
 *   - median_thresholding (:163-167): per batch sample the threshold is torch's LOWER median, rank (N - 1) / 2 of the N = 3 B / n masked
 *     values ascending -- invalid rays contribute zeros to that ranking, so a sample with more than half of its values masked has threshold 0
 *     and keeps only zeros; the kept set is e <= thr, ties at the threshold are ALL kept; the term is (sum of kept) / count with ONE integer
 *     count over all samples.  The selection is exact (radix on the bit pattern, 11 + 11 + 10 bits: thr is an element of e, bit for bit);
 *   - weight_guided_diverse (:109-118): a (ray, view) is flagged when (sum_k invalid w > .9) | (mean_c std_k(rgb_samps) < .01), std the
 *     unbiased one (K - 1) in fp32, mean first, then the squared deviations, k ascending; K == 1 gives NaN and the comparison is false;
 *     a ray is invalid when every view is flagged;
 *   - the gradient follows torch's amin: views tied at the minimum share it EQUALLY; sign(0) = 0 for l1, 2 d for l2; nothing flows
 *     through the threshold; the smoothness mask is the same keep flag, its clamp gradient is over the closed interval.
 * out (4) receives [rgb term = sum of kept e / count, sum over the rays of the smoothness term, number of invalid rays, count as a float]
 * (count = 3 B without median); thresholds (n) and kept (1, the count as an integer) are optional and written with median only.
 * g_rgb (B, nv, 3), when given, receives scale_rgb * d out[0] / d rgb; g_depth (B) scale_eas * d out[1] / d depth; with both NULL only
 * the forward runs.  No float atomics: every sum is a fixed-order sum of per-work-group partials, reruns are bit-identical.
 * `workspace`: at least bts_pixel_loss_workspace(B, n, patch_h, patch_w) bytes of device memory (about 18 bytes per ray and 24 KB per batch sample; any alignment;
 * contents need not be initialised or kept).  BTS_E_INVALID with a bts_last_error text, nothing launched, for: a NULL required pointer
 * (args, rgb, rgb_gt, out; depth with edge_aware_smoothness), a non-positive size, B not a multiple of n * patch_h * patch_w, more than
 * 2^29 rays, an unknown criterion or invalid_policy, policy 1 / 2 without invalid_any / invalid_wsum or invalid (and weights) with K > 0,
 * weight_guided_diverse without rgb_samps, weights or invalid, a workspace that is NULL or too small. */
typedef struct {
  const float* rgb;           /* (B, nv, 3) */
  const float* rgb_gt;        /* (B, 3) */
  const float* depth;         /* (B) or NULL without edge_aware_smoothness */
  const float* weights;       /* (B, K)      policies 2, 3 */
  const float* invalid;       /* (B, K, nv)  policies 1, 2, 3 */
  const float* invalid_wsum;  /* (B, nv) or NULL: replaces weights / invalid for policy 2 */
  const float* invalid_any;   /* (B, nv) or NULL: replaces invalid for policy 1 */
  const float* rgb_samps;     /* (B, K, nv, 3)  policy 3 */
  float* out;                 /* (4) */
  float* thresholds;          /* (n) or NULL */
  int64_t* kept;              /* (1) or NULL */
  float* g_rgb;               /* (B, nv, 3) or NULL */
  float* g_depth;             /* (B) or NULL */
  int64_t B;
  int32_t n, patch_h, patch_w, nv, K;
  int32_t criterion;               /* 1 l1, 2 l2 */
  int32_t invalid_policy;          /* 0 none, 1 strict, 2 weight_guided, 3 weight_guided_diverse */
  int32_t median_thresholding;     /* 0 / 1 */
  int32_t edge_aware_smoothness;   /* 0 / 1 */
  int32_t reserved_;
  float scale_rgb, scale_eas;
} BtsPixelLossArgs;
size_t bts_pixel_loss_workspace(int64_t B, int32_t n, int32_t patch_h, int32_t patch_w);
int bts_pixel_loss(const BtsPixelLossArgs* args, void* workspace, size_t workspace_bytes, void* stream);

/* The same criteria l1 / l2 for `channels` = C colour channels, 1 <= C <= 27 (csrc/bts_loss_pixel_c.hip; the colour targets of
 * image_processor {type: patch} have 27): rgb (B, nv, C), rgb_gt (B, C), g_rgb (B, nv, C) of the same BtsPixelLossArgs,
 *   e[ray, ch] = min_v crit(rgb[ray, v, ch] - gt[ray, ch]) * keep[ray],   out[0] = sum e / (B C),
 * out = [rgb term, 0, number of invalid rays, B C as a float].  The keep flag, the per-channel minimum over the views, amin's equally
 * shared ties, sign(0) = 0 and the fixed-order sums are bts_pixel_loss's; invalid_policy none / strict / weight_guided.  g_depth, when
 * given, receives zeros (no term reads the depth).  n, patch_h, patch_w are not read.  NOT served, BTS_E_UNSUPPORTED with a message
 * naming the option: median_thresholding, weight_guided_diverse, edge_aware_smoothness (the reference itself fails there on other than
 * 3 channels: its edge_aware_smoothness reshapes the target to 3).  `workspace`: bts_pixel_loss_channels_workspace(B) bytes (8 bytes per
 * 256 rays; any alignment; contents need not be initialised).  BTS_E_INVALID as bts_pixel_loss, and for C outside [1, 27]. */
#define BTS_PIXEL_LOSS_MAX_CHANNELS 27
size_t bts_pixel_loss_channels_workspace(int64_t B);
int bts_pixel_loss_channels(const BtsPixelLossArgs* args, int32_t channels, void* workspace, size_t workspace_bytes, void* stream);

/* The per-(ray, view) flag of weight_guided_diverse (above) as 0 / 1 floats: rgb_samps (B, K, nv, 3), weights (B, K), invalid (B, K, nv)
 * -> flags (B, nv).  Criterion "l1+ssim" with weight_guided_diverse needs no kernel of its own: these flags, handed to
 * bts_photometric_loss / _tiled as invalid_any under the strict policy, give its all_v(flag > .5) -- the diverse rule.  BTS_E_INVALID for
 * a NULL pointer or a non-positive size. */
int bts_loss_diverse_flags(const float* rgb_samps, const float* weights, const float* invalid, int64_t B, int32_t K, int32_t nv, float* flags,
                           void* stream);

/* Auto-masking (use_automasking, trainer.py:201-206 and loss.py:139-143, 157-158, 174-175).  The trainer forms, per frame, the mean
 * l1+ssim error of that frame against the loss frames and carries it as a FOURTH ground-truth channel; the loss bounds every pixel's
 * error by it.  Two pieces:
 *
 * bts_automask_errors: images (n, v, 3, H, W) fp32, the PROCESSED frames in [0, 1]; ids_loss: n_loss HOST int32 values, 1 <= n_loss <=
 * BTS_MAX_VIEWS, each in [0, v), any order, repeats allowed.  With x = scale * frame f and y_j = scale * frame ids_loss[j]:
 *   err[n, f, p] = (1 / n_loss) sum_j ( .85 mean_c ssim(x, y_j)[c, p] + .15 mean_c |x - y_j|[c, p] )
 * ssim as in bts_photometric_loss (3 x 3 Gaussian window, ZERO padding at the frame border, clamp(1 - n / d, 0, 1) / 2, C1 = 1e-4, C2 =
 * 9e-4 unscaled), plain fp32.  errors (n, v, H, W) and / or images4 (n, v, 4, H, W) = the input planes copied plus the map as plane 3
 * (the trainer's torch.cat, written by the same launch); at least one of them non-NULL.  One launch, no atomics, reruns bit-identical
 * (csrc/bts_automask.hip).  Quirks of the reference that are reproduced ON PURPOSE:
 *   - the frames, already in [0, 1], are multiplied by `scale` = .5 a second time (C1 / C2 are not scaled with them);
 *   - the partner frames are the LOSS frames although trainer.py calls them render_imgs; its .view only works when
 *     len(ids_loss) == len(ids_render);
 *   - the mean over j includes a frame's comparison with itself when f is one of ids_loss (that term is ~ 0).
 * BTS_E_INVALID, nothing launched, for: a NULL images / ids_loss, both outputs NULL, a non-positive size, n_loss outside
 * [1, BTS_MAX_VIEWS], an id outside [0, v), more than 2^31 - 1 tiles.
 *
 * bts_photometric_loss_automask / _tiled_automask / bts_pixel_loss_automask: the three loss entry points above with the per-ray threshold
 * thresh (B) = the fourth channel of rgb_gt.  Every check of the base entry point applies; thresh == NULL is BTS_E_INVALID.  Semantics:
 *   - e <- min(e, thresh) AFTER the minimum over the views, BEFORE the invalid-ray keep factor and before bts_pixel_loss' median ranking;
 *     for l1 / l2 the ray's one threshold is compared with each of its three channels, for l1+ssim with the pixel's single error;
 *   - the gradient is torch's binary min: full where e < thresh, zero where e > thresh, HALF where they are equal; nothing flows into
 *     thresh; under SSIM a bound pixel's factor multiplies its own backward coefficients before the neighbours gather them;
 *   - thresh = +inf gives the base entry point's results bit for bit.
 * The tiled form's workspace is bts_photometric_loss_tiled_automask_workspace bytes (the base's plus one float per ray).
 * DIVERGENCE from the reference, on purpose: the reference renders the fourth channel too and cuts it off first thing in the loss
 * (rgb_coarse[..., :-1]; its gradient is exactly 0) -- these kernels only ever render and read three channels per view.  One visible
 * consequence: under weight_guided_diverse the reference's diversity test (mean over the channels of std_k(rgb_samps)) would average
 * in the rendered map channel as a fourth; here it is the mean over the three colours, as without automasking. */
int bts_automask_errors(const float* images, int32_t n, int32_t v, int32_t H, int32_t W, const int32_t* ids_loss, int32_t n_loss, float scale,
                        float* errors, float* images4, void* stream);
int bts_photometric_loss_automask(const BtsLossArgs* args, const float* thresh, void* stream);
size_t bts_photometric_loss_tiled_automask_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv);
int bts_photometric_loss_tiled_automask(const BtsLossArgs* args, const float* thresh, void* workspace, size_t workspace_bytes, void* stream);
int bts_pixel_loss_automask(const BtsPixelLossArgs* args, const float* thresh, void* workspace, size_t workspace_bytes, void* stream);

/* Criterion "l1+ssim" WITH median_thresholding (loss.py:151-167): bts_photometric_loss_tiled's passes over the same BtsLossArgs, joined to
 * bts_pixel_loss' exact radix selection (csrc/bts_loss_tiled.hip has the pipeline: up to eight launches and one memset on one stream).
 * Patches of ANY size go through the 16 x 16 tiles, the 8 x 8 training patch included (it then uses a quarter of a work-group's lanes;
 * bts_photometric_loss' wave kernel sees one patch per wave and cannot rank another patch's errors).  n: batch samples, n_patches a
 * multiple of it, every sample n_patches / n consecutive patches.  thresh (B) or NULL: the automasking bound of the _automask entry points.
 * With e[p] = min(min_v e_v[p], thresh[p]) * keep[p], ONE value per pixel:
 *   thr[sample] = the element of rank (N - 1) / 2 of the sample's N = B / n values ascending; kept = { p : e[p] <= thr[sample of p] };
 *   out (4) = [sum of the kept e / count, sum over the rays of the smoothness term, number of invalid rays, count as a float], count = the
 *   size of the kept set over ALL samples; thresholds (n) and kept (1, the count as an integer) are optional.
 * args->parts (n_patches, 4) per patch: column 0 the sum of e BEFORE thresholding, columns 1 and 2 bts_photometric_loss_tiled's values bit
 * for bit (the smoothness passes are that entry's: out[1] is the fp32 number nearest to the sum of column 1, g_depth is its g_depth).
 * g_rgb (B, nv, 3) = scale_rgb * d out[0] / d rgb, g_depth (B) = scale_eas * d out[1] / d depth; both NULL: forward only.
 * The reference's quirks, kept on purpose:
 *   - the threshold is torch's LOWER median (rank (N - 1) / 2, not N / 2), exact: thr is an element of e, bit for bit;
 *   - the kept set is e <= thr: ties at the threshold are ALL kept;
 *   - ONE count over all samples divides the sum (not a mean of per-sample means);
 *   - invalid rays rank as zeros (e * keep is ranked): a sample with more than half of its rays invalid has threshold 0 and keeps only zeros;
 *   - the automasking bound is applied BEFORE the keep factor and before the ranking;
 *   - a pixel whose two best views tie exactly goes to the FIRST of them, as in every l1+ssim entry here (the reference's amin would
 *     split the gradient; the tests keep every pixel's two smallest e_v apart).
 * No gradient flows through the threshold; a kept pixel's upstream gradient is 1 / count and it hands its SSIM coefficients to its 3 x 3
 * neighbours whether or not those are kept themselves; a dropped pixel hands on nothing.  No float atomics (integer atomics build the
 * histograms, every float sum is a fixed-order sum of partials): reruns are bit-identical.
 * `workspace`: at least bts_photometric_loss_median_workspace(n_patches, patch_h, patch_w, nv, n) bytes of device memory (the tiled
 * automask layout plus one float per ray and 24 KB per batch sample; any alignment; contents need not be initialised or kept; the
 * size function returns 0 for arguments the entry would reject).  BTS_E_INVALID with a bts_last_error text, nothing launched, for: a NULL
 * required pointer (args, rgb, rgb_gt, parts, out; depth with edge_aware_smoothness), a non-positive size, n <= 0, n_patches not a
 * multiple of n, more than 2^31 - 1 rays, an invalid_policy outside 0 .. 2 or without the tensors it reads (the combinations
 * bts_photometric_loss checks), a workspace that is NULL or too small. */
size_t bts_photometric_loss_median_workspace(int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t nv, int32_t n);
int bts_photometric_loss_median(const BtsLossArgs* args, int32_t n, const float* thresh /* (B) | NULL: no automasking bound */,
                                float* out /* (4) */, float* thresholds /* (n) | NULL */, int64_t* kept /* (1) | NULL */,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The optional REGULARISERS of ReconstructionLoss (loss.py:192-245, 261-281) for one scale: alpha_reg, surfaceness, ray entropy and the
 * depth term, forward and gradient (csrc/bts_loss_reg.hip: up to five launches on one stream).  Rays in the flat patch layout of the
 * other loss entries: ray = ((s * pc + p) * patch_h + y) * patch_w + x, B = n_patches * patch_h * patch_w.  alphas (B, K) and depth (B)
 * are THIS scale's; the invalid-ray inputs are scale 0's, in one of the forms the other loss entries take (per-sample weights + invalid,
 * the renderer's invalid_wsum / invalid_any, the diverse rgb_samps + weights + invalid, or bts_loss_diverse_flags' result as invalid_any
 * under the strict policy); keep[ray] = 1 - invalid ray.  A term runs when its coefficient is > 0; a term that is off costs nothing and
 * its entry of `terms` is 0.  With K samples per ray, in plain fp32:
 *   terms[0] alpha_reg    A = sum_{k < K-1} a_k, cap = K * alpha_reg_fraction;
 *                         ray:   mean_B clamp_min(A keep - cap keep, 0)
 *                         slice: per patch row clamp_min(sum_x A keep - sum_x cap keep, 0) / patch_w, mean over the n_patches * patch_h rows
 *   terms[1] surfaceness  mean_B keep * mean_k -log(exp(-|a_k|) + exp(-|1 - a_k|))
 *   terms[2] entropy      a' = a + 1e-5, d = a' / sum_k a': mean_B keep * (-sum_k d ln d) / log2(K)
 *   terms[3] depth        mean((d[y+1] - d[y])^2) + mean((d[x+1] - d[x])^2) over the pairs inside a patch
 *   terms[4]              the number of invalid rays
 *   reg[0] = coef_alpha_reg terms[0] + coef_surfaceness terms[1] + coef_entropy terms[2] + coef_depth terms[3]
 * g_alphas (B, K) = d reg / d alphas, g_depth (B) = d reg / d depth (upstream 1); every element is written exactly once.
 * The reference's quirks, kept on purpose:
 *   - alpha_reg leaves the LAST sample out of A but counts it in cap = K * fraction (not (K - 1) * fraction); its gradient is 0 there;
 *   - under an invalid policy other than none both A and cap are multiplied by keep (an invalid ray adds 0 to a slice row's sum AND to its cap);
 *   - clamp_min's gradient is torch's: it passes at an exact tie (>=), so an invalid ray's gate is open and its gradient is keep = 0;
 *   - surfaceness is masked by keep only under an invalid policy other than none; its gradient has sign(0) = 0 for |a| and |1 - a|
 *     (hard_alpha_cap's last sample is exactly 1); the reference adds the term to the loss and never logs it;
 *   - the entropy's logarithm is natural while its normaliser is log2(K); it is masked by keep under EVERY policy (policy none has no
 *     invalid rays, so keep = 1); the reference evaluates it at scale 0 only and adds it AFTER the division by the number of scales --
 *     the caller passes coef_entropy = lambda_entropy at scale 0 and 0 elsewhere, the other coefficients as lambda / n_scales;
 *   - lambda_depth_reg and lambda_depth_smoothness name the SAME number (the differences inside a patch, never across a patch border,
 *     never masked by keep): the term is computed once, coef_depth is the sum of both.
 * DIVERGENCE, on purpose: with patch_h == 1 or patch_w == 1 the reference's depth term is NaN (the mean of an empty tensor); here
 * that is BTS_E_UNSUPPORTED.
 * No float atomics: every sum is a wave reduction, then per-work-group partials a last small launch adds in index order (in fp64,
 * rounded once); reruns are bit-identical.  `workspace`: at least bts_loss_regularisers_workspace(B, n_patches, patch_h, patch_w, K)
 * bytes of device memory (about 17 bytes per ray; any alignment; contents need not be initialised or kept; 0 for arguments the entry
 * would reject).  BTS_E_INVALID with a bts_last_error text, nothing launched, for: a NULL required pointer (args, terms, reg; alphas
 * with an alpha term, depth with the depth term), a non-positive size, B != n_patches * patch_h * patch_w, more than 2^29 rays, an unknown invalid_policy or one
 * without the tensors it reads, g_alphas without an alpha term, g_depth without the depth term, a workspace that is NULL or too small.
 * BTS_E_UNSUPPORTED for K < 2, K > 256, or the depth term with patch_h < 2 or patch_w < 2. */
typedef struct {
  const float* alphas;        /* (B, K); may be NULL when alpha_reg, surfaceness and entropy are all off */
  const float* depth;         /* (B) or NULL without the depth term */
  const float* weights;       /* (B, K_invalid)         policies 2, 3 */
  const float* invalid;       /* (B, K_invalid, nv)     policies 1, 2, 3 */
  const float* invalid_wsum;  /* (B, nv) or NULL: replaces weights / invalid for policy 2 */
  const float* invalid_any;   /* (B, nv) or NULL: replaces invalid for policy 1 */
  const float* rgb_samps;     /* (B, K_invalid, nv, 3)  policy 3 */
  float* terms;               /* (5) */
  float* reg;                 /* (1) */
  float* g_alphas;            /* (B, K) or NULL */
  float* g_depth;             /* (B) or NULL */
  int64_t B;
  int32_t n_patches, patch_h, patch_w, nv;
  int32_t K;                  /* samples per ray of alphas */
  int32_t K_invalid;          /* samples per ray of weights / invalid / rgb_samps (0 with invalid_wsum / invalid_any) */
  int32_t invalid_policy;     /* 0 none, 1 strict, 2 weight_guided, 3 weight_guided_diverse */
  int32_t alpha_reg_slice;    /* 0 ray, 1 slice */
  float alpha_reg_fraction;
  float coef_alpha_reg, coef_surfaceness, coef_entropy, coef_depth;
  int32_t reserved_;
} BtsLossRegArgs;
size_t bts_loss_regularisers_workspace(int64_t B, int32_t n_patches, int32_t patch_h, int32_t patch_w, int32_t K);
int bts_loss_regularisers(const BtsLossRegArgs* args, void* workspace, size_t workspace_bytes, void* stream);

/* PatchRaySampler.sample (models/bts/model/ray_sampler.py:125-162) on device: for each of the n samples, P patches given by
 * (view, y0, x0) triples (int32, (n, P) each; the caller draws them -- the reference uses the CPU RNG) of ph x pw pixels.
 * poses_c2w (n, v, 4, 4), projs (n, v, 3, 3), images (n, v, c, H, W) or NULL -> rays (n, P*ph*pw, 8) and, with images,
 * rgb_gt (n, P*ph*pw, c), in the reference's order (patch, row, column).  Patch pixels must lie inside the frame. */
int bts_patch_rays(const float* poses_c2w, const float* projs, const float* images, const int32_t* patch_v, const int32_t* patch_y,
                   const int32_t* patch_x, int32_t n, int32_t v, int32_t c, int32_t H, int32_t W, int32_t P, int32_t ph, int32_t pw,
                   float z_near, float z_far, int32_t norm_dir, float* rays, float* rgb_gt, void* stream);

/* NeRFRenderer.sample_coarse (nerf.py:103-123) with the uniform jitter u (B, K) in [0,1) supplied by the caller. */
int bts_sample_coarse(const float* rays, const float* u, int64_t B, int32_t K, int32_t lindisp, float* z_samp,
                      void* stream);

/* What sits between the coarse and the fine render of NeRFRenderer.forward (models/common/render/nerf.py:161-208, 356-367), and
 * sample_coarse_from_dist (:125-159), in ONE launch (csrc/bts_sample_fine.hip).  The caller draws the random numbers.
 * mode BTS_SAMPLE_FINE: rays (B, 8), weights (B, Kc), z_coarse (B, Kc), depth (B), u and t (B, Kf - Kfd) in [0, 1), noise (B, Kfd)
 * standard normal -> z_out (B, Kc + Kf) = the ascending sort of [z_coarse | sample_fine | sample_fine_depth].  With z_coarse == NULL
 * ("pieces") nothing is merged: z_out (B, Kf - Kfd) = sample_fine and z_depth_out (B, Kfd) = sample_fine_depth as drawn, unsorted (a
 * part with no draws is neither read nor written: its pointers may be NULL).
 * mode BTS_SAMPLE_FROM_DIST: weights and z_coarse (= z_samp) (B, Kc = ns), u and t (B, n_coarse) -> z_out (B, n_coarse), ascending when
 * `sorted`; rays, depth, noise, Kf and Kfd are not read.
 * Per ray, in plain fp32 with IEEE divisions and no contraction:
 *   S = sum_k (w_k + 1e-5), pdf_k = (w_k + 1e-5) / S, cdf = [0, inclusive scan of pdf] (a fixed order of summation, not the sequential one)
 *   importance draw: ind = max(upper_bound(cdf, u) - 1, 0), sv = (ind + t) / Kc, z = bts_sample_coarse's near / far map of sv
 *   depth draw:      z = max(min(depth + noise * depth_std, far), near), product and sum rounded separately
 *   from-dist:       id = clamp(upper_bound(cdf, u) - 1, 0, n_coarse - 1), borders = [z_0, (z_i + z_{i+1}) / 2, z_{ns-1}] over 1 / z under
 *                    lindisp, z = left (1 - t) + right t, 1 / z under lindisp
 * The reference's quirks, kept on purpose:
 *   - the last cdf entry is whatever fp32 gives, not 1, and ind has NO upper clamp: u at or above it gives ind = Kc and a depth beyond far;
 *   - upper_bound is searchsorted(right=True), the first entry > u, with ATen's comparison (a NaN weight makes every entry "not above u":
 *     finite samples, NOT counted below);
 *   - sv divides by the number of weights per ray Kc (the reference's self.n_coarse), also when Kf differs;
 *   - from-dist clamps the interval by n_coarse - 1, not by ns - 1: with n_coarse < ns the far intervals are never drawn;
 *   - min / max are torch's: a NaN operand gives NaN (fminf / fmaxf would drop it);
 *   - the merge orders like torch.sort: ascending, NaNs last; only the values are produced (the reference discards the permutation);
 *     z_coarse need not be sorted.
 * nan_count (int32, may be NULL): the number of NaNs among the PRODUCED samples (not the coarse ones) is ADDED to it with at most one
 * integer atomic per wave -- what the reference's `assert not torch.any(torch.isnan(...))` look at, without a synchronisation.
 * No float atomics; reruns are bit-identical.  BTS_E_INVALID with a bts_last_error text, nothing launched, for: a NULL required pointer, a
 * non-positive size, Kfd > Kf, n_coarse > ns (the reference raises there), an unknown mode.  BTS_E_UNSUPPORTED outside 2 <= Kc,
 * 1 <= Kf, Kc + Kf <= 256 (the render kernels' own limit; from-dist: 2 <= ns <= 256) or with more than 2^29 rays. */
#define BTS_SAMPLE_FINE 0
#define BTS_SAMPLE_FROM_DIST 1
typedef struct {
  const float* rays;       /* (B, 8): near = [6], far = [7] */
  const float* weights;    /* (B, Kc) */
  const float* z_coarse;   /* (B, Kc); fine mode: NULL = pieces; from-dist: z_samp */
  const float* depth;      /* (B) */
  const float* u;          /* (B, Kf - Kfd) | (B, n_coarse) */
  const float* t;          /* like u */
  const float* noise;      /* (B, Kfd) */
  float* z_out;
  float* z_depth_out;      /* pieces only: (B, Kfd) */
  int32_t* nan_count;      /* (1) or NULL */
  int64_t B;
  int32_t mode;            /* BTS_SAMPLE_FINE | BTS_SAMPLE_FROM_DIST */
  int32_t Kc;              /* weights per ray (from-dist: ns) */
  int32_t n_coarse;        /* from-dist: samples to draw */
  int32_t Kf, Kfd;         /* fine: n_fine, n_fine_depth */
  int32_t lindisp;
  int32_t sorted;          /* from-dist: sort z_out */
  float depth_std;
} BtsSampleFineArgs;
int bts_sample_fine(const BtsSampleFineArgs* args, void* stream);

/* distance_to_z (utils/projection_operations.py:4-16): depths (N, H, W), inv_K (N, 3, 3) = inverse(projs) -> z (N, H, W) */
int bts_distance_to_z(const float* depths, const float* inv_K, int32_t N, int32_t H, int32_t W, float* out, void* stream);

/* Batched inverse of N dim x dim matrices, dim = 3 or 4 (row-major).  Stands in for torch.inverse on the c2w poses in
 * BTSNet.encode (models/bts/model/models_bts.py:71) and on the intrinsics in distance_to_z (utils/projection_operations.py:9):
 * fp64 Gauss-Jordan with partial pivoting rounded to fp32, enqueued on the stream (no solver library, no host sync). */
int bts_invert_small(const float* src, float* dst, int32_t N, int32_t dim, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * ABI 7: a training step's share of the renderer as TWO calls.
 *
 * The reference's training forward (BTSWrapper.forward, models/bts/trainer.py:208-259, and the criterion call of
 * utils/base_trainer.py:287-297) is, after the CNN: encode's hand-over (models_bts.py:65-136), PatchRaySampler.sample
 * (ray_sampler.py:125-162), one render per scale (trainer.py:220-259 -> nerf.py:315-375), reconstruct (views only) and
 * ReconstructionLoss.__call__ (loss.py:83-293); autograd then walks the same chain backwards.  Entry by entry that is ~20 calls into
 * this library per step with allocator, autograd and ctypes work around each -- at exp_kitti_raw.yaml's shapes the HOST then takes
 * longer to issue the step (1.1 ms) than the GPU to run it (0.5 ms).  bts_train_step_fwd enqueues the whole forward chain, and
 * bts_train_step_bwd the whole backward chain, from one call each: the same kernels in the same order with the same arguments as the
 * entry-by-entry path (bit-identical forward results; the backward's float atomics make its summation order run-to-run variable
 * either way).  Every buffer is the caller's: nothing is allocated, nothing synchronises, the struct is only read.
 *
 * Frames: images (n, v, 3, H, W) in [-1, 1] as the data loader delivers them; x * img_scale + img_shift (0.5, 0.5: models_bts.py:82,
 * trainer.py's image processor) happens where a frame is read.  id_encoder / ids_render / ids_loss index the v frames of a batch
 * element (trainer.py:118-190 draws them per step); the patches' view index patch_v indexes ids_loss (the reference samples from
 * images_ip[:, ids_loss]).
 * Per scale s (trainer.py:220-242 "multiscale": encoder.scales; otherwise one scale): the decoder's map at ITS size (feat_shift, ABI
 * 4), this render's jitter, and the loss term on this scale's rgb / depth with scale 0's invalid-ray reductions (loss.py:100-118).
 * loss_matrix (9 x 3 n_scales, row-major): the logging dict of loss.py:219-229 and the loss itself are LINEAR in the per-scale sums
 * [rgb term, smoothness term, invalid rays] the loss pass returns; row 8 is the loss (its entries 3 s and 3 s + 1 are also the
 * coefficients d loss / d sums the backward applies), rows 0-7 the dict's other entries, in the order loss_rgb_coarse, loss_rgb_fine,
 * loss_ray_entropy, loss_depth_reg, loss_alpha_reg, loss_eas, loss_depth_smoothness, loss_invalid_ratio.
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_MAX_SCALES 4
#define BTS_MAX_LOSS_VIEWS 16

typedef struct BtsTrainScale {
  /* inputs */
  const float* feat_nchw;    /* (n, C, H >> feat_shift, W >> feat_shift) the decoder's map of this scale */
  const float* jitter;       /* (n*Bp, K) in [0, 1): this render's stratified jitter (the caller's torch.rand draw, nerf.py:112) */
  /* outputs of the forward */
  float* rgb;                /* (n*Bp, nv*3) */
  float* depth;              /* (n*Bp) */
  float* invalid_wsum;       /* (n*Bp, nv)  } BtsRenderArgs.invalid_wsum / invalid_any (ABI 2) */
  float* invalid_any;        /* (n*Bp, nv)  } */
  /* state the forward leaves for the backward (contents need no initialisation) */
  float* proj_nhwc;          /* (n, H >> s, W >> s, Hd): valid in the tiles flagged in sampled_tiles only (ABI 6) */
  uint8_t* sampled_tiles;    /* (n, tiles of the scale's map), 4-byte aligned */
  float* z_samp;             /* (n*Bp, K) */
  float* sigma_raw;          /* (n*Bp, K) */
  float* trans;              /* (n*Bp, K) */
  float* rgb_samps;          /* (n*Bp, K, nv*3) */
  float* loss_parts;         /* (n*P, 4) per-patch sums of the loss pass */
  float* g_rgb;              /* (n*Bp, nv*3) d (sum of the rgb term) / d rgb            } written by the forward's loss pass */
  float* g_depth;            /* (n*Bp)       d (sum of the smoothness term) / d depth   } */
  float* gs_rgb;             /* the two above times (loss_matrix[8][3 s], [3 s + 1]) * upstream gradient: backward scratch */
  float* gs_depth;
  /* backward */
  float* d_proj_nhwc;        /* (n, H >> s, W >> s, Hd) ALL ZERO on entry, all zero again on return (the kept pair of ABI 6) */
  uint8_t* d_proj_tiles;     /* (n, tiles)              ALL ZERO on entry, all zero again on return */
  float* d_feat_nchw;        /* (n, C, H >> s, W >> s) gradient of feat_nchw, WRITTEN by the backward, or NULL */
  int32_t feat_shift;
  int32_t feat_channels_last; /* ABI 8: 1 = feat_nchw and d_feat_nchw of this scale are channels-last, (n, h, w, C) in memory (see
                               * bts_project_features_cl); 0 = NCHW */
} BtsTrainScale;

typedef struct BtsTrainStep {
  BtsFieldCfg cfg;           /* n, H, W (frame size), C, d_hidden, ..., nv = number of render views; feat_shift is per scale (ignored
                              * here); enc_render_view as in ABI 5 (-1 is always correct) */
  int32_t v;                 /* frames per batch element */
  int32_t id_encoder;        /* ids_encoder[0] */
  int32_t ids_render[BTS_MAX_VIEWS];
  int32_t n_loss;            /* number of loss frames, <= BTS_MAX_LOSS_VIEWS */
  int32_t ids_loss[BTS_MAX_LOSS_VIEWS];
  int32_t P, ph, pw;         /* patches per batch element, patch size: Bp = P * ph * pw rays per batch element, ph * pw <= 64 */
  int32_t K;                 /* samples per ray */
  int32_t lindisp, hard_alpha_cap;          /* nerf.py:117, :285-286 */
  int32_t invalid_policy;    /* 0 none, 1 strict, 2 weight_guided (BtsLossArgs) */
  int32_t edge_aware_smoothness;
  int32_t n_scales;          /* 1 .. BTS_MAX_SCALES */
  /* 1: the scales' chains of kernels run side by side on queues of the library's own, forked from and joined back into the caller's
   * stream inside the call (the scales share nothing but read-only inputs and the atomically accumulated d_mlp_params); the backward then
   * needs bwd_workspace_bytes >= n_scales * (bts_render_bwd_workspace rounded up to 256), else it runs them one after the other.  0:
   * everything on the caller's stream, in order.  Results are the same either way (the backward's float atomics are unordered anyway). */
  int32_t concurrent_scales;
  float z_near, z_far;       /* the ray sampler's (ray_sampler.py:108-123) */
  float img_scale, img_shift;
  float loss_matrix[9 * 3 * BTS_MAX_SCALES];   /* (9, 3 n_scales) row-major, see above */
  /* inputs */
  const float* images;       /* (n, v, 3, H, W) */
  const float* Ks;           /* (n, v, 3, 3) normalised intrinsics */
  const float* poses_c2w;    /* (n, v, 4, 4) */
  const int32_t* patch_v;    /* (n, P) index into ids_loss  } the caller's draws (the reference uses the CPU RNG, */
  const int32_t* patch_y;    /* (n, P) top row              }  ray_sampler.py:141-143)                            */
  const int32_t* patch_x;    /* (n, P) left column          } */
  const float* mlp_params;   /* packed (see the top of this file) */
  const float* empty_feature;/* (C) or NULL (learn_empty) */
  /* outputs of the forward */
  float* rays;               /* (n*Bp, 8) */
  float* rgb_gt;             /* (n*Bp, 3) colours of the patch pixels in [0, 1] */
  float* loss_vals;          /* (9) loss_matrix . sums: [8] = the loss */
  /* scratch (caller-owned, contents need no initialisation) */
  float* cams;               /* n * (9 + 16 + nv * (9 + 16)) floats: K_enc (n, 9), w2c_enc (n, 16), K_r (n, nv, 9), w2c_r (n, nv, 16) */
  float* imgs_nhwc4;         /* (n, nv, H, W, 4) */
  /* max over the scales of bts_render_bwd_workspace.  BOTH calls write here.  For a scale whose map has n_tiles = n * ceil(h w / 64)
   * >= 4096 tiles (BTS_LIST_MIN_TILES of csrc/bts_prep.hip) the projection passes take their list-driven form and keep the tile list in
   * this workspace: L(n_tiles) = (4 + n_tiles) * 4 + n_tiles + 16 bytes -- int32[0] the number of flagged tiles, int32[1 .. 3] zero,
   * int32[4 ..] their indices in no particular order, and (backward only) at byte (4 + n_tiles) * 4 one byte per tile: the copy of the
   * flags the backward found in d_proj_tiles.
   *   forward:  scale s uses the slice of slice = (bwd_workspace_bytes / n_scales) & ~255 bytes that starts at byte s * slice, when
   *             slice >= L(n_tiles);
   *   backward: scale s uses the start of the workspace (with concurrent_scales: of its slice of bts_render_bwd_workspace rounded up to
   *             256 bytes, at s times that), when bts_render_bwd_workspace minus the 8 x 40 x d_hidden floats at its end >= L(n_tiles) --
   *             after the scale's render passes have read what they parked there.  One after the other, a later scale's passes overwrite
   *             an earlier scale's list.
   * A scale whose slice is too small (or whose map is smaller) takes the flag-driven form: the same results, tile by tile.
   * So a workspace must not be shared between a step whose backward is still to come and another step's forward or backward on
   * another stream; on ONE stream a forward may reuse the workspace of a pending backward (the lists are rebuilt by each call). */
  void* bwd_workspace;
  size_t bwd_workspace_bytes;
  float* d_empty_proj;       /* (Hd) or NULL */
  /* outputs of the backward */
  float* d_mlp_params;       /* packed like mlp_params, WRITTEN (zero-filled inside, then accumulated over the scales), or NULL */
  float* d_empty_feature;    /* (C) WRITTEN, or NULL */
  BtsTrainScale scale[BTS_MAX_SCALES];
} BtsTrainStep;

/* Forward: cameras (bts_invert_small on the encoder / render poses), bts_pack_rgb of the render frames, bts_patch_rays, then per scale
 * bts_mark_sampled_tiles + bts_project_features_tiles + bts_render_fwd (lean outputs: rgb, depth, the invalid-ray reductions and the
 * backward's saved state) + bts_photometric_loss, and one reduction of the per-patch sums into loss_vals. */
int bts_train_step_fwd(const BtsTrainStep* st, void* stream);
/* Backward of the above for the SAME struct contents: g_loss = device pointer to the upstream gradient of loss_vals[8] (a scalar), or
 * NULL for 1.  Per scale bts_render_bwd (adding into the kept (d_proj, tiles) pair) + bts_project_features_bwd_tiles (clear_after);
 * d_mlp_params / d_empty_feature collect every scale's contribution. */
int bts_train_step_bwd(const BtsTrainStep* st, const float* g_loss, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * ABI 7: the Monodepth2 decoder's last convolutions, the layers that PRODUCE the renderer's scale-0
 * feature map.  One operator:
 *     y = [ELU]( conv3x3( reflect_pad1( [nearest x2]( x ) ), weight ) + bias )
 * = Conv3x3 / ConvBlock of models/common/model/layers.py:11-40 (ReflectionPad2d(1) + 3 x 3 convolution [+ ELU, alpha 1]) with the
 * decoder's nearest x2 upsampling (monodepth2.py:225) folded into the read of x.  With d_out = 64 the tail is (monodepth2.py:189-239)
 *     upconv(0,0): {elu}            on (N, H/2, W/2, 64)   ->  upconv(0,1): {up2, elu}  ->  dispconv(0): {out_nchw}   at (N, H, W, 64)
 * and its last output, NCHW, is exactly what bts_project_features / bts_train_step_fwd take as feat_nchw.  Tensors are channels-last
 * (N, H, W, C) fp32 -- the memory of a torch tensor in channels_last format -- except an NCHW output when out_nchw is set.  C = 64.
 * fp32 in, fp32 out, fp32 accuracy: every operand enters the bf16 matrix pipe as the exact sum of three bf16 terms, six products per
 * pair reproduce the fp32 product to 2^-24, accumulation in fp32 (the summation order differs from a library convolution's).  A
 * non-finite input gives NaN where a library convolution gives Inf.
 * --------------------------------------------------------------------------------------------------------------------------------- */
typedef struct BtsConv3x3 {
  int32_t N, H, W;       /* OUTPUT size; the input is (N, H, W, C), or (N, H / 2, W / 2, C) with up2 (H, W even) */
  int32_t C;             /* input = output channels: 64 */
  int32_t up2;           /* 1: read x through a nearest x2 upsampling */
  int32_t elu;           /* 1: ELU on the output (ConvBlock) */
  int32_t out_nchw;      /* 1: y is (N, C, H, W); not together with elu */
  int32_t reserved_;
  const float* x;        /* input, channels-last */
  const float* weight;   /* (C, C, 3, 3) = nn.Conv2d.weight */
  const float* bias;     /* (C) or NULL */
  float* y;              /* output (written by bts_conv3x3_fwd; READ by bts_conv3x3_bwd of an ELU layer: elu' comes from the output) */
} BtsConv3x3;

int bts_conv3x3_fwd(const BtsConv3x3* c, void* stream);
/* Backward for the same struct: g_y = gradient of y in y's layout.  d_x (layout of x), d_weight (C, C, 3, 3), d_bias (C) are WRITTEN (not
 * accumulated); any of them may be NULL.  workspace: bts_conv3x3_bwd_workspace(c) bytes (g_y times elu' as a channels-last tensor + the
 * weight gradient's partial sums); contents need no initialisation.  Deterministic: no atomics anywhere. */
size_t bts_conv3x3_bwd_workspace(const BtsConv3x3* c);
int bts_conv3x3_bwd(const BtsConv3x3* c, const float* g_y, void* workspace, size_t workspace_bytes, float* d_x, float* d_weight, float* d_bias,
                    void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * ABI 7: an evaluation frame in ONE call -- BTSWrapper.forward of models/bts/evaluator.py:60-79 after the CNN: encode's hand-over
 * (models_bts.py:65-136: cameras, rgb0 packing of the render frames, the projection of the feature map), ImageRaySampler.sample
 * (ray_sampler.py:233-260: the rays of every pixel of the `n_ray_views` frames), the render with sample_coarse inside (nerf.py:315-375),
 * distance_to_z (utils/projection_operations.py:4-16).  The same kernels with the same arguments as the entry-by-entry path, enqueued
 * without the host work between them (at 1 ms per frame that is 8 % of the frame).  Every buffer is the caller's.
 * --------------------------------------------------------------------------------------------------------------------------------- */
typedef struct BtsEvalFrame {
  BtsFieldCfg cfg;           /* n, H, W, C, ..., nv = number of render (colour) views; enc_render_view as in ABI 5 */
  int32_t v;                 /* frames per batch element */
  int32_t id_encoder;
  int32_t ids_render[BTS_MAX_VIEWS];
  int32_t K, lindisp, hard_alpha_cap, norm_dir;
  float z_near, z_far;       /* the ray sampler's */
  float img_scale, img_shift;
  /* inputs */
  const float* images;       /* (n, v, 3, H, W) */
  const float* Ks;           /* (n, v, 3, 3) */
  const float* poses_c2w;    /* (n, v, 4, 4) */
  const float* feat_nchw;    /* (n, C, H, W) the encoder's scale-0 map */
  const float* mlp_params;
  const float* empty_feature;/* (C) or NULL */
  const float* jitter;       /* (n * v * H * W, K) in [0, 1) */
  /* scratch */
  float* cams;               /* n * (25 + nv * 25) floats, as in BtsTrainStep */
  float* imgs_nhwc4;         /* (n, nv, H, W, 4) */
  float* proj_nhwc;          /* (n, H, W, Hd) */
  float* inv_K;              /* (n, v, 3, 3) */
  /* outputs: rays of ALL v frames of every batch element, B = n * v * H * W */
  float* rays;               /* (B, 8) */
  float* rgb;                /* (B, nv*3) */
  float* depth;              /* (B) distance along the ray */
  float* depth_z;            /* (B) = (n, v, H, W): distance_to_z of `depth`, or NULL */
  float* weights;            /* (B, K) or NULL */
  float* alphas;             /* (B, K) or NULL */
  float* invalid;            /* (B, K, nv) or NULL */
  int32_t feat_channels_last; /* ABI 9: 1 = feat_nchw is channels-last, (n, H, W, C) in memory -- what the shipped Monodepth2 decoder writes
                              * (as BtsTrainScale.feat_channels_last, ABI 8): read as it is, no layout pass.  Appended: every ABI 8 offset stands */
  int32_t reserved_;
} BtsEvalFrame;
/* bts_eval_frame_gt (additive to ABI 9, the struct is unchanged): the same frame plus the ground-truth colours of ImageRaySampler.sample
 * (ray_sampler.py:253-258).  rgb_gt: (n, v, 3, H, W) floats, the frames' own layout, rgb_gt[i] = images[i] * img_scale + img_shift (multiply,
 * then add, each rounded: bit for bit torch's `images * .5 + .5`); the caller views it as (n, v, H, W, 3).  NULL skips it.  It is written by
 * the hand-over launch (eval_handover_kernel: cameras, inv_K, rgb0 packing, rays and rgb_gt as work-group ranges of ONE dispatch in front of
 * the projection and the render), so the frame is four dispatches: hand-over, projection, render, distance_to_z.
 * bts_eval_frame(f, stream) = bts_eval_frame_gt(f, NULL, stream). */
int bts_eval_frame_gt(const BtsEvalFrame* f, float* rgb_gt, void* stream);
int bts_eval_frame(const BtsEvalFrame* f, void* stream);
/* bts_eval_frame_sched (additive to ABI 9, the struct is unchanged): the same frame with ticket counters for the render launch.  sched: 1 024
 * bytes (256 words) of device memory owned by the caller, used by one frame at a time; the hand-over launch zeroes them.  With it the render kernel's
 * waves walk fixed lists over the first part of the rays only and claim the rest ray by ray, from one counter per XCD (sched[32 x], x = 0 .. 7: a cache line each -- claims on one line serialise),
 * as they run out (a persistent launch lasts as long as its slowest wave); a ray is still evaluated by exactly one wave iteration, every output is the same bits.  Frames
 * with too few rays per wave for a tail take the fixed lists alone.  NULL: the fixed lists alone;
 * bts_eval_frame_gt(f, rgb_gt, stream) = bts_eval_frame_sched(f, rgb_gt, NULL, stream). */
int bts_eval_frame_sched(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, void* stream);
/* bts_eval_frame_prep (additive to ABI 9, the struct is unchanged): the same frame without a packed parameter vector from the caller: the
 * launch behind the hand-over is eval_prep_kernel, the projection and the MLP (packed, and staged for the render) as work-group ranges of one dispatch.
 *   params      the MLP's own tensors, device pointers to contiguous fp32: lin_in.weight, lin_in.bias, then per ResnetBlockFC fc_0.weight,
 *               fc_0.bias, fc_1.weight, fc_1.bias, then lin_out.weight, lin_out.bias -- n_tensors = 4 + 4 * cfg.n_blocks.  Read by the
 *               launch on the stream, every frame: weights changed in place between two frames are seen.  f->mlp_params is not read.
 *   mlp_packed  scratch, bts_mlp_param_count(&f->cfg) floats: the launch writes the packed vector (the layout at the top of this header)
 *               there and the render reads it
 *   mlp_image   scratch, bts_mlp_image_floats(&f->cfg) floats on a 16-byte boundary, or NULL: the MLP as the render kernel stages it into LDS
 *               (k-major fp32 rows, the split-f16 weights and their scale, the projected empty feature), computed once by the launch; the
 *               render's work-groups copy it instead of staging it themselves, each for itself.  NULL: they stage from mlp_packed.
 * Both scratch buffers belong to one frame at a time, like `sched`.  Every output is the same bits as bts_eval_frame_sched's: the frame
 * is four dispatches as before, hand-over, prep, render, distance_to_z, and the caller's `torch.cat` of the parameters is gone. */
#define BTS_MLP_MAX_TENSORS 12
typedef struct BtsMlpTensors {
  const float* tensor[BTS_MLP_MAX_TENSORS];
  int32_t n_tensors;
  int32_t reserved_;
} BtsMlpTensors;
int64_t bts_mlp_image_floats(const BtsFieldCfg* cfg);   /* 0: a shape outside the compiled envelope */
int bts_eval_frame_prep(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, const BtsMlpTensors* params, float* mlp_packed, float* mlp_image,
                        void* stream);
/* The split that launch uses, on the host (no GPU): `grid` work-groups of four waves, `groups` rays -> the first claimed ray (= groups: no
 * tail), a multiple of 8 << *chunk_log2 (the XCD interleave's chunk, written when chunk_log2 is not NULL). */
int64_t bts_render_dyn_first(int32_t grid, int64_t groups, int32_t* chunk_log2);
/* The pinned set (additive to ABI 9, no struct changes).  A render launch with a claimed tail and a staged MLP -- bts_eval_frame_prep's with
 * `sched` and `mlp_image` -- whose arguments are the evaluation frame's under the shipped KITTI configs takes a kernel with those
 * switches compiled in: K = 64 drawn inside the kernel (jitter, no z_samp, no z_samp_out), lindisp; nv = 1 and enc_render_view = 0, feat_shift
 * = 0; code_mode 0 with inv_z, learn_empty, no empty_empty; hard_alpha_cap, no white_bkgd, no sigma_noise; rgb, depth, weights, alphas
 * and invalid given, every other output NULL.  The same arithmetic: every output is the same bits.  Any other launch takes the kernel it
 * took before.  bts_render_pinned: that test on the host (no GPU, nothing is dereferenced), 1 / 0, -1 for a NULL argument.
 * bts_eval_frame_prep_unpinned: bts_eval_frame_prep whose render launch never takes the pinned kernel (A/B and tests). */
int32_t bts_render_pinned(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a);
int bts_eval_frame_prep_unpinned(const BtsEvalFrame* f, float* rgb_gt, uint32_t* sched, const BtsMlpTensors* params, float* mlp_packed,
                                 float* mlp_image, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * MLP-predicted colour: BTSNet with sample_color=False (models_bts.py:41-42, 315-321), the PixelNeRF-style head that BTS's sampled
 * colours are compared against.  The MLP has FOUR outputs: sigma = relu(o0) (:317), rgb = sigmoid(o1..3) (:318-320); there are no
 * colour taps and one "view" (nv = 1, :321).  Additive to ABI 9: every struct and entry point above is unchanged.
 *
 * Packed parameters: as at the top of this file up to lin_out, then w_out (4 x d_hidden, row-major = nn.Linear.weight) and b_out (4);
 * w_in stays at offset 0, so bts_project_features* and their backwards serve this layout unchanged.
 * BtsFieldCfg: nv must be 1 and enc_render_view -1 (BTS_E_INVALID otherwise); C, d_hidden, n_blocks inside the envelope of
 * bts_supported (BTS_E_UNSUPPORTED otherwise).  BtsFieldTensors: proj_nhwc is required; imgs_nhwc4, K_r and w2c_r are not read (NULL is
 * fine).  Every error leaves a message and launches nothing.
 * --------------------------------------------------------------------------------------------------------------------------------- */
/* floats in mlp_params of this head: bts_mlp_param_count(cfg) + 3 d_hidden + 3; -1 for a NULL cfg */
int64_t bts_mlp_color_param_count(const BtsFieldCfg* cfg);

/* NeRFRenderer.composite (nerf.py:210-313) over BTSNet.forward with sample_color=False: per sample sigma = relu(o0) (empty_empty as in
 * bts_render_fwd), + sigma_noise, alpha = 1 - exp(-|delta| relu(sigma)) (nerf.py:279-283), hard_alpha_cap, white_bkgd, in-kernel
 * sample_coarse (jitter, z_samp_out, lindisp) and feat_shift as in bts_render_fwd.  Outputs: rgb (n*Bp, 3) = sum_k w_k sigmoid(o1..3),
 * depth, weights, alphas, invalid (n*Bp, K, 1) = the encoder view's frustum flag, rgb_samps (n*Bp, K, 3) = the per-sample colours,
 * sigma_raw = o0 before the relu, trans as in bts_render_fwd.  invalid_wsum / invalid_any are NOT produced (BTS_E_UNSUPPORTED when
 * given): the photometric loss reads weights and invalid in this mode.  K <= 256. */
int bts_render_fwd_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, void* stream);

/* Backward of bts_render_fwd_mlp_color.  Inputs: g_rgb (n*Bp, 3), g_depth, g_weights, g_alphas (any may be NULL); `a` carries z_samp and
 * the forward's sigma_raw and trans; a->rgb_samps, when given, is READ (the forward's colours).  Outputs, ACCUMULATED: d_proj_nhwc with
 * its tile flags (d_proj_tiles, the geometry of ABI 9), d_mlp_params in the four-output layout, d_empty_proj.  relu'(0) = 0 as in torch.
 * workspace: bts_render_bwd_mlp_color_workspace(cfg, a) bytes (4 (d_hidden + 1) bytes per sample: the gradient row at lin_in's output
 * and a liveness slot, + the dW_pe slot copies); contents need no initialisation. */
size_t bts_render_bwd_mlp_color_workspace(const BtsFieldCfg* cfg, const BtsRenderArgs* a);
int bts_render_bwd_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g,
                             void* workspace, size_t workspace_bytes, void* stream);

/* BTSNet.forward on raw points with sample_color=False (models_bts.py:266-338): xyz (n, P, 3) -> rgb (n, P, 3) = sigmoid(o1..3),
 * invalid (n, P, 1) = the encoder view's frustum flag, sigma (n, P) = relu(o0) (empty_empty applied).  only_density != 0: rgb, when
 * given, is written with zeros (:336). */
int bts_field_query_mlp_color(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const float* xyz, int32_t P, int32_t only_density,
                              float* rgb, float* invalid, float* sigma, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * Merged encoder views: BTSNet.encode(..., combine_ids=...) or more than one ids_encoder (models_bts.py:93-136, 190-210, 237-258; the
 * reference trainer's `frame_sample_mode: waymo-N`).  Additive to ABI 9: every struct and entry point above is unchanged.
 *
 * For a point and the encoder views v = 0 .. V-1, view v gives the projection with its frustum flag o_v, the bilinear features F_v
 * (learn_empty: empty_feature where o_v is set), the positional code PE_v of ITS (x, y, depth code) and the entry e_v = [F_v, PE_v].
 * What the reference computes, quirks included:
 *   - every encoder GROUP yields one entry: its first member with o = 0, else its first member (torch.min's tie rule on the CPU); the
 *     entry's flag is the picked member's;
 *   - a one-member group of a field WITH combine_ids enters the mean and its divisor TWICE (models_bts.py:196-209 lacks the `continue`
 *     its colour twin has): enc_mult[g] = 2;
 *   - no combine_ids and V > 1: the plain mean over the views, flag = any -- V one-member groups with enc_mult = 1;
 *   - MLP input = sum_g enc_mult[g] entry_g / T, T = sum_g enc_mult[g]; invalid_features = any of the entries' flags; empty_empty zeroes
 *     sigma on that merged flag;
 *   - colours: the same pick per RENDER group over the cfg's nv render views, one-member groups once; nv' = n_ren_groups;
 *     invalid (.., nv') = the picked render view's flag | invalid_features;
 *   - only_density with V > 1 fails in the reference: there is no such entry here.
 * lin_in is linear, so the kernels read view v's PROJECTED map G_v = F_v . w_in[:, :C]^T (bts_project_features*).
 *
 * BtsMultiViewField: view v is the ordinary single-view field (cfg[v], view[v]); of view[v] proj_nhwc, K_enc and w2c_enc are read, the
 * render views (imgs_nhwc4, K_r, w2c_r: cfg[0].nv of them), empty_feature and mlp_params come from view[0].  enc_render_view is ignored.
 * Checked before any launch, with a message (bts_last_error):
 *   BTS_E_INVALID      V < 1, V or a group count above BTS_MV_MAX_VIEWS, a group table that does not start at 0 or runs past
 *                      BTS_MV_MAX_VIEWS members, an empty group, a member index out of range, a view in two groups, a multiplicity other
 *                      than 1 or 2, a required NULL pointer
 *   BTS_E_UNSUPPORTED  views whose n / C / d_hidden / n_blocks / H / W / feat_shift / tile_blocks differ or lie outside bts_supported
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_MV_MAX_VIEWS 8
typedef struct BtsMultiViewField {
  int32_t V;                 /* encoder views */
  int32_t n_enc_groups;      /* encoder groups, 1 .. BTS_MV_MAX_VIEWS */
  int32_t n_ren_groups;      /* render groups = nv', 1 .. BTS_MV_MAX_VIEWS */
  int32_t reserved_;
  BtsFieldCfg cfg[BTS_MV_MAX_VIEWS];
  BtsFieldTensors view[BTS_MV_MAX_VIEWS];
  int32_t enc_group_start[BTS_MV_MAX_VIEWS + 1];   /* members of encoder group g: enc_member[enc_group_start[g] .. enc_group_start[g + 1]) */
  int32_t enc_member[BTS_MV_MAX_VIEWS];            /* encoder view indices 0 .. V-1, in the group's order */
  int32_t enc_mult[BTS_MV_MAX_VIEWS];              /* per encoder group: 1, or 2 for the one-member group counted twice */
  int32_t ren_group_start[BTS_MV_MAX_VIEWS + 1];
  int32_t ren_member[BTS_MV_MAX_VIEWS];            /* render view indices 0 .. cfg[0].nv - 1 */
} BtsMultiViewField;

/* NeRFRenderer.composite (nerf.py:210-313) over this field: sigma = softplus(o0); sigma_noise, hard_alpha_cap, white_bkgd, in-kernel
 * sample_coarse (jitter, z_samp_out, lindisp) and feat_shift as in bts_render_fwd.  Outputs: rgb (n*Bp, nv' * 3), depth, weights, alphas,
 * invalid (n*Bp, K, nv'), rgb_samps (n*Bp, K, nv' * 3), sigma_raw, trans, z_samp_out.  invalid_wsum / invalid_any are NOT produced
 * (BTS_E_UNSUPPORTED when given).  K <= 256 (BTS_E_UNSUPPORTED above). */
int bts_render_fwd_multi_view(const BtsMultiViewField* mv, const BtsRenderArgs* a, void* stream);

/* Backward of bts_render_fwd_multi_view, the sigma path (sampled colours carry no parameter gradient).  Inputs: g_rgb (n*Bp, nv' * 3),
 * g_depth, g_weights, g_alphas (any may be NULL); `a` carries z_samp and the forward's sigma_raw and trans; a->rgb_samps, when given, is
 * READ.  Outputs, ACCUMULATED: d_proj_views[v] (view v's projected-map gradient, NULL entries and a NULL array are skipped) with
 * d_proj_tiles_views[v] (its tile flags in ABI 9's geometry, or NULL), g->d_mlp_params, g->d_empty_proj; g->d_proj_nhwc and
 * g->d_proj_tiles are not read.  workspace: bts_render_bwd_multi_view_workspace(mv, a) bytes (0 for a NULL argument); contents need no
 * initialisation. */
size_t bts_render_bwd_multi_view_workspace(const BtsMultiViewField* mv, const BtsRenderArgs* a);
int bts_render_bwd_multi_view(const BtsMultiViewField* mv, const BtsRenderArgs* a, const BtsRenderGrads* g, float* const* d_proj_views,
                              unsigned char* const* d_proj_tiles_views, void* workspace, size_t workspace_bytes, void* stream);

/* BTSNet.forward on raw points: xyz (n, P, 3) -> rgb (n, P, nv' * 3) or NULL, invalid (n, P, nv') or NULL, sigma (n, P). */
int bts_field_query_multi_view(const BtsMultiViewField* mv, const float* xyz, int32_t P, float* rgb, float* invalid, float* sigma,
                               void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * LiDAR occupancy evaluation: the ground-truth half of models/bts/evaluator_lidar.py (BTSWrapper.forward :266-340), next to the density
 * query (bts_field_query) it is compared with.  Additive to ABI 9: every struct and entry point above is unchanged.
 *
 * Plain fp32, IEEE division and square root, no contraction; every reduction is an integer or bit-pattern atomic, so a rerun is
 * bit-identical.  Quirks of the reference that are reproduced ON PURPOSE:
 *   - check_occupancy measures the query's distance as the norm over all FOUR components of world_to_velo @ [p, 1], the homogeneous 1
 *     included (torch.norm(pts_velo, dim=-1), :136);
 *   - the occupancy vote starts at ones_like (:119): is_occupied = (1 + sum_j occupied_by_cloud_j) / T > (T - 2) / T, in fp32;
 *   - visibility comes from the FIRST cloud only (:153);
 *   - the carry that fills leading empty bins starts at the distance of the selected point with the smallest angle
 *     (slice_points_polar[0, 1], :93), not at bin 0's minimum.
 * Limits: T <= BTS_LIDAR_MAX_CLOUDS clouds, y_res <= BTS_LIDAR_MAX_SLICES slices, every cloud holds at least 360 points (the
 * reference's [:n_bins] at :90 assumes 360 SELECTED points per slice and cloud, silently) -- anything else is BTS_E_UNSUPPORTED with a
 * message and launches nothing.  What only the device could know: a (slice, cloud) that selects fewer than 360 points still gets the
 * carried-forward table of the points it has; one that selects NO point gets +inf in every distance, so `dists > surface` never holds
 * for that cloud (it can call a point occupied only through `dists < min_dist`).
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_LIDAR_MAX_CLOUDS 32
#define BTS_LIDAR_MAX_SLICES 16

/* bytes of bts_lidar_slices' bins_workspace (the per-bin minima and the smallest-angle keys; contents need no initialisation);
 * 0 outside the limits */
size_t bts_lidar_slices_workspace(int32_t T, int32_t y_res);

/* get_lidar_slices (:57-115).  points (sum N_t, 4): the clouds concatenated, 16-byte aligned; offsets: HOST array of T + 1 int32,
 * cloud t = points[offsets[t] : offsets[t + 1]], offsets[0] = 0, non-decreasing; velo_poses (T, 4, 4); borders361: the 361 bin borders
 * on the device, built by the caller as the reference builds them (torch.linspace(-pi, pi, 361), :91); slices as :59-72 from
 * (y_lo, y_hi, y_res).  Per point and slice: selected when y_world in [min_y, max_y] or |pc_world.xyz| >= max_dist (:79); angle and
 * distance of the velodyne-frame x, y (:83-84); bin i = [border_i, border_i+1) (:96); minimum distance per bin (:102), empty bins carry
 * the previous value (:101).  tables (y_res, T, 362, 2): rows of (angle, distance) with the two wrap rows of :109. */
int bts_lidar_slices(const float* points, const int32_t* offsets, int32_t T, const float* velo_poses, const float* borders361, float y_lo,
                     float y_hi, int32_t y_res, float max_dist, void* bins_workspace, float* tables, void* stream);

/* check_occupancy (:118-160).  q_pts (P, 3); tables (y_res, T, 362, 2) as above; world_to_velo (T, 4, 4) = the inverses of velo_poses
 * (bts_invert_small stands in for torch.inverse, :126).  Slice i owns the points [i * step, (i + 1) * step), step = P / y_res; the
 * remainder keeps is_occupied = (1 / T > thresh), is_visible = 0 as in the reference.  Outputs are bytes (0 / 1) of P entries each. */
int bts_lidar_occupancy(const float* q_pts, int32_t P, const float* tables, int32_t y_res, int32_t T, const float* world_to_velo,
                        float min_dist, uint8_t* is_occupied, uint8_t* is_visible, void* stream);

/* The evaluator's frame after the render (:292-330) from one call, nothing synchronised: bts_field_query with only_density on the
 * caller's encoded field (the SAME kernel with the same arguments: sigma is bit-identical to the stand-alone query; cfg->n must be 1),
 * the inverses of velo_poses and cam_pose, bts_lidar_slices, bts_lidar_occupancy, and the metrics kernel: per query point
 *   is_visible_pred = dist <= nearest border-clamped align_corners look-up of pred_depth_z at project_into_cam(p) (:163-168, :296-298)
 *   P = sigma > occ_threshold (:308),  V = is_visible | is_visible_pred (:314),  O = is_occupied & !V (:317)
 * counts[6] (zeroed inside the call) = number of points with
 *   [0] V & P   [1] V & !P   [2] !V & O & P   [3] !V & O & !P   [4] !V & !O & P   [5] !V & !O & !P
 * from which the nine metrics of :319-330 follow on the host. */
typedef struct {
  const float* q_pts;          /* (P, 3) world points (get_pts, :37-50) */
  int32_t P, T, y_res, H, W;   /* H, W: size of pred_depth_z */
  int32_t reserved_;
  const float* points;         /* as bts_lidar_slices */
  const int32_t* offsets;      /* HOST, T + 1 */
  const float* velo_poses;     /* (T, 4, 4) */
  const float* borders361;
  float y_lo, y_hi, max_dist, min_dist, occ_threshold;
  int32_t reserved2_;
  const float* pred_depth_z;   /* (H, W) predicted z-depth of the encoder view (distance_to_z of the rendered depth, :289) */
  const float* proj;           /* (3, 3) normalised intrinsics of that view, as project_into_cam multiplies them (:165) */
  const float* cam_pose;       /* (4, 4) its camera-to-world pose */
  int32_t* counts;             /* (6) */
  uint8_t* masks;              /* (3, P): P, O, V -- or NULL */
  float* sigma;                /* (P) or NULL */
  float* tables;               /* (y_res, T, 362, 2) or NULL (kept in the workspace) */
} BtsOccupancyEval;
size_t bts_occupancy_eval_workspace(int32_t P, int32_t T, int32_t y_res);
int bts_occupancy_eval(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsOccupancyEval* a, void* workspace, size_t workspace_bytes,
                       void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * Depth evaluation metrics: BTSWrapper.compute_depth_metrics of models/bts/evaluator.py:96-151 (models/bts/evaluator_nvs.py:96-139 is
 * the same function without scaling) -- what follows bts_eval_frame's depth_z in an eval_depth frame.  Additive to ABI 9: every struct
 * and entry point above is unchanged.
 *
 * Per frame: F.interpolate(pred, gt's size), nearest (:101); scaling by the ratio of the medians (:103-106) or by the least-squares
 * line (:107-114) over gt > 0; clamp (:116); over gt != 0 (:117) the terms of :122-139 in plain fp32 with IEEE division and no
 * contraction; their sums in fp64 in a fixed order.  No float atomics anywhere, so a rerun is bit-identical; nothing synchronises.
 * Quirks of the reference that are reproduced ON PURPOSE:
 *   - the scaling is fitted over gt > 0, the metrics run over gt != 0: a negative ground-truth value enters the metrics (rmse_log is
 *     then NaN, as the reference's) but not the scaling;
 *   - torch.median is the LOWER median, the element of rank (N - 1) / 2; it is found by exact radix selection on the bit patterns, so
 *     `scale` is bit-equal to the reference's, ties included;
 *   - the nearest source index is min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out in fp32, as PyTorch computes
 *     it, not the exact rational (the two differ e.g. for 26 -> 44 and 30 -> 58);
 *   - l2: x = lstsq([p, 1], g) from the five moments in fp64 (normal equations), rounded to fp32, then pred * x0 + x1 as two rounded
 *     fp32 operations.
 * Outside the contract: NaN / inf in pred or gt (nothing faults, the row is unspecified); l2 scaling with fewer than two distinct
 * predictions under the mask (non-finite coefficients where LAPACK returns the minimum-norm solution).  N = 0 gives a NaN row and zero
 * counts; N = 1 works.
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_DEPTH_METRICS_MAX_FRAMES 64
#define BTS_DEPTH_METRICS_ROW 12

typedef struct {
  const float* pred;  int32_t H, W;      /* (B, H, W) predicted z-depth */
  const float* gt;    int32_t Hg, Wg;    /* (B, Hg, Wg) ground truth, 0 = no measurement */
  int32_t B, mode;                       /* frames, each evaluated on its own (the reference: batch 1); mode 0 none, 1 median, 2 l2 */
  float clamp_lo, clamp_hi;              /* 1e-3, 80 (:116) */
  float* metrics;                        /* (B, 12): abs_rel sq_rel rmse rmse_log a1 a2 a3 scale shift n_metric n_scale reserved */
  int32_t* counts;                       /* (B, 5): n_metric, n_scale, a1, a2, a3 as integers -- or NULL */
} BtsDepthMetrics;

/* bytes of bts_depth_metrics' workspace (histograms of the radix passes, per-work-group partial sums; contents need no
 * initialisation); 0 for non-positive sizes, B > 64, an unknown mode or more than 2^30 pixels per frame */
size_t bts_depth_metrics_workspace(int32_t B, int32_t Hg, int32_t Wg, int32_t mode);

/* Enqueues, on `stream`: mode 1 -- one clear, three radix passes (11 + 11 + 10 key bits, both medians at once), the metrics pass,
 * finish; mode 2 -- the moments pass, the 2 x 2 solve, the metrics pass, finish; mode 0 -- the metrics pass, finish.  Everything is
 * validated before anything is enqueued: BTS_E_INVALID with a message for a NULL pointer, a non-positive size, B > 64, an unknown mode,
 * more than 2^30 pixels per frame or a workspace that is NULL, too small or not 16-byte aligned. */
int bts_depth_metrics(const BtsDepthMetrics* a, void* workspace, size_t workspace_bytes, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * NVS evaluation metrics: the image half of BTSWrapper.compute_nvs_metrics of models/bts/evaluator_nvs.py:141-178 -- PSNR and SSIM of
 * the rendered target view against its ground truth over the 5 % crop at eval_resolution.  (Its depth half, :96-139, is
 * bts_depth_metrics in mode 0; LPIPS, :171, stays with the caller.)  Additive to ABI 9: every struct and entry point above is unchanged.
 *
 * Per frame, with both images read where they lie through element strides (the prediction a view slice of the render's
 * (n, v, H, W, nv, 3) output, the ground truth a channel-planar view): the value at eval pixel (y, x, c) is
 * src[nearest(y)][nearest(x)][c] (F.interpolate, :154-155); the crop [y0, y1) x [x0, x1) of size h x w (:158-164);
 *   mse  = mean over the crop and the 3 channels of (pred - gt)^2,  psnr = 10 log10(R^2 / mse), +inf for mse == 0  (:170);
 *   ssim = structural_similarity(win_size=7, gaussian_weights=False, data_range=R) per channel, then the mean over channels (:169):
 *          for every crop pixel whose 7 x 7 window lies inside the crop (the interior, (h - 6) x (w - 6) pixels) the window means
 *          ux, uy, uxx, uyy, uxy of x, y, x^2, y^2, xy;  vx = cov_norm (uxx - ux^2), vy likewise, vxy = cov_norm (uxy - ux uy);
 *          C1 = (0.01 R)^2, C2 = (0.03 R)^2;  S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2));  the mean of S.
 * All arithmetic is fp64 from the fp32 inputs (skimage's, which promoted float32 images before 0.19), with no contraction; the sums
 * are per-work-group partials added in a fixed order by a second launch.  No float atomics, so a rerun is bit-identical; no resized
 * or cropped image is ever written; nothing synchronises.
 * Quirks of the reference that are reproduced ON PURPOSE:
 *   - the nearest source index is min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out in fp32, as PyTorch computes
 *     it, not the exact rational (the index of bts_depth_metrics); the same map serves both images;
 *   - the crop box is the caller's: y0 = ceil(0.05 * He), y1 = floor(0.95 * He) as the reference's Python evaluates them on doubles,
 *     x0 and x1 likewise from We; the library takes the box and does not derive it a second time;
 *   - cov_norm = 49 / 48, the sample covariance (skimage's default use_sample_covariance=True);
 *   - the mean of S runs over the interior only: skimage crops (win_size - 1) // 2 = 3 pixels from every side before it averages, so
 *     its filter's reflect border never reaches the result and there is no border mode here.
 * Outside the contract: NaN / inf in either image (nothing faults, the row is unspecified).
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_NVS_METRICS_MAX_FRAMES 64
#define BTS_NVS_METRICS_ROW 8

typedef struct {
  const float* pred; int64_t pred_sb, pred_sy, pred_sx, pred_sc;   /* element strides: frame, row, column, channel */
  const float* gt;   int64_t gt_sb,   gt_sy,   gt_sx,   gt_sc;
  int32_t B, H, W;            /* frames (each on its own), source size */
  int32_t He, We;             /* eval_resolution */
  int32_t y0, y1, x0, x1;     /* crop box at eval_resolution */
  double data_range;          /* 1 */
  double* metrics;            /* (B, 8): ssim psnr mse ssim_c0 ssim_c1 ssim_c2 n_interior n_crop */
} BtsNvsMetrics;

/* bytes of bts_nvs_metrics' workspace (per-work-group partial sums for the largest crop eval_resolution admits; contents need no
 * initialisation); 0 for non-positive sizes, B > 64 or more than 2^30 pixels per frame */
size_t bts_nvs_metrics_workspace(int32_t B, int32_t He, int32_t We);

/* Enqueues, on `stream`: the tile pass (one work-group per 16 x 32 tile of the interior and frame) and finish.  Everything is validated
 * before anything is enqueued: BTS_E_INVALID with a message for a NULL pointer, a non-positive size, B > 64, a crop box outside
 * [0, He] x [0, We], a crop side below 7 (skimage raises there), a non-positive data_range, more than 2^30 pixels per frame (source or
 * eval_resolution) or a workspace that is NULL, too small or not 16-byte aligned. */
int bts_nvs_metrics(const BtsNvsMetrics* a, void* workspace, size_t workspace_bytes, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * 3D-bounding-box occupancy evaluation: the ground-truth half of models/bts/evaluator_3dbb.py (BTSWrapper.forward :212-241, :253-299)
 * -- occupancy against KITTI-360's annotated boxes -- next to the density query it is compared with.  Additive to ABI 9: every struct
 * and entry point above is unchanged.
 *
 * Plain fp32, IEEE division and square root, no contraction; three-term dot products are summed left to right.  The only reductions are
 * int32 adds and a bit-pattern minimum of positive floats, so a rerun is bit-identical.  Everything happens in the key frame (the
 * encoder view's camera frame): rays start at the origin, the query points are given in it.  Quirks of the reference that are
 * reproduced ON PURPOSE:
 *   - EPS = 1e-4 widens BOTH sides of every slab test, lo - EPS <= n . p <= hi + EPS (:70), for the ray intercepts and for the query
 *     points alike;
 *   - an intercept counts only with p_z > 0 (:119), whatever the sign of the ray parameter;
 *   - a ray meets only the boxes whose semanticId EQUALS its label, and the label is the one of the nearest-resized label map
 *     (F.interpolate to the ray grid, :231; the fp32 source index of bts_depth_metrics, the identity when the sizes agree);
 *   - a box takes part when ANY of its vertices projects into [-1, 1]^2 with 0 < z <= max_d, and max_d is z_range[0] = 20 (:216), not
 *     the far plane: a box can be active while the rays hit it beyond max_d, and inactive while it is in view further away;
 *   - a degenerate face (two parallel edges) has the normal 0 / 0 = NaN (:54); every comparison with it is false, so that box holds
 *     no query point and stops no ray.  Nothing special-cases it: the NaN travels through the arithmetic;
 *   - a ray that no box stops has the pseudo depth +inf, and dist <= +inf calls every point on it visible (:261).
 * Limits: B <= BTS_BBOX_MAX_BOXES boxes, 1 <= V <= BTS_BBOX_MAX_VERTS vertices and 1 <= F <= BTS_BBOX_MAX_FACES faces per box --
 * beyond them BTS_E_UNSUPPORTED with a message, nothing launched.  A face index outside its box's vertices is outside the contract (it
 * is clamped into them; nothing faults).
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_BBOX_MAX_BOXES 4096
#define BTS_BBOX_MAX_VERTS 64
#define BTS_BBOX_MAX_FACES 32

/* verts_to_cam (:30-35), bbox_in_frustum (:38-44), compute_bounds (:47-60), one wave per box.  vertices (sum V_b, 3) world coordinates,
 * faces (sum F_b, 3) int32 indices LOCAL to their box; v_offsets, f_offsets: HOST arrays of B + 1 int32, offsets[0] = 0, increasing;
 * to_keyframe (4, 4) = inverse(poses[0, 0]) (bts_invert_small stands in for torch.inverse, :212); proj (3, 3) = projs[0, 0].
 * tables (B, 32, 5): (nx, ny, nz, lo, hi) per face, zeros in the rows past F_b; n_faces (B) int32; active (B) bytes. */
int bts_bbox_bounds(const float* vertices, const int32_t* faces, const int32_t* v_offsets, const int32_t* f_offsets, int32_t B,
                    const float* to_keyframe, const float* proj, float max_d, float* tables, int32_t* n_faces, uint8_t* active, void* stream);

/* bbox_intercept_labeled over all active boxes and the argmin over boxes (:102-128, :236-241), of which the reference keeps z.
 * rays (ph * pw, 8) in the library's ray layout (direction = floats 3..5; the origin is not read), ray y * pw + x; seg (hs, ws) the
 * label map as fp32; semantic_id (B) fp32.  pseudo_depth (ph, pw): min p_z over the valid candidates p = (bound_j / (n_j . d)) d of the
 * label-matching active boxes, +inf where there is none. */
int bts_bbox_pseudo_depth(const float* rays, int32_t ph, int32_t pw, const float* seg, int32_t hs, int32_t ws, const float* tables,
                          const int32_t* n_faces, const uint8_t* active, const float* semantic_id, int32_t B, float* pseudo_depth, void* stream);

/* The evaluator's frame after the render from one call, nothing synchronised: the inverse of cam_pose, bts_bbox_bounds,
 * bts_bbox_pseudo_depth, bts_field_query with only_density on the caller's encoded field (the SAME kernel with the arguments
 * bts_occupancy_eval passes; cfg->n must be 1), and the metrics kernel: per query point (key frame)
 *   dist, (gx, gy) = project_into_cam(p) (:146-150); gt, pred = the nearest border-clamped align_corners look-up of the pseudo depth and
 *   of pred_depth_z (:259-260);  V = dist <= gt | dist <= pred (:261);  O = (in_bbox of any active box) & !V (:264-275);
 *   P = sigma > occ_threshold (:286)
 * counts[7] (zeroed inside the call): [0..5] the cells of bts_occupancy_eval, in its order; [6] the number of active boxes.  The nine
 * metrics of :288-299 follow from the six cells on the host. */
typedef struct {
  const float* q_pts;             /* (P, 3) key-frame points (get_pts, :131-143) */
  int32_t P, B, ph, pw, hs, ws;   /* query points, boxes, ray grid (= size of pred_depth_z), size of seg */
  const float* vertices;          /* as bts_bbox_bounds */
  const int32_t* faces;
  const int32_t* v_offsets;       /* HOST, B + 1 */
  const int32_t* f_offsets;       /* HOST, B + 1 */
  const float* semantic_id;       /* (B) */
  const float* rays;              /* (ph * pw, 8) */
  const float* seg;               /* (hs, ws) */
  float max_d, occ_threshold;     /* z_range[0] (:216), 0.5 (:177) */
  const float* pred_depth_z;      /* (ph, pw) predicted z-depth of the half-resolution render (:251) */
  const float* proj;              /* (3, 3) normalised intrinsics of the encoder view */
  const float* cam_pose;          /* (4, 4) its camera-to-world pose, poses[0, 0] */
  int32_t* counts;                /* (7) */
  uint8_t* masks;                 /* (3, P): P, O, V -- or NULL */
  float* sigma;                   /* (P) or NULL */
  float* pseudo_depth;            /* (ph, pw) or NULL (kept in the workspace) */
  float* tables;                  /* (B, 32, 5) or NULL (kept in the workspace) */
} BtsBBoxOccupancyEval;
/* 0 outside the limits or for non-positive sizes */
size_t bts_bbox_occupancy_eval_workspace(int32_t P, int32_t B, int32_t ph, int32_t pw);
int bts_bbox_occupancy_eval(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsBBoxOccupancyEval* a, void* workspace,
                            size_t workspace_bytes, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * Novel-view frames and colour-mapped depth: what the demo scripts do around a render -- render_poses (scripts/inference_setup.py:
 * 182-198), color_tensor (utils/plotting.py:41-46) and the per-frame lines of scripts/videos/gen_vid_nvs.py:102-120,
 * gen_vid_transition.py:111-171 and gen_vid_seq.py:108-137 -- ending in uint8 panels of a (P, Hc, Wc, 3) canvas on the device.
 * Additive to ABI 9: every struct and entry point above is unchanged.  Nothing synchronises, nothing is allocated; the only
 * reductions are minima and maxima (two stages, no atomics), so a rerun is bit-identical.
 *
 * The colour map is the CALLER's table, as matplotlib holds it (Colormap._lut after _init()): N + 3 rows of three channels, rows N,
 * N + 1, N + 2 the under, over and bad colours.  The float64 output takes the float64 table, the uint8 outputs take
 * (lut * 255).astype(uint8), formed once on the host.  Index of a value x, in fp32 as numpy evaluates it on a float32 array:
 *   t = x * N;  t == N -> N - 1;  t < 0 -> under;  t >= N -> over;  NaN -> bad;  otherwise trunc(t).
 * Bytes: uint8(trunc((double)c * 255.0)), saturated to [0, 255], NaN -> 0.  A panel is written at (row0, col0) of its pose's
 * canvas; the caller zero-fills the canvas and keeps every panel inside it (checked: BTS_E_INVALID otherwise).
 * Quirks of the reference that are reproduced ON PURPOSE:
 *   - color_tensor's norm is (x - min) / (max - min) in fp32 with the image's own extrema: a constant image is 0 / 0 = NaN and takes
 *     the bad colour, and one NaN makes the whole image bad (torch's min() / max() propagate it);
 *   - x = 1 exactly folds to the last colour, nextafter(1, 2) is already "over" (matplotlib's xa == N test after the fp32 product);
 *   - the invalid mask is sum_k invalid * weights > 0.8 with the threshold as fp32 (a comparison on a float32 tensor, :192), the sum
 *     being the render epilogue's invalid_wsum;
 *   - black_invalid gives an invalid pixel the frame's maximum depth, taken over ALL pixels before any assignment (depth.max(), :195),
 *     so a maximum that sits on an invalid pixel is kept, and the colour 0;
 *   - the depth panel is ((1 / depth - 1 / d_max) / (1 / d_min - 1 / d_max)).clamp(0, 1): 1 / d_max and the denominator are Python
 *     doubles rounded ONCE to fp32 (norm_range holds the two), the per-pixel operations are fp32 with IEEE division;
 *   - the image panel is converted through double ((frame * 255).astype(uint8) on the float64 concatenation of gen_vid_nvs.py:110-120).
 * Outside the contract: NaN in the rendered depth with black_invalid (torch's max() would propagate it: so does this), values outside
 * [0, 1] in an image panel (saturated here, unspecified in numpy).
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_FRAMES_PARTIALS 64      /* per image: work-groups of the min / max pre-pass; scratch is (images, 64, 3) floats */
#define BTS_CMAP_MAX_N 65536

/* color_tensor.  x (B, h, w) fp32; norm != 0: per-image min / max first (minmax_scratch (B, 64, 3) floats, contents need no
 * initialisation; may be NULL without norm).  Outputs, at least one: out (B, h * w, 3) float64 from lut_f64 (N + 3, 3), and / or the
 * bytes of lut_u8 (N + 3, 3) into canvas (B, Hc, Wc, 3) at (row0, col0). */
int bts_colorize(const float* x, int32_t B, int32_t h, int32_t w, int32_t norm, int32_t N, const double* lut_f64, const uint8_t* lut_u8,
                 float* minmax_scratch, double* out, uint8_t* canvas, int32_t Hc, int32_t Wc, int32_t row0, int32_t col0, void* stream);

/* A float image as bytes of x * scale + shift (fp32: multiply, then add; the input panel's images * .5 + .5) into canvas (B, Hc, Wc, 3)
 * at (row0, col0).  x is read through element strides (image, row, column, channel), three channels. */
int bts_pack_u8(const float* x, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t h, int32_t w, float scale, float shift,
                uint8_t* canvas, int32_t Hc, int32_t Wc, int32_t row0, int32_t col0, void* stream);

/* One chunk of P novel poses at one (h, w), from ONE call: the rays of every pose (bts_gen_rays' ray_of_pixel with the near / far
 * planes per pose), bts_render_fwd with sample_coarse inside from `jitter` and the epilogue's invalid_wsum (weights, alphas, invalid
 * and rgb_samps are neither written nor requested), the per-frame maximum depth (black_invalid only) and the finish kernel.
 * Four launches, three without black_invalid.  finish_only != 0 skips rays and render: rgb, depth and invalid_wsum are then the caller's
 * inputs and cfg / t may be NULL.
 * Requires cfg->n == 1 and cfg->nv == 1 (the scripts' ids_encoder=[0], ids_render=[0]), sampled colours (this is bts_render_fwd's
 * field) and the projected feature map: BTS_E_UNSUPPORTED with a message otherwise. */
typedef struct {
  int32_t P, h, w, K;              /* poses of the chunk, render size, samples per ray */
  int32_t lindisp, hard_alpha_cap, norm_dir, black_invalid;
  int32_t write_masked;            /* black_invalid: also write the masked values back into rgb / depth (render_poses' return values) */
  int32_t finish_only;
  int32_t lut_N, reserved_;
  const float* poses_c2w;          /* (P, 4, 4) */
  const float* Ks;                 /* (P, 3, 3) normalised intrinsics */
  const float* near_far;           /* (P, 2) */
  const float* norm_range;         /* (P, 2): (float)(1 / d_max), (float)(1 / d_min - 1 / d_max), evaluated in double; NULL without depth panel */
  const float* jitter;             /* (P * h * w, K) of U[0, 1) */
  float* rays;                     /* scratch (P * h * w, 8) */
  float* invalid_wsum;             /* scratch (P * h * w) */
  float* frame_max;                /* scratch (P, 64, 3); may be NULL without black_invalid */
  float* rgb;                      /* out (P, h, w, 3) */
  float* depth;                    /* out (P, h, w) ray distance */
  const uint8_t* lut_u8;           /* (lut_N + 3, 3); NULL without depth panel */
  uint8_t* canvas;                 /* (P, Hc, Wc, 3) or NULL (no panels) */
  int32_t Hc, Wc;
  int32_t img_row0, img_col0;      /* image panel; a negative row0 = panel off */
  int32_t depth_row0, depth_col0;  /* depth panel; a negative row0 = panel off */
} BtsNovelViews;
int bts_novel_views(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsNovelViews* a, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * Training visualisation panels: the trainer's `visualize` (models/bts/trainer.py:430-506) up to, not including, make_grid -- for the
 * first T = min(v, 6) rendered frames of batch element 0 the eight float32, channel-planar panels it logs.  Additive to ABI 9: every
 * struct and entry point above is unchanged.  Two launches, nothing synchronises, nothing is allocated, no atomics: a rerun is
 * bit-identical.  Inputs are float32, contiguous, read where they lie; only frames [0, T) of them are touched.
 *   input_im      (T, 3, h, w)     img * .5 + .5 (multiply, then add)
 *   recon_im      (T, 3, h, w)     mean over the nv render views of rgb
 *   recon_depth   (S, T, 3, h, w)  cmap(((1 / d - 1 / z_far) / (1 / z_near - 1 / z_far)).clamp(0, 1)) per scale
 *   depth_profile (3 T, 3, K, w)   cmap(alphas[rows].clamp_min(0) / max), transposed to K x w; row 3 f + j = frame f, image row rows[j]
 *   ray_entropy   (T, 3, h, w)     cmap(-sum_k p ln p / log2(K)), p = (alphas + 1e-5) / sum_k (alphas + 1e-5)
 *   alpha_sum     (T, 3, h, w)     cmap(sum_k (alphas + 1e-5) / K)
 *   recon_mse     (T, 3, h, w)     cmap((((input_im - recon_im)^2) / 2).mean over the channels.clamp(0, 1))
 *   invalids      (T, 3, h, w)     cmap(invalid.mean over K, then over nv)
 * cmap: the caller's float64 table (lut_N + 3, 3) as for bts_colorize, the index rule stated there; a panel value is the row's double
 * rounded once to fp32.  The f_* pointers, when not NULL, receive the scalar fields the colour map is applied to.
 * Quirks of the reference that are reproduced ON PURPOSE:
 *   - the entropy is a NATURAL logarithm above and log2(K) below;
 *   - 1e-5 is added to alphas before the entropy and before the alpha sum, but not before the profile (which is taken first);
 *   - the profile is divided by ONE maximum over all 3 T rows, taken unclamped (all rows zero: 0 / 0 = NaN, the bad colour; a NaN in
 *     them makes the maximum NaN, as torch's max());
 *   - the profile rows are h / 4, h / 2 and 3 h / 4 (integer divisions; they may coincide on tiny frames);
 *   - the depth is clamped AFTER the normalisation, every step in fp32 with IEEE division (z_near, z_far are float32 tensors there):
 *     a depth of 0 is +inf -> 1 -> the last colour, a NaN stays a NaN and takes the bad colour;
 *   - a value of exactly 1 folds to the last colour (matplotlib's xa == N), a NaN takes the bad colour;
 *   - the squared error is halved before its channel mean;
 *   - recon_im is a MEAN over the render views;
 *   - alpha_sum's .clamp(-1) is a lower bound of -1, a no-op, and is not there.
 * The one divergence: the reference's in-place `alphas += 1e-5` edits the caller's render dict; here alphas and invalid are const and
 * the inputs are bit-identical after the call.  Every use of the sum includes the 1e-5, so no output differs.
 * BTS_E_INVALID with a message naming the argument: NULL pointers, T outside [1, 6] or above v, K outside [2, 256], nv outside
 * [1, BTS_MAX_VIEWS], S outside [1, BTS_MAX_SCALES], h or w outside [1, 8192], lut_N outside [1, BTS_CMAP_MAX_N]; BTS_E_WORKSPACE.
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_TRAIN_VIS_MAX_FRAMES 6
typedef struct {
  int32_t T, v, h, w;              /* frames shown, frames rendered (T = min(v, 6)), frame size */
  int32_t K, nv, S, lut_N;         /* samples per ray, render views, depth scales, colours of the table */
  float z_near, z_far;
  const float* imgs[BTS_TRAIN_VIS_MAX_FRAMES];   /* the first T: (3, h, w) each in [-1, 1], batch element 0 of the loader's list */
  const float* rgb;                /* (v, h, w, nv, 3) */
  const float* depth[BTS_MAX_SCALES];            /* the first S: (v, h, w) */
  const float* alphas;             /* (v, h, w, K) */
  const float* invalid;            /* (v, h, w, K, nv) */
  const double* lut;               /* (lut_N + 3, 3) */
  const float* z_near_far;         /* (2) on the device: read instead of z_near / z_far (the trainer holds them as tensors); or NULL */
  float *input_im, *recon_im, *recon_depth, *depth_profile, *ray_entropy, *alpha_sum, *recon_mse, *invalids;   /* out, see above */
  /* out or NULL: the fields before the colour map -- (S, T, h, w), (3 T, K, w), and (T, h, w) for the last four */
  float *f_depth, *f_profile, *f_entropy, *f_alpha_sum, *f_mse, *f_invalid;
  void* workspace;                 /* bts_train_vis_workspace bytes, 16-byte aligned; contents need no initialisation */
  size_t workspace_bytes;
} BtsTrainVis;
/* 0 outside the limits above */
size_t bts_train_vis_workspace(int32_t T, int32_t h, int32_t w, int32_t K);
int bts_train_vis(const BtsTrainVis* a, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Patch colours: the trainer's `image_processor: {type: patch}` (models/bts/trainer.py:54-69, models/bts/model/image_processor.py:
 * 69-93) on the render side.  PatchProcessor(3) turns every colour frame into 27 channels; encode(images_alt=...) makes them the colour
 * grid, and the renderer's rgb becomes (..., nv * 27).  Additive to ABI 9: every struct and entry point above is unchanged.
 *   channel order      channel (y * 3 + x) * 3 + c of the processed frame at pixel (i, j) is rgb[c] at row clamp(i + y - 1, 0, H - 1),
 *                      column clamp(j + x - 1, 0, W - 1), y, x in 0..2 (y slowest, then x, then the colour c).
 *   double clamp       the 27-channel frames are never formed.  A grid_sample(bilinear, border, align_corners=False) tap of them at a
 *                      point whose four bilinear texels are rows y_0, y_1 and columns x_0, x_1 (already clamped into the frame) with weights
 *                      w_ab is   colour[(y, x, c)] = sum_{a, b} w_ab * rgb0[clamp(y_a + y - 1), clamp(x_b + x - 1)].c   -- the texel is
 *                      shifted and clamped AGAIN, not the coordinate.  imgs_nhwc4 are the renderer's packed frames (n, nv, H, W, 4) in [0, 1].
 *   border behaviour   a sample outside a render view (or behind it) reads the clamped border colours, as padding_mode="border" does; the
 *                      flags are the render's `invalid`, these entries write none.
 * Colours are linear in the compositing weights: bts_render_fwd runs unchanged and hands its `weights` to bts_patch_color_fwd,
 *   rgb[ray, v * 27 + ch] = sum_k weights[ray, k] * colour[ray, k, v, ch]  (+ 1 - sum_k weights[ray, k] with white_bkgd),
 * and bts_patch_color_bwd returns g_weights[ray, k] = sum_{v, ch} g_rgb[ray, v * 27 + ch] * colour[ray, k, v, ch] (- sum g_rgb with
 * white_bkgd) for bts_render_bwd's g_weights: WRITTEN, not accumulated; the taps are formed again, nothing per sample is saved.  A
 * sample's position is the render kernels' (rays[0:3] + z * rays[3:6], the same projection routine).  fp32, fixed-order sums along the
 * ray, no atomics: a rerun is bit-identical.  K is any positive sample count.
 * bts_patch_color_query: the colours of n x P world points xyz (n, P, 3) -> rgb (n, P, nv * 27), BTSNet.forward(xyz)'s rgb; rays, z_samp,
 * weights, K, rays_per_sample and white_bkgd are not read.
 * Quirks of the reference that are kept ON PURPOSE:
 *   - PatchProcessor pads by REPLICATION (F.pad mode="replicate"), hence the clamps;
 *   - the centre triple, channels 12..14, is the ordinary processed frame: the 3-channel render's colours;
 *   - colours are sampled for points outside the frustum as well (they are only flagged).
 * BTS_E_INVALID with a message: NULL struct or required pointer, imgs_nhwc4 not 16-byte aligned or another pointer not 4-byte aligned,
 * non-positive n, nv, H, W (K, rays_per_sample, P where read), nv above BTS_MAX_VIEWS.  BTS_E_UNSUPPORTED: patch != 3 (the one size
 * that is compiled; an even size fails in the reference too), or more than 2^31 - 2^20 rays / points in one call.
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_PATCH_COLOR_SIZE 3
#define BTS_PATCH_COLOR_CHANNELS 27
typedef struct {
  int32_t n, nv, H, W;             /* batch elements, render views, frame size */
  int32_t K, patch, white_bkgd, reserved_;   /* samples per ray, patch size (3), rgb += 1 - sum(weights) */
  int64_t rays_per_sample;         /* rays of one batch element: B = n * rays_per_sample */
  const float* rays;               /* (B, 8) */
  const float* z_samp;             /* (B, K) the render's depths */
  const float* weights;            /* (B, K) the render's weights */
  const float* imgs_nhwc4;         /* (n, nv, H, W, 4) rgb0 */
  const float* K_r;                /* (n, nv, 3, 3) */
  const float* w2c_r;              /* (n, nv, 4, 4) */
  float* rgb;                      /* out (B, nv * 27); not read by _bwd / _query */
  float* rgb_samps;                /* out (B, K, nv * 27) or NULL: the per-sample colours */
} BtsPatchColor;
int bts_patch_color_fwd(const BtsPatchColor* a, void* stream);
int bts_patch_color_bwd(const BtsPatchColor* a, const float* g_rgb, float* g_weights, void* stream);
int bts_patch_color_query(const BtsPatchColor* a, const float* xyz, int32_t P, float* rgb, void* stream);


/* ---------------------------------------------------------------------------------------------------------------------------------
 * LiDAR ground-truth depth maps: load_depth of datasets/kitti_raw/kitti_raw_dataset.py:256-302 and of datasets/kitti_360/
 * kitti_360_dataset.py:505-539 -- the producer of bts_depth_metrics' `gt` from a raw Velodyne cloud.  The .bin read, the calibration
 * and the split files stay with the caller.  Additive to ABI 9: every struct and entry point above is unchanged.
 *
 * Per frame, from points (N, 4) fp32 whose fourth column is taken as 1, P (3, 4) and the target size (H, W); all arithmetic in P's
 * dtype (fp32 or fp64) with IEEE division and no contraction, every row of P . p accumulated left to right with one rounding per term.
 * The rules of the reference, reproduced ON PURPOSE (the plain z-buffer, the nearest point per pixel, is a DIFFERENT function):
 *   1. front filter, kitti_raw only: points with x < 0 (or NaN) are dropped first; kitti_360 drops nothing, so a point behind the
 *      camera can land in frame there with a negative depth (rule 7 removes it);
 *   2. u = P . p, px = u0 / u2, py = u1 / u2, z = u2;
 *   3. the pixel: kitti_raw x = rint(px) - 1, y = rint(py) - 1; kitti_360 x = rint((px * .5 + .5) * W), y = rint((py * .5 + .5) * H);
 *      np.round rounds half to even, which is rint;
 *   4. valid: 0 <= x < W and 0 <= y < H, compared as floating-point values (NaN and u2 == 0 fall out here, as in numpy);
 *   5. scatter depth[y, x] = z: among the valid points of one pixel the one with the HIGHEST index wins (numpy's fancy assignment);
 *   6. the "duplicates": key = y * (W - 1) + x - 1, the off-by-one of the Monodepth loaders.  Two pixels share a key exactly when
 *      they are (y, W - 1) and (y + 1, 0).  For every key held by two or more valid points, the pixel of the key's FIRST point (lowest
 *      index) receives the minimum z over ALL the key's points, the other pixel's included; the other pixel keeps rule 5.  So a pixel
 *      that holds one point can receive the depth of a point of another row;
 *   7. depth < 0 becomes 0;
 *   8. eigen_depth (kitti_raw): only 1e-3 < depth < 80 inside rows [int(0.40810811 H), int(0.99189189 H)) and columns
 *      [int(0.03594771 W), int(0.96405229 W)) survives, everything else becomes 0.
 * Closed form per pixel q with key partner q': if q and q' together hold two or more points and the lowest index among them lies in
 * q, depth[q] = min z over both pixels; otherwise depth[q] = the z of q's highest-indexed point; 0 where q holds no point.
 * Integer atomics only (count, lowest index, highest index, the minimum of z's order-preserving integer image), so a rerun is
 * bit-identical; nothing synchronises.  Outside the contract: an infinite coordinate or entry of P (nothing faults).
 * --------------------------------------------------------------------------------------------------------------------------------- */
#define BTS_LIDAR_DEPTH_MAX_FRAMES 32
#define BTS_LIDAR_DEPTH_KITTI_RAW 0
#define BTS_LIDAR_DEPTH_KITTI_360 1

typedef struct {
  const float* points;      /* (N, 4) fp32, the B clouds concatenated; 16-byte aligned */
  const int64_t* offsets;   /* HOST array of B + 1: cloud f is points[offsets[f] : offsets[f + 1]]; offsets[0] = 0, non-decreasing */
  const void* P;            /* (3, 4) fp32, or fp64 with p_fp64; one projection for all B clouds */
  int32_t B, H, W;          /* frames, target size */
  int32_t convention;       /* BTS_LIDAR_DEPTH_KITTI_RAW / _KITTI_360 */
  int32_t eigen_depth;      /* rule 8; kitti_raw only */
  int32_t p_fp64;           /* 0: P and depth are fp32; 1: fp64 */
  int32_t max_blocks;       /* production callers pass 0.  > 0 caps the points pass's grid per frame: a test's way to more than one
                             * grid trip at a small N; the map is the same, only slower */
  int32_t reserved_;
  void* depth;              /* out (B, H, W) in P's dtype */
} BtsLidarDepth;

/* bytes of bts_lidar_depth's workspace (four integers per pixel; contents need no initialisation: the call clears them); 0 for
 * arguments the entry would reject */
size_t bts_lidar_depth_workspace(int32_t B, int32_t H, int32_t W, int32_t p_fp64);

/* Enqueues, on `stream`: the clear of the workspace, the points pass (thread = point, grid-stride), the pixels pass (thread = pixel).
 * Everything is validated before anything is enqueued.  BTS_E_INVALID with a message: a NULL pointer, points not 16-byte aligned,
 * B outside [1, 32], a non-positive H or W, offsets that do not start at 0 or decrease, an unknown convention, eigen_depth with
 * kitti_360, a workspace that is NULL, too small or not 16-byte aligned.  BTS_E_UNSUPPORTED with a message: W < 2 (with W == 1 every
 * pixel shares one key), H * W >= 2^24 (above it the reference's float32 key stops being exact), N >= 2^31. */
int bts_lidar_depth(const BtsLidarDepth* a, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTS_RENDER_H */
