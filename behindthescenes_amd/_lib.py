"""ctypes binding of libbts_render.so (the C ABI in include/bts_render.h).

The library is the product: there is NO Python/torch fallback for anything it exports.  If it is missing or a call
fails, a ``BtsNativeError`` is raised."""
import ctypes as C
import os
import threading

PKG = os.path.dirname(os.path.abspath(__file__))
# The product always loads libbts_render.so from the package directory.  The profiling / A-B tools load another build of the same sources
# (the instrumented probe build, an older revision's kernels) through BTS_RENDER_LIB -- honoured ONLY together with
# BTS_ALLOW_LIB_OVERRIDE=1 and announced on stderr, so that a stale variable in somebody's shell cannot silently swap the library.
_OVERRIDE = os.environ.get("BTS_RENDER_LIB") if os.environ.get("BTS_ALLOW_LIB_OVERRIDE") == "1" else None
LIB_PATH = _OVERRIDE or os.path.join(PKG, "libbts_render.so")
ABI_VERSION = 9
BTS_MAX_SCALES = 4
BTS_MAX_LOSS_VIEWS = 16

BTS_MAX_VIEWS = 8
ERRORS = {-1: "BTS_E_INVALID", -2: "BTS_E_UNSUPPORTED", -3: "BTS_E_LAUNCH", -4: "BTS_E_WORKSPACE"}


class BtsNativeError(RuntimeError):
    pass


class BtsFieldCfg(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "H", "W", "C", "d_hidden", "n_blocks", "nv", "num_freqs", "code_mode", "inv_z",
                                         "learn_empty", "empty_empty")] + \
               [("freq_factor", C.c_float), ("d_min", C.c_float), ("d_max", C.c_float), ("feat_shift", C.c_int32), ("enc_render_view", C.c_int32),
                ("tile_blocks", C.c_int32)]       # ABI 9


class BtsFieldTensors(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("feat_nhwc", "proj_nhwc", "K_enc", "w2c_enc", "imgs_nhwc4", "K_r", "w2c_r",
                                          "empty_feature", "mlp_params")]


class BtsRenderArgs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("rays_per_sample", "K", "hard_alpha_cap", "white_bkgd")] + \
               [(k, C.c_void_p) for k in ("rays", "z_samp", "rgb", "depth", "weights", "alphas", "invalid", "rgb_samps",
                                          "sigma_raw", "trans", "invalid_wsum", "invalid_any", "sigma_noise", "jitter", "z_samp_out")] + \
               [("lindisp", C.c_int32), ("reserved_", C.c_int32)]


class BtsRenderGrads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("g_rgb", "g_depth", "g_weights", "g_alphas", "d_proj_nhwc", "d_mlp_params",
                                          "d_empty_proj", "d_proj_tiles")]


BTS_MV_MAX_VIEWS = 8


class BtsMultiViewField(C.Structure):
    """Merged encoder views (include/bts_render.h): view v is the single-view field (cfg[v], view[v]), then the encoder / render group tables."""
    _fields_ = [(k, C.c_int32) for k in ("V", "n_enc_groups", "n_ren_groups", "reserved_")] + \
               [("cfg", BtsFieldCfg * BTS_MV_MAX_VIEWS), ("view", BtsFieldTensors * BTS_MV_MAX_VIEWS),
                ("enc_group_start", C.c_int32 * (BTS_MV_MAX_VIEWS + 1)), ("enc_member", C.c_int32 * BTS_MV_MAX_VIEWS),
                ("enc_mult", C.c_int32 * BTS_MV_MAX_VIEWS), ("ren_group_start", C.c_int32 * (BTS_MV_MAX_VIEWS + 1)),
                ("ren_member", C.c_int32 * BTS_MV_MAX_VIEWS)]


class BtsLossArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rgb", "depth", "weights", "invalid", "rgb_gt", "parts", "g_rgb", "g_depth")] + \
               [(k, C.c_int32) for k in ("n_patches", "patch_h", "patch_w", "nv", "K", "invalid_policy", "edge_aware_smoothness")] + \
               [("scale_rgb", C.c_float), ("scale_eas", C.c_float)] + [(k, C.c_void_p) for k in ("invalid_wsum", "invalid_any")]


class BtsPixelLossArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rgb", "rgb_gt", "depth", "weights", "invalid", "invalid_wsum", "invalid_any", "rgb_samps", "out",
                                          "thresholds", "kept", "g_rgb", "g_depth")] + [("B", C.c_int64)] + \
               [(k, C.c_int32) for k in ("n", "patch_h", "patch_w", "nv", "K", "criterion", "invalid_policy", "median_thresholding",
                                         "edge_aware_smoothness", "reserved_")] + [("scale_rgb", C.c_float), ("scale_eas", C.c_float)]


class BtsLossRegArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("alphas", "depth", "weights", "invalid", "invalid_wsum", "invalid_any", "rgb_samps", "terms", "reg",
                                          "g_alphas", "g_depth")] + [("B", C.c_int64)] + \
               [(k, C.c_int32) for k in ("n_patches", "patch_h", "patch_w", "nv", "K", "K_invalid", "invalid_policy", "alpha_reg_slice")] + \
               [(k, C.c_float) for k in ("alpha_reg_fraction", "coef_alpha_reg", "coef_surfaceness", "coef_entropy", "coef_depth")] + \
               [("reserved_", C.c_int32)]


class BtsSampleFineArgs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rays", "weights", "z_coarse", "depth", "u", "t", "noise", "z_out", "z_depth_out", "nan_count")] + \
               [("B", C.c_int64)] + [(k, C.c_int32) for k in ("mode", "Kc", "n_coarse", "Kf", "Kfd", "lindisp", "sorted")] + \
               [("depth_std", C.c_float)]


BTS_SAMPLE_FINE, BTS_SAMPLE_FROM_DIST = 0, 1


class BtsTrainScale(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("feat_nchw", "jitter", "rgb", "depth", "invalid_wsum", "invalid_any", "proj_nhwc", "sampled_tiles",
                                          "z_samp", "sigma_raw", "trans", "rgb_samps", "loss_parts", "g_rgb", "g_depth", "gs_rgb", "gs_depth",
                                          "d_proj_nhwc", "d_proj_tiles", "d_feat_nchw")] + \
               [("feat_shift", C.c_int32), ("feat_channels_last", C.c_int32)]


class BtsTrainStep(C.Structure):
    _fields_ = [("cfg", BtsFieldCfg), ("v", C.c_int32), ("id_encoder", C.c_int32), ("ids_render", C.c_int32 * BTS_MAX_VIEWS),
                ("n_loss", C.c_int32), ("ids_loss", C.c_int32 * BTS_MAX_LOSS_VIEWS)] + \
               [(k, C.c_int32) for k in ("P", "ph", "pw", "K", "lindisp", "hard_alpha_cap", "invalid_policy", "edge_aware_smoothness", "n_scales",
                                         "concurrent_scales")] + \
               [(k, C.c_float) for k in ("z_near", "z_far", "img_scale", "img_shift")] + \
               [("loss_matrix", C.c_float * (9 * 3 * BTS_MAX_SCALES))] + \
               [(k, C.c_void_p) for k in ("images", "Ks", "poses_c2w", "patch_v", "patch_y", "patch_x", "mlp_params", "empty_feature", "rays", "rgb_gt",
                                          "loss_vals", "cams", "imgs_nhwc4", "bwd_workspace")] + \
               [("bwd_workspace_bytes", C.c_size_t)] + \
               [(k, C.c_void_p) for k in ("d_empty_proj", "d_mlp_params", "d_empty_feature")] + \
               [("scale", BtsTrainScale * BTS_MAX_SCALES)]


class BtsEvalFrame(C.Structure):
    _fields_ = [("cfg", BtsFieldCfg), ("v", C.c_int32), ("id_encoder", C.c_int32), ("ids_render", C.c_int32 * BTS_MAX_VIEWS)] + \
               [(k, C.c_int32) for k in ("K", "lindisp", "hard_alpha_cap", "norm_dir")] + \
               [(k, C.c_float) for k in ("z_near", "z_far", "img_scale", "img_shift")] + \
               [(k, C.c_void_p) for k in ("images", "Ks", "poses_c2w", "feat_nchw", "mlp_params", "empty_feature", "jitter", "cams", "imgs_nhwc4",
                                          "proj_nhwc", "inv_K", "rays", "rgb", "depth", "depth_z", "weights", "alphas", "invalid")] + \
               [("feat_channels_last", C.c_int32), ("reserved_", C.c_int32)]      # ABI 9 (appended)
    # NOT a field of the C struct (ABI 9 pins its layout): the (n, v, 3, H, W) output tensor of bts_eval_frame_gt's `rgb_gt` argument, carried
    # on the host object so that native.eval_frame(fr, stream) keeps its two-argument form for whoever wraps it
    rgb_gt = None
    # likewise: the 256-word int32 device tensor of bts_eval_frame_sched's `sched` argument (None: the render's fixed ray lists alone)
    sched = None
    # likewise: bts_eval_frame_prep's arguments as a dict -- params: the MLP's parameter tensors in the packed vector's order, packed / image:
    # the float32 scratch tensors (image may be None) -- or None: the entry points that read mlp_params
    prep = None
    # likewise: False = bts_eval_frame_prep_unpinned (the render launch never takes the kernel with the frame's switches compiled in)
    pinned = True


BTS_MLP_MAX_TENSORS = 12


class BtsMlpTensors(C.Structure):
    _fields_ = [("tensor", C.c_void_p * BTS_MLP_MAX_TENSORS), ("n_tensors", C.c_int32), ("reserved_", C.c_int32)]


class BtsConv3x3(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("N", "H", "W", "C", "up2", "elu", "out_nchw", "reserved_")] + \
               [(k, C.c_void_p) for k in ("x", "weight", "bias", "y")]


class BtsOccupancyEval(C.Structure):
    _fields_ = [("q_pts", C.c_void_p)] + [(k, C.c_int32) for k in ("P", "T", "y_res", "H", "W", "reserved_")] + \
               [(k, C.c_void_p) for k in ("points", "offsets", "velo_poses", "borders361")] + \
               [(k, C.c_float) for k in ("y_lo", "y_hi", "max_dist", "min_dist", "occ_threshold")] + [("reserved2_", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("pred_depth_z", "proj", "cam_pose", "counts", "masks", "sigma", "tables")]


class BtsDepthMetrics(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("gt", C.c_void_p), ("Hg", C.c_int32), ("Wg", C.c_int32),
                ("B", C.c_int32), ("mode", C.c_int32), ("clamp_lo", C.c_float), ("clamp_hi", C.c_float), ("metrics", C.c_void_p),
                ("counts", C.c_void_p)]


class BtsLidarDepth(C.Structure):
    _fields_ = [("points", C.c_void_p), ("offsets", C.POINTER(C.c_int64)), ("P", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("B", "H", "W", "convention", "eigen_depth", "p_fp64", "max_blocks", "reserved_")] + \
               [("depth", C.c_void_p)]


class BtsNvsMetrics(C.Structure):
    _fields_ = [("pred", C.c_void_p)] + [(k, C.c_int64) for k in ("pred_sb", "pred_sy", "pred_sx", "pred_sc")] + \
               [("gt", C.c_void_p)] + [(k, C.c_int64) for k in ("gt_sb", "gt_sy", "gt_sx", "gt_sc")] + \
               [(k, C.c_int32) for k in ("B", "H", "W", "He", "We", "y0", "y1", "x0", "x1")] + \
               [("data_range", C.c_double), ("metrics", C.c_void_p)]


class BtsBBoxOccupancyEval(C.Structure):
    _fields_ = [("q_pts", C.c_void_p)] + [(k, C.c_int32) for k in ("P", "B", "ph", "pw", "hs", "ws")] + \
               [(k, C.c_void_p) for k in ("vertices", "faces", "v_offsets", "f_offsets", "semantic_id", "rays", "seg")] + \
               [("max_d", C.c_float), ("occ_threshold", C.c_float)] + \
               [(k, C.c_void_p) for k in ("pred_depth_z", "proj", "cam_pose", "counts", "masks", "sigma", "pseudo_depth", "tables")]


class BtsNovelViews(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("P", "h", "w", "K", "lindisp", "hard_alpha_cap", "norm_dir", "black_invalid", "write_masked", "finish_only",
                                         "lut_N", "reserved_")] + \
               [(k, C.c_void_p) for k in ("poses_c2w", "Ks", "near_far", "norm_range", "jitter", "rays", "invalid_wsum", "frame_max", "rgb", "depth",
                                          "lut_u8", "canvas")] + \
               [(k, C.c_int32) for k in ("Hc", "Wc", "img_row0", "img_col0", "depth_row0", "depth_col0")]


BTS_TRAIN_VIS_MAX_FRAMES = 6


class BtsTrainVis(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("T", "v", "h", "w", "K", "nv", "S", "lut_N")] + [("z_near", C.c_float), ("z_far", C.c_float)] + \
               [("imgs", C.c_void_p * BTS_TRAIN_VIS_MAX_FRAMES), ("rgb", C.c_void_p), ("depth", C.c_void_p * BTS_MAX_SCALES)] + \
               [(k, C.c_void_p) for k in ("alphas", "invalid", "lut", "z_near_far", "input_im", "recon_im", "recon_depth", "depth_profile", "ray_entropy",
                                          "alpha_sum", "recon_mse", "invalids", "f_depth", "f_profile", "f_entropy", "f_alpha_sum", "f_mse",
                                          "f_invalid", "workspace")] + \
               [("workspace_bytes", C.c_size_t)]


BTS_PATCH_COLOR_SIZE = 3
BTS_PATCH_COLOR_CHANNELS = 27


class BtsPatchColor(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "nv", "H", "W", "K", "patch", "white_bkgd", "reserved_")] + [("rays_per_sample", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("rays", "z_samp", "weights", "imgs_nhwc4", "K_r", "w2c_r", "rgb", "rgb_samps")]


BTS_LIDAR_MAX_CLOUDS = 32
BTS_BBOX_MAX_BOXES = 4096
BTS_BBOX_MAX_VERTS = 64
BTS_BBOX_MAX_FACES = 32
BTS_DEPTH_METRICS_MAX_FRAMES = 64
BTS_DEPTH_METRICS_ROW = 12
BTS_NVS_METRICS_MAX_FRAMES = 64
BTS_NVS_METRICS_ROW = 8
BTS_LIDAR_MAX_SLICES = 16
BTS_LIDAR_DEPTH_MAX_FRAMES = 32
BTS_LIDAR_DEPTH_CONVENTIONS = {"kitti_raw": 0, "kitti_360": 1}
BTS_FRAMES_PARTIALS = 64
BTS_CMAP_MAX_N = 65536

# every symbol include/bts_render.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_I = C.c_int32
SYMBOLS = {
    "bts_abi_version": (C.c_int, []),
    "bts_last_error": (C.c_char_p, []),
    "bts_supported": (C.c_int, [C.POINTER(BtsFieldCfg)]),
    "bts_mlp_param_count": (C.c_int64, [C.POINTER(BtsFieldCfg)]),
    "bts_render_fwd": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsRenderArgs), _P]),
    "bts_render_bwd_workspace": (C.c_size_t, [C.POINTER(BtsFieldCfg), C.POINTER(BtsRenderArgs)]),
    "bts_render_bwd": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsRenderArgs),
                                 C.POINTER(BtsRenderGrads), _P, C.c_size_t, _P]),
    "bts_project_features": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _I, _P, _P]),
    "bts_project_features_bwd": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _P, _I, _P, _P, _P]),
    "bts_proj_tile_count": (C.c_int64, [C.POINTER(BtsFieldCfg)]),
    "bts_project_features_bwd_tiles": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "bts_project_features_cl": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _I, _P, _P, _P]),
    "bts_project_features_bwd_cl": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "bts_mark_sampled_tiles": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, C.POINTER(BtsRenderArgs), _P, _P]),
    "bts_project_features_tiles": (C.c_int, [C.POINTER(BtsFieldCfg), _P, _P, _I, _P, _P, _P]),
    "bts_field_query": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), _P, _I, _I, _P, _P, _P, _P]),
    "bts_occupancy_profile": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), _P, _I, _I, C.c_float, _I, _P, _P, _P]),
    "bts_nchw_to_nhwc": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "bts_nhwc_to_nchw": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "bts_pack_rgb": (C.c_int, [_P, _P, _I, _I, _I, C.c_float, C.c_float, _P]),
    "bts_gen_rays": (C.c_int, [_P, _P, _I, _I, _I, C.c_float, C.c_float, _I, _P, _P]),
    "bts_patch_rays": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _I, _P, _P, _P]),
    "bts_photometric_loss": (C.c_int, [C.POINTER(BtsLossArgs), _P]),
    # the same loss for patches of any size (16 x 16 tiles, csrc/bts_loss_tiled.hip)
    "bts_photometric_loss_tiled_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_photometric_loss_tiled": (C.c_int, [C.POINTER(BtsLossArgs), _P, C.c_size_t, _P]),
    # the per-pixel criteria l1 / l2, median thresholding, the diverse flags (csrc/bts_loss_pixel.hip)
    "bts_pixel_loss_workspace": (C.c_size_t, [C.c_int64, _I, _I, _I]),
    "bts_pixel_loss": (C.c_int, [C.POINTER(BtsPixelLossArgs), _P, C.c_size_t, _P]),
    # the criteria l1 / l2 for a run-time channel count (csrc/bts_loss_pixel_c.hip)
    "bts_pixel_loss_channels_workspace": (C.c_size_t, [C.c_int64]),
    "bts_pixel_loss_channels": (C.c_int, [C.POINTER(BtsPixelLossArgs), _I, _P, C.c_size_t, _P]),
    "bts_loss_diverse_flags": (C.c_int, [_P, _P, _P, C.c_int64, _I, _I, _P, _P]),
    # auto-masking: the error map (csrc/bts_automask.hip) and the three loss entry points with the per-ray bound `thresh`
    "bts_automask_errors": (C.c_int, [_P, _I, _I, _I, _I, C.POINTER(C.c_int32), _I, C.c_float, _P, _P, _P]),
    "bts_photometric_loss_automask": (C.c_int, [C.POINTER(BtsLossArgs), _P, _P]),
    "bts_photometric_loss_tiled_automask_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_photometric_loss_tiled_automask": (C.c_int, [C.POINTER(BtsLossArgs), _P, _P, C.c_size_t, _P]),
    "bts_pixel_loss_automask": (C.c_int, [C.POINTER(BtsPixelLossArgs), _P, _P, C.c_size_t, _P]),
    # l1+ssim with median thresholding: the tiled passes joined to the radix selection (csrc/bts_loss_tiled.hip)
    "bts_photometric_loss_median_workspace": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "bts_photometric_loss_median": (C.c_int, [C.POINTER(BtsLossArgs), _I, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # the alpha / surfaceness / entropy / depth regularisers (csrc/bts_loss_reg.hip)
    "bts_loss_regularisers_workspace": (C.c_size_t, [C.c_int64, _I, _I, _I, _I]),
    "bts_loss_regularisers": (C.c_int, [C.POINTER(BtsLossRegArgs), _P, C.c_size_t, _P]),
    "bts_sample_coarse": (C.c_int, [_P, _P, C.c_int64, _I, _I, _P, _P]),
    # importance / depth draws merged with the coarse depths, from-dist sampling (csrc/bts_sample_fine.hip)
    "bts_sample_fine": (C.c_int, [C.POINTER(BtsSampleFineArgs), _P]),
    "bts_distance_to_z": (C.c_int, [_P, _P, _I, _I, _I, _P, _P]),
    "bts_invert_small": (C.c_int, [_P, _P, _I, _I, _P]),
    "bts_train_step_fwd": (C.c_int, [C.POINTER(BtsTrainStep), _P]),
    "bts_train_step_bwd": (C.c_int, [C.POINTER(BtsTrainStep), _P, _P]),
    "bts_eval_frame": (C.c_int, [C.POINTER(BtsEvalFrame), _P]),
    "bts_eval_frame_gt": (C.c_int, [C.POINTER(BtsEvalFrame), _P, _P]),
    "bts_eval_frame_sched": (C.c_int, [C.POINTER(BtsEvalFrame), _P, _P, _P]),
    "bts_mlp_image_floats": (C.c_int64, [C.POINTER(BtsFieldCfg)]),
    "bts_eval_frame_prep": (C.c_int, [C.POINTER(BtsEvalFrame), _P, _P, C.POINTER(BtsMlpTensors), _P, _P, _P]),
    "bts_render_dyn_first": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "bts_render_pinned": (C.c_int32, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsRenderArgs)]),
    "bts_eval_frame_prep_unpinned": (C.c_int, [C.POINTER(BtsEvalFrame), _P, _P, C.POINTER(BtsMlpTensors), _P, _P, _P]),
    "bts_conv3x3_fwd": (C.c_int, [C.POINTER(BtsConv3x3), _P]),
    "bts_conv3x3_bwd_workspace": (C.c_size_t, [C.POINTER(BtsConv3x3)]),
    "bts_conv3x3_bwd": (C.c_int, [C.POINTER(BtsConv3x3), _P, _P, C.c_size_t, _P, _P, _P, _P]),
    # MLP-predicted colour (sample_color=False)
    "bts_mlp_color_param_count": (C.c_int64, [C.POINTER(BtsFieldCfg)]),
    "bts_render_fwd_mlp_color": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsRenderArgs), _P]),
    "bts_render_bwd_mlp_color_workspace": (C.c_size_t, [C.POINTER(BtsFieldCfg), C.POINTER(BtsRenderArgs)]),
    "bts_render_bwd_mlp_color": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsRenderArgs),
                                           C.POINTER(BtsRenderGrads), _P, C.c_size_t, _P]),
    "bts_field_query_mlp_color": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), _P, _I, _I, _P, _P, _P, _P]),
    # merged encoder views (combine_ids / several ids_encoder)
    "bts_render_fwd_multi_view": (C.c_int, [C.POINTER(BtsMultiViewField), C.POINTER(BtsRenderArgs), _P]),
    "bts_render_bwd_multi_view_workspace": (C.c_size_t, [C.POINTER(BtsMultiViewField), C.POINTER(BtsRenderArgs)]),
    "bts_render_bwd_multi_view": (C.c_int, [C.POINTER(BtsMultiViewField), C.POINTER(BtsRenderArgs), C.POINTER(BtsRenderGrads), C.POINTER(_P),
                                            C.POINTER(_P), _P, C.c_size_t, _P]),
    "bts_field_query_multi_view": (C.c_int, [C.POINTER(BtsMultiViewField), _P, _I, _P, _P, _P, _P]),
    # LiDAR occupancy evaluation (evaluator_lidar.py)
    "bts_lidar_slices_workspace": (C.c_size_t, [_I, _I]),
    "bts_lidar_slices": (C.c_int, [_P, C.POINTER(C.c_int32), _I, _P, _P, C.c_float, C.c_float, _I, C.c_float, _P, _P, _P]),
    "bts_lidar_occupancy": (C.c_int, [_P, _I, _P, _I, _I, _P, C.c_float, _P, _P, _P]),
    "bts_occupancy_eval_workspace": (C.c_size_t, [_I, _I, _I]),
    "bts_occupancy_eval": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsOccupancyEval), _P, C.c_size_t, _P]),
    # depth evaluation metrics (evaluator.py:96-151)
    "bts_depth_metrics_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_depth_metrics": (C.c_int, [C.POINTER(BtsDepthMetrics), _P, C.c_size_t, _P]),
    # LiDAR ground-truth depth maps (kitti_raw_dataset.py:256-302, kitti_360_dataset.py:505-539)
    "bts_lidar_depth_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_lidar_depth": (C.c_int, [C.POINTER(BtsLidarDepth), _P, C.c_size_t, _P]),
    # NVS evaluation metrics (evaluator_nvs.py:141-178 without LPIPS)
    "bts_nvs_metrics_workspace": (C.c_size_t, [_I, _I, _I]),
    "bts_nvs_metrics": (C.c_int, [C.POINTER(BtsNvsMetrics), _P, C.c_size_t, _P]),
    # 3D-bounding-box occupancy evaluation (evaluator_3dbb.py)
    "bts_bbox_bounds": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _P, C.c_float, _P, _P, _P, _P]),
    "bts_bbox_pseudo_depth": (C.c_int, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "bts_bbox_occupancy_eval_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_bbox_occupancy_eval": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsBBoxOccupancyEval), _P, C.c_size_t, _P]),
    # novel-view frames and colour-mapped depth (scripts/inference_setup.py:182-198, utils/plotting.py:41-46)
    "bts_colorize": (C.c_int, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "bts_pack_u8": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _I, _I, _I, C.c_float, C.c_float, _P, _I, _I, _I, _I, _P]),
    "bts_novel_views": (C.c_int, [C.POINTER(BtsFieldCfg), C.POINTER(BtsFieldTensors), C.POINTER(BtsNovelViews), _P]),
    # the trainer's visualisation panels (models/bts/trainer.py:430-506)
    "bts_train_vis_workspace": (C.c_size_t, [_I, _I, _I, _I]),
    "bts_train_vis": (C.c_int, [C.POINTER(BtsTrainVis), _P]),
    # patch colours (image_processor {type: patch}): the 27-channel rgb from the render's weights, its backward, the point query
    "bts_patch_color_fwd": (C.c_int, [C.POINTER(BtsPatchColor), _P]),
    "bts_patch_color_bwd": (C.c_int, [C.POINTER(BtsPatchColor), _P, _P, _P]),
    "bts_patch_color_query": (C.c_int, [C.POINTER(BtsPatchColor), _P, _I, _P, _P]),
}

_lock = threading.Lock()
_lib = None


def load():
    """Loads the shared library (once).  Raises BtsNativeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise BtsNativeError(
                f"{LIB_PATH} not found: the HIP renderer has not been built. Run `python -m behindthescenes_amd.build` "
                "(needs hipcc, no GPU). There is no fallback path.")
        if _OVERRIDE:
            import sys
            print(f"behindthescenes_amd: loading {LIB_PATH} instead of the package's libbts_render.so (BTS_RENDER_LIB + BTS_ALLOW_LIB_OVERRIDE=1)",
                  file=sys.stderr)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise BtsNativeError(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype, fn.argtypes = res, args
        # (A/B tools load an older revision's kernels through BTS_RENDER_LIB: the structs only ever grew at their ends, so a library
        # of an older ABI reads the prefix it knows -- opt-in, tools only)
        if lib.bts_abi_version() != ABI_VERSION and not (_OVERRIDE and os.environ.get("BTS_ALLOW_OLDER_ABI") == "1"
                                                         and lib.bts_abi_version() < ABI_VERSION):
            raise BtsNativeError(f"ABI mismatch: library {lib.bts_abi_version()} vs binding {ABI_VERSION}; rebuild")
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().bts_last_error().decode(errors="replace")
        raise BtsNativeError(f"{what} failed: {ERRORS.get(rc, rc)}: {msg}")
