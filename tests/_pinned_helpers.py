"""The arguments of the evaluation frame's render launch as ctypes structs, for the host test of the pinned set (bts_render_pinned): what
eval_frame_impl of bts_train.hip hands render_fwd_sched_impl for a frame of the shipped KITTI eval configuration, with switches to miss it."""
import ctypes as C

from behindthescenes_amd import _lib

_FAKE = 0x1000      # a non-NULL pointer: the predicate dereferences nothing


def frame_launch(K=64, nv=1, enc_view=0, hard_alpha_cap=1, learn_empty=1, weights=True, alphas=True, lindisp=1, code_mode=0, inv_z=1,
                 empty_empty=0, feat_shift=0, white_bkgd=0, z_samp=False, z_samp_out=False, sigma_noise=False, rgb_samps=False, sigma_raw=False,
                 trans=False, invalid_wsum=False, invalid=True, C_=64, d_hidden=64, n=1, v=2, H=24, W=160):
    cfg = _lib.BtsFieldCfg(n=n, H=H, W=W, C=C_, d_hidden=d_hidden, n_blocks=0, nv=nv, num_freqs=6, code_mode=code_mode, inv_z=inv_z,
                           learn_empty=learn_empty, empty_empty=empty_empty, freq_factor=1.5, d_min=3.0, d_max=80.0, feat_shift=feat_shift,
                           enc_render_view=enc_view, tile_blocks=0)
    t = _lib.BtsFieldTensors()
    for k in ("proj_nhwc", "K_enc", "w2c_enc", "imgs_nhwc4", "K_r", "w2c_r", "mlp_params"):
        setattr(t, k, _FAKE)
    t.empty_feature = _FAKE if learn_empty else None
    a = _lib.BtsRenderArgs(rays_per_sample=v * H * W, K=K, hard_alpha_cap=hard_alpha_cap, white_bkgd=white_bkgd, lindisp=lindisp)
    a.rays, a.jitter, a.rgb, a.depth = _FAKE, _FAKE, _FAKE, _FAKE
    for name, on in (("z_samp", z_samp), ("z_samp_out", z_samp_out), ("weights", weights), ("alphas", alphas), ("invalid", invalid),
                     ("sigma_noise", sigma_noise), ("rgb_samps", rgb_samps), ("sigma_raw", sigma_raw), ("trans", trans),
                     ("invalid_wsum", invalid_wsum)):
        setattr(a, name, _FAKE if on else None)
    return cfg, t, a


def pinned(**kw):
    cfg, t, a = frame_launch(**kw)
    return int(_lib.load().bts_render_pinned(C.byref(cfg), C.byref(t), C.byref(a)))
