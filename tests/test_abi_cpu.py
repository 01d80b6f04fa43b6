"""CPU (no GPU, no kernel launches): libbts_render.so loads and exports every symbol include/bts_render.h declares, the ctypes
structs have the C layout (checked against gcc), the host-only entry points answer, errors are loud, and the host mirror of the
reference interface keeps the reference's constructor keys and state-dict layout."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native
from behindthescenes_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bts_render.h")


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def _declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bts_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared_symbols()
    assert len(names) >= 17 and "bts_render_fwd" in names and "bts_render_bwd" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/bts_render.h but not exported"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes signature in _lib.SYMBOLS"
    assert set(_lib.SYMBOLS) == set(names)
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9


def test_ctypes_structs_match_the_c_layout():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "bts_render.h"
int main(void) {
  printf("%zu %zu\n", sizeof(BtsLossArgs), offsetof(BtsLossArgs, scale_rgb));
  printf("%zu %zu %zu %zu\n", sizeof(BtsFieldCfg), sizeof(BtsFieldTensors), sizeof(BtsRenderArgs), sizeof(BtsRenderGrads));
  printf("%zu %zu %zu %zu\n", offsetof(BtsFieldCfg, freq_factor), offsetof(BtsFieldTensors, mlp_params), offsetof(BtsRenderArgs, rays),
         offsetof(BtsRenderArgs, trans));
  printf("%zu %zu %zu\n", offsetof(BtsRenderArgs, invalid_wsum), offsetof(BtsRenderArgs, invalid_any), offsetof(BtsLossArgs, invalid_wsum));
  printf("%zu %zu\n", offsetof(BtsRenderArgs, sigma_noise), offsetof(BtsFieldCfg, feat_shift));
  printf("%zu %zu %zu %zu\n", offsetof(BtsFieldCfg, enc_render_view), offsetof(BtsRenderArgs, jitter), offsetof(BtsRenderArgs, z_samp_out),
         offsetof(BtsRenderArgs, lindisp));
  printf("%zu\n", offsetof(BtsRenderGrads, d_proj_tiles));
  printf("%zu %zu %zu %zu\n", sizeof(BtsTrainScale), sizeof(BtsTrainStep), offsetof(BtsTrainScale, feat_shift), offsetof(BtsTrainScale, d_feat_nchw));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(BtsTrainStep, ids_loss), offsetof(BtsTrainStep, loss_matrix), offsetof(BtsTrainStep, images),
         offsetof(BtsTrainStep, bwd_workspace_bytes), offsetof(BtsTrainStep, d_empty_feature), offsetof(BtsTrainStep, scale));
  printf("%zu %zu %zu\n", sizeof(BtsConv3x3), offsetof(BtsConv3x3, x), offsetof(BtsConv3x3, y));
  printf("%zu %zu %zu\n", sizeof(BtsEvalFrame), offsetof(BtsEvalFrame, images), offsetof(BtsEvalFrame, invalid));
  printf("%zu\n", offsetof(BtsTrainScale, feat_channels_last));   /* ABI 8: the former reserved_ word */
  printf("%zu\n", offsetof(BtsEvalFrame, feat_channels_last));    /* ABI 9: appended behind the last ABI 8 field */
  printf("%zu\n", offsetof(BtsFieldCfg, tile_blocks));            /* ABI 9: the tile flags' geometry, behind enc_render_view */
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    sizes = [C.sizeof(_lib.BtsFieldCfg), C.sizeof(_lib.BtsFieldTensors), C.sizeof(_lib.BtsRenderArgs), C.sizeof(_lib.BtsRenderGrads)]
    offs = [_lib.BtsFieldCfg.freq_factor.offset, _lib.BtsFieldTensors.mlp_params.offset, _lib.BtsRenderArgs.rays.offset,
            _lib.BtsRenderArgs.trans.offset]
    assert [int(x) for x in out[:2]] == [C.sizeof(_lib.BtsLossArgs), _lib.BtsLossArgs.scale_rgb.offset]
    out = out[2:]
    assert [int(x) for x in out[:4]] == sizes and [int(x) for x in out[4:8]] == offs
    # ABI 2: the loss epilogue's per-ray reductions, appended to both structs
    assert [int(x) for x in out[8:11]] == [_lib.BtsRenderArgs.invalid_wsum.offset, _lib.BtsRenderArgs.invalid_any.offset,
                                           _lib.BtsLossArgs.invalid_wsum.offset]
    # ABI 3: the density noise; ABI 4: the feature map at its own scale -- both appended
    assert [int(x) for x in out[11:13]] == [_lib.BtsRenderArgs.sigma_noise.offset, _lib.BtsFieldCfg.feat_shift.offset]
    # ABI 5: the encoder-view hint and the in-kernel sample_coarse -- appended
    assert [int(x) for x in out[13:17]] == [_lib.BtsFieldCfg.enc_render_view.offset, _lib.BtsRenderArgs.jitter.offset,
                                            _lib.BtsRenderArgs.z_samp_out.offset, _lib.BtsRenderArgs.lindisp.offset]
    # ABI 6: the tile flags of the sparse map gradient -- appended
    assert [int(x) for x in out[17:18]] == [_lib.BtsRenderGrads.d_proj_tiles.offset]
    # ABI 7: the two-call training step
    assert [int(x) for x in out[18:22]] == [C.sizeof(_lib.BtsTrainScale), C.sizeof(_lib.BtsTrainStep), _lib.BtsTrainScale.feat_shift.offset,
                                            _lib.BtsTrainScale.d_feat_nchw.offset]
    T = _lib.BtsTrainStep
    assert [int(x) for x in out[22:28]] == [T.ids_loss.offset, T.loss_matrix.offset, T.images.offset, T.bwd_workspace_bytes.offset,
                                            T.d_empty_feature.offset, T.scale.offset]
    assert [int(x) for x in out[28:31]] == [C.sizeof(_lib.BtsConv3x3), _lib.BtsConv3x3.x.offset, _lib.BtsConv3x3.y.offset]
    assert [int(x) for x in out[31:34]] == [C.sizeof(_lib.BtsEvalFrame), _lib.BtsEvalFrame.images.offset, _lib.BtsEvalFrame.invalid.offset]
    # ABI 8: the layout word of a scale's map sits where reserved_ was (same size, same offsets as ABI 7)
    assert int(out[35]) == _lib.BtsEvalFrame.feat_channels_last.offset == _lib.BtsEvalFrame.invalid.offset + 8     # ABI 9: appended
    assert int(out[36]) == _lib.BtsFieldCfg.tile_blocks.offset == _lib.BtsFieldCfg.enc_render_view.offset + 4
    assert [int(x) for x in out[34:35]] == [_lib.BtsTrainScale.feat_channels_last.offset] and _lib.BtsTrainScale.feat_channels_last.offset == _lib.BtsTrainScale.feat_shift.offset + 4


def test_host_only_entry_points(lib):
    kitti = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), nv=4)
    re10k = native._spec_cfg(native.FieldSpec(C=32, d_hidden=32, n_blocks=1), nv=2)
    assert lib.bts_supported(C.byref(kitti)) == 1 and lib.bts_supported(C.byref(re10k)) == 1
    assert lib.bts_mlp_param_count(C.byref(kitti)) == 6721 and lib.bts_mlp_param_count(C.byref(re10k)) == 4449
    odd = native._spec_cfg(native.FieldSpec(C=48, d_hidden=64, n_blocks=0))
    assert lib.bts_supported(C.byref(odd)) == 0
    many = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), nv=9)
    assert lib.bts_supported(C.byref(many)) == 0


def test_backward_workspace_is_what_the_passes_hand_each_other(lib):
    """bts_render_bwd_workspace: 20 B per sample for the plain MLP with K <= 64 (g_s + the relu gates as bits, per sample and per
    channel); the gradient row at lin_in's output (4 * d_hidden B) + g_s per sample for the ResnetBlockFC model and for K > 64 (the
    row passes of bts_bwd_blocks.hip) -- per SAMPLE, no rounding of the ray count to work-group tiles any more; behind it the slot
    copies pass C reduces dW_pe through (csrc/bts_bwd.h: kFlushSlots)."""
    def ws(spec, n, rays_per_sample, K, nv=2):
        cfg = native._spec_cfg(spec, n=n, H=8, W=8, nv=nv)
        args = _lib.BtsRenderArgs(rays_per_sample=rays_per_sample, K=K, hard_alpha_cap=1, white_bkgd=0)
        return lib.bts_render_bwd_workspace(C.byref(cfg), C.byref(args))
    kitti, re10k = native.FieldSpec(C=64, d_hidden=64, n_blocks=0), native.FieldSpec(C=32, d_hidden=32, n_blocks=1)

    def a16(b):
        return (b + 15) // 16 * 16

    def slots(hd):      # + pass C's eight slot copies of dW_pe / db_in (40 x d_hidden floats each): 80 KB at d_hidden 64
        return 8 * 40 * hd * 4
    assert ws(kitti, 16, 4096, 64) == 16 * 4096 * 64 * 20 + slots(64)                                        # 84 MB, not 1.07 GB
    assert ws(kitti, 2, 320, 16) == a16(2 * 320 * (16 * 3 + 128) * 4) + slots(64)
    assert ws(kitti, 1, 300, 128) == a16(300 * 128 * (64 + 1) * 4) + slots(64)                              # K > 64: rows
    assert ws(re10k, 24, 1024, 48) == a16(24 * 1024 * 48 * (32 + 1) * 4) + slots(32)                        # one ResnetBlockFC: rows
    # an odd number of samples: the per-sample dwords are rounded up to 8 bytes (the 64-bit per-channel masks start there)
    assert ws(kitti, 1, 3, 5) == a16((3 * 5 * 3 + 1) * 4 + 3 * 128 * 4) + slots(64)


def test_loss_workspace_sizes_are_the_recorded_ones(lib):
    """bts_photometric_loss_tiled[_automask]_workspace and bts_pixel_loss_workspace count the bytes with the layout function that
    carves the pointers (csrc/bts_host.h: Carver).  The literals were printed by the library of the commit before that function
    existed, where size and carving were two hand-kept lists: (n_patches, ph, pw, nv) on both sides of a 16 x 16 tile boundary and of
    the 256-byte rounding, the pixel form with B = n_patches * ph * pw rays in n = 1 and 2 batch samples."""
    recorded = {(1, 1, 1, 1): (1792, 2048, 27648, 51456),
                (3, 8, 8, 2): (9472, 10240, 30208, 54784),
                (2, 16, 16, 1): (23808, 25856, 35584, 60160),
                (2, 17, 33, 4): (51712, 56320, 46336, 70912),
                (1, 192, 640, 1): (5537792, 6029312, 2124800, 2149376)}
    for (n_patches, ph, pw, nv), (tiled, tiled_automask, pixel_n1, pixel_n2) in recorded.items():
        assert lib.bts_photometric_loss_tiled_workspace(n_patches, ph, pw, nv) == tiled
        assert lib.bts_photometric_loss_tiled_automask_workspace(n_patches, ph, pw, nv) == tiled_automask
        assert lib.bts_pixel_loss_workspace(n_patches * ph * pw, 1, ph, pw) == pixel_n1
        assert lib.bts_pixel_loss_workspace(n_patches * ph * pw, 2, ph, pw) == pixel_n2


def test_eval_workspace_sizes_are_the_recorded_ones(lib):
    """The five evaluation workspaces count their bytes with the layout function that carves the pointers (lidar_bins_layout,
    occ_eval_layout, bbox_eval_layout, depth_layout, nvs_layout over csrc/bts_host.h's Carver).  The literals were printed by the library
    of the commit that introduced those functions -- every buffer rounded up to 256 bytes, plus the 256 the workspace pointer's own
    rounding may cost -- so that the next change to a layout is a deliberate one.  Invalid arguments still size to 0."""
    assert lib.bts_lidar_slices_workspace(3, 2) == 9216                  # T, y_res
    assert lib.bts_occupancy_eval_workspace(1000, 3, 2) == 33536         # P, T, y_res
    assert lib.bts_bbox_occupancy_eval_workspace(1000, 5, 12, 40) == 10496   # P, boxes, ph, pw
    assert lib.bts_depth_metrics_workspace(2, 37, 121, 1) == 99840       # B, Hg, Wg, mode
    assert lib.bts_nvs_metrics_workspace(2, 48, 160) == 1280             # B, He, We
    assert (lib.bts_lidar_slices_workspace(0, 1), lib.bts_occupancy_eval_workspace(0, 1, 1), lib.bts_bbox_occupancy_eval_workspace(1, 0, 1, 1),
            lib.bts_depth_metrics_workspace(0, 1, 1, 0), lib.bts_nvs_metrics_workspace(0, 1, 1)) == (0, 0, 0, 0, 0)


def test_errors_are_codes_with_messages_never_exceptions(lib):
    assert lib.bts_render_fwd(None, None, None, None) == -1                       # BTS_E_INVALID
    assert b"NULL" in lib.bts_last_error()
    cfg = native._spec_cfg(native.FieldSpec(C=48, d_hidden=64, n_blocks=0), n=1, H=4, W=4)
    tens = _lib.BtsFieldTensors(*([1] * 9))
    assert lib.bts_render_fwd(C.byref(cfg), C.byref(tens), None, None) == -2      # BTS_E_UNSUPPORTED before anything is touched
    assert b"envelope" in lib.bts_last_error()
    assert lib.bts_invert_small(None, None, 1, 3, None) == -1
    # ABI 4: a down-scaled feature map needs frame sizes that are multiples of 2^feat_shift (checked before anything is touched)
    bad = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=36, W=100, feat_shift=3)
    assert lib.bts_render_fwd(C.byref(bad), C.byref(tens), None, None) == -1 and b"feat_shift" in lib.bts_last_error()
    assert lib.bts_project_features(C.byref(bad), 16, 16, 1, 16, None) == -1 and b"feat_shift" in lib.bts_last_error()
    raw = _lib.BtsFieldTensors(1, None, 1, 1, 1, 1, 1, 1, 1)      # raw features only: the kernels that read them know full-size maps
    ok_size = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=32, W=96, feat_shift=2)
    assert lib.bts_render_fwd(C.byref(ok_size), C.byref(raw), None, None) == -1 and b"proj_nhwc" in lib.bts_last_error()
    # ABI 5: enc_render_view must name a render view (or be -1); a render call needs z_samp or the jitter
    hint = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=32, W=96, nv=2)
    hint.enc_render_view = 2
    assert lib.bts_render_fwd(C.byref(hint), C.byref(tens), None, None) == -1 and b"enc_render_view" in lib.bts_last_error()
    hint.enc_render_view = 1
    args = _lib.BtsRenderArgs(rays_per_sample=8, K=4, rays=1, rgb=1, depth=1)       # neither z_samp nor jitter
    assert lib.bts_render_fwd(C.byref(hint), C.byref(tens), C.byref(args), None) == -1 and b"jitter" in lib.bts_last_error()
    # ABI 6: tiles of 64 texels of the map in memory; the tile backward wants its flag array
    assert lib.bts_proj_tile_count(C.byref(native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=192, W=640))) == 1920
    assert lib.bts_proj_tile_count(C.byref(ok_size)) == (8 * 24 + 63) // 64
    # an invalid cfg (H, W not multiples of 2^feat_shift; a shift beyond 6) answers -1 with a message -- never 0: a caller sizing its flag
    # array with that would hand the kernels no flags; shifts 4 .. 6 are as valid here as in every entry point that takes the flags
    assert lib.bts_proj_tile_count(C.byref(bad)) == -1 and b"feat_shift" in lib.bts_last_error()
    deep = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=192, W=640, feat_shift=5)
    assert lib.bts_proj_tile_count(C.byref(deep)) == (6 * 20 + 63) // 64
    deep.feat_shift = 7
    assert lib.bts_proj_tile_count(C.byref(deep)) == -1
    assert lib.bts_proj_tile_count(None) == -1
    # ABI 7: the two-call training step validates the whole struct before anything is enqueued
    assert lib.bts_train_step_fwd(None, None) == -1 and b"NULL" in lib.bts_last_error()
    st = _lib.BtsTrainStep()
    st.cfg = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=2, H=48, W=160, nv=2)
    st.v, st.P, st.ph, st.pw, st.K, st.n_scales, st.n_loss = 4, 4, 8, 8, 64, 1, 2
    st.ids_render[0], st.ids_render[1], st.ids_loss[1] = 2, 3, 1
    assert lib.bts_train_step_fwd(C.byref(st), None) == -1 and b"NULL input" in lib.bts_last_error()
    st.ids_render[1] = 9
    assert lib.bts_train_step_bwd(C.byref(st), None, None) == -1 and b"frame id" in lib.bts_last_error()
    st.ids_render[1], st.pw = 3, 16
    assert lib.bts_train_step_fwd(C.byref(st), None) == -1 and b"64 pixels" in lib.bts_last_error()
    st.pw, st.cfg.C = 8, 48
    assert lib.bts_train_step_fwd(C.byref(st), None) == -2 and b"envelope" in lib.bts_last_error()
    # ABI 7: the decoder-tail convolution
    cv = _lib.BtsConv3x3(N=1, H=8, W=8, C=32, x=16, weight=16, y=16)
    assert lib.bts_conv3x3_fwd(C.byref(cv), None) == -1 and b"C != 64" in lib.bts_last_error()
    cv.C, cv.up2, cv.H = 64, 1, 7
    assert lib.bts_conv3x3_fwd(C.byref(cv), None) == -1
    cv.up2, cv.H = 0, 8
    assert lib.bts_conv3x3_bwd(C.byref(cv), 16, None, 0, 16, 16, 16, None) == -4 and b"workspace" in lib.bts_last_error()
    assert lib.bts_conv3x3_bwd_workspace(C.byref(cv)) >= 8 * 8 * 64 * 4 + 2 * (9 * 4096 + 64) * 4
    assert lib.bts_project_features_bwd_tiles(C.byref(ok_size), 16, 16, None, 16, 1, 16, 16, 1, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_project_features_bwd_tiles(C.byref(cfg), 16, 16, 16, 16, 1, 16, 16, 1, None) == -2 and b"envelope" in lib.bts_last_error()
    assert lib.bts_project_features_tiles(C.byref(ok_size), 16, 16, 1, None, 16, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_project_features_tiles(C.byref(cfg), 16, 16, 1, 16, 16, None) == -2 and b"envelope" in lib.bts_last_error()
    # ABI 8: the channels-last hand-over
    assert lib.bts_project_features_cl(C.byref(ok_size), 16, 16, 1, None, None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_project_features_cl(C.byref(cfg), 16, 16, 1, None, 16, None) == -2 and b"envelope" in lib.bts_last_error()
    assert lib.bts_project_features_bwd_cl(C.byref(ok_size), None, 16, None, 16, 1, 16, 16, 0, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_project_features_bwd_cl(C.byref(bad), 16, 16, None, 16, 1, 16, 16, 0, None) == -1 and b"feat_shift" in lib.bts_last_error()
    margs = _lib.BtsRenderArgs(rays_per_sample=8, K=4, rays=1)                      # neither z_samp nor jitter
    assert lib.bts_mark_sampled_tiles(C.byref(ok_size), 16, 16, C.byref(margs), 16, None) == -1 and b"jitter" in lib.bts_last_error()
    assert lib.bts_mark_sampled_tiles(C.byref(bad), 16, 16, C.byref(_lib.BtsRenderArgs(rays_per_sample=8, K=4, rays=1, z_samp=1)), 16, None) == -1
    assert b"feat_shift" in lib.bts_last_error()
    with pytest.raises(bts.BtsNativeError):
        native.nchw_to_nhwc(torch.zeros(1, 4, 2, 2))                                # CPU tensor: no CPU path
    with pytest.raises(bts.BtsNativeError):
        native.check_supported(native.FieldSpec(C=48, d_hidden=64, n_blocks=0))


def test_host_mirror_keeps_reference_interface():
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=False, code_mode="z",
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64),
                mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    net = bts.BTSNet(conf)
    r = bts.NeRFRenderer.from_conf(dict(n_coarse=64, n_fine=0, lindisp=True, hard_alpha_cap=True, eval_batch_size=100000, sched=[]))
    w = r.bind_parallel(net)
    assert w.net is net and w.renderer is r and r.n_coarse == 64 and r.lindisp and not r.using_fine
    keys = set(w.state_dict())
    # checkpoint layout of the reference: renderer.net.* / renderer.renderer.* below the task wrapper
    for k in ("net.code_xyz._freqs", "net.code_xyz._phases", "net.mlp_coarse.lin_in.weight", "net.mlp_coarse.lin_in.bias",
              "net.mlp_coarse.lin_out.weight", "net.mlp_coarse.lin_out.bias", "renderer.iter_idx", "renderer.last_sched"):
        assert k in keys, k
    assert net.mlp_coarse.lin_in.weight.shape == (64, 103) and net.mlp_coarse.packed().numel() == 6721
    assert net._d_in == 103 and net.get_scale() == 0
    with pytest.raises(native.BtsNativeError):
        r.composite(torch.nn.Linear(3, 3), torch.zeros(4, 8), torch.zeros(4, 64), sb=1)
    # patch sampler draws with torch's CPU generator like the reference (ray_sampler.py:134-140)
    ps = bts.PatchRaySampler(ray_batch_size=128, z_near=3.0, z_far=80.0, patch_size=8)
    torch.manual_seed(3)
    a = ps.draw_patches(2, 4, 32, 64)
    torch.manual_seed(3)
    ref = [(torch.randint(0, 4, (2,)), torch.randint(0, 32 - 8, (2,)), torch.randint(0, 64 - 8, (2,))) for _ in range(2)]
    assert torch.equal(a[0], torch.stack([x[0] for x in ref])) and torch.equal(a[2], torch.stack([x[2] for x in ref]))


def test_synthetic_generators_match_oracle():
    """bench.py / tools take their inputs from behindthescenes_amd.synthetic (no oracle import on those paths); the tests and the
    cpu_baseline leg use the oracle's generators.  Same seeds must give the same tensors, or GPU and CPU legs would differ."""
    import torch
    from behindthescenes_amd import synthetic as S
    from behindthescenes_amd.field import BTSNet
    from oracle import bts_oracle as O
    for smooth in (False, True):
        a = S.synthetic_scene(2, 3, 16, 24, 8, seed=11, intrinsics=S.K_KITTIRAW, smooth=smooth)
        b = O.synthetic_scene(2, 3, 16, 24, 8, seed=11, intrinsics=O.K_KITTIRAW, smooth=smooth)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert (S.K_KITTI360, S.K_KITTIRAW, S.K_RE10K) == (O.K_KITTI360, O.K_KITTIRAW, O.K_RE10K)
    for hd, nb in ((64, 0), (32, 1)):
        net = BTSNet(S.field_conf(hd, hd, nb, 16, 24))
        S.init_mlp_(net.mlp_coarse, seed=7)
        ref = O.init_mlp(hd + 39, hd, nb, gen=torch.Generator().manual_seed(7))
        m = net.mlp_coarse
        assert torch.equal(m.lin_in.weight, ref.w_in) and torch.equal(m.lin_out.weight, ref.w_out)
        for blk, (w0, b0, w1, b1) in zip(m.blocks, ref.blocks):
            assert torch.equal(blk.fc_0.weight, w0) and torch.equal(blk.fc_1.weight, w1)


def test_pk_opsel_lint_catches_the_erratum_form(tmp_path):
    """The build refuses assembly with the packed-FP32 form MI355X evaluates wrongly next to a wide MFMA (low result <- src1's HIGH
    register, tools/check_pk_opsel.py / tools/ubench/pk_opsel_lanes.hip) and stays quiet on the forms measured safe."""
    bad = tmp_path / "bad.s"
    bad.write_text("_Zk:\n\tv_pk_mul_f32 v[2:3], v[8:9], v[28:29] op_sel:[0,1]\n\tv_pk_fma_f32 v[2:3], v[8:9], v[28:29], v[2:3] op_sel:[1,1,0] op_sel_hi:[0,1,1]\n"
                   "\tv_pk_add_f32 v[6:7], v[6:7], v[6:7] op_sel:[1,1] op_sel_hi:[0,1]\n")
    ok = tmp_path / "ok.s"
    ok.write_text("_Zk:\n\tv_pk_mul_f32 v[2:3], v[8:9], v[28:29] op_sel:[1,0]\n\tv_pk_fma_f32 v[2:3], v[8:9], v[28:29], v[2:3] op_sel_hi:[1,0,1]\n"
                  "\tv_pk_fma_f32 v[2:3], v[8:9], v[28:29], v[2:3] op_sel:[0,0,1]\n\tv_pk_mov_b32 v[2:3], v[8:9], v[28:29] op_sel:[0,1]\n"
                  "\tv_pk_add_f32 v[6:7], v[6:7], v[10:11]\n")
    tool = os.path.join(ROOT, "tools", "check_pk_opsel.py")
    r_bad = subprocess.run([sys.executable, tool, str(bad)], capture_output=True, text=True)
    r_ok = subprocess.run([sys.executable, tool, str(ok)], capture_output=True, text=True)
    assert r_bad.returncode == 1 and "3 packed-FP32" in r_bad.stdout, r_bad.stdout
    assert r_ok.returncode == 0 and "0 packed-FP32" in r_ok.stdout, r_ok.stdout


def test_shipped_build_flags_disable_the_slp_vectoriser():
    from behindthescenes_amd import build
    assert "-fno-slp-vectorize" in build.FLAGS and "-ffp-contract=off" in build.FLAGS


def test_loss_module_keeps_the_reference_interface_and_is_loud_outside_its_envelope():
    """ReconstructionLoss mirrors models/bts/model/loss.py:43-81 (constructor keys, metric names); what the fused pass does not
    cover is rejected at construction, not silently served by something else."""
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_edge_aware_smoothness": 0.001})
    assert (crit.lambda_coarse, crit.lambda_fine, crit.lambda_edge_aware_smoothness, crit.alpha_reg_fraction) == (1, 1, 0.001, 1 / 8)
    assert crit.get_loss_metric_names() == ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg"]
    for conf in ({"criterion": "l2"}, {"criterion": "l1+ssim", "median_thresholding": True},
                 {"criterion": "l1+ssim", "invalid_policy": "weight_guided_diverse"}):
        with pytest.raises(NotImplementedError):
            bts.ReconstructionLoss(conf)
    with pytest.raises(NotImplementedError):
        bts.ReconstructionLoss({"criterion": "l1+ssim"}, use_automasking=True)
    with pytest.raises(ValueError):
        bts.ReconstructionLoss({"criterion": "l1+ssim", "alpha_reg_reduction": "batch"})
    with pytest.raises(bts.BtsNativeError):   # CPU tensors: no fallback
        crit(dict(coarse=[dict(rgb=torch.zeros(1, 1, 8, 8, 1, 3), depth=torch.ones(1, 1, 8, 8), weights=torch.zeros(1, 1, 8, 8, 4),
                               invalid=torch.zeros(1, 1, 8, 8, 4, 1))], fine=[{}], rgb_gt=torch.zeros(1, 1, 8, 8, 3)))


def test_lean_render_dict_with_alpha_regularisers_is_rejected_with_a_clear_message():
    """lean_training_outputs drops alphas / weights from the render dict; the alpha-based regularisers then used to fail
    with a bare KeyError('alphas')."""
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_alpha_reg": 0.1})
    lean = dict(rgb=torch.zeros(1, 1, 8, 8, 1, 3), depth=torch.ones(1, 1, 8, 8), invalid_wsum=torch.zeros(1, 1, 8, 8, 1),
                invalid_any=torch.zeros(1, 1, 8, 8, 1))
    with pytest.raises(KeyError, match="want_alphas"):
        crit(dict(coarse=[lean], fine=[{}], rgb_gt=torch.zeros(1, 1, 8, 8, 3)))


def test_drop_in_emits_the_reference_profiler_ranges():
    """a reference user's torch.profiler trace shows renderer_forward / renderer_composite / model_inference /
    loss_computation (nerf.py:222, 328, models_bts.py:275, loss.py:84); the drop-in wraps the same entry points in the same ranges."""
    import inspect
    from behindthescenes_amd import field, loss, renderer
    for mod, names in ((renderer, ("renderer_forward", "renderer_composite")), (field, ("model_inference",)), (loss, ("loss_computation",))):
        src = inspect.getsource(mod)
        for nme in names:
            assert f'record_function("{nme}")' in src, nme


def test_the_product_library_reads_no_environment_variables():
    """The instruments' switches (BTS_ABLATE, BTS_DBG_PTR) exist only in the probe and diagnostic builds: the shipped library does not
    even import getenv.  (The loader's BTS_RENDER_LIB is Python-side, honoured only with BTS_ALLOW_LIB_OVERRIDE=1 and documented in README.md.)"""
    import shutil
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    lib = os.path.join(ROOT, "behindthescenes_amd", "libbts_render.so")
    out = subprocess.run([nm, "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in out
