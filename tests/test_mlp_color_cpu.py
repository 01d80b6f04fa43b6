"""MLP-predicted colour (``sample_color: false``) on the HIP kernels, host side: the ABI additions (parameter count, error codes and
messages, nothing launched) and the ``native_mlp_color`` switch of BTSNet.  No GPU needed."""
import ctypes as C

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _conf(**kw):
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=True, code_mode="z", sample_color=False,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64),
                mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    conf.update(kw)
    return conf


@pytest.mark.parametrize("C_,hd,nb", [(64, 64, 0), (32, 32, 1), (32, 32, 0)])
def test_param_count_is_the_base_plus_three_rows(lib, C_, hd, nb):
    cfg = native._spec_cfg(native.FieldSpec(C=C_, d_hidden=hd, n_blocks=nb), nv=1)
    base = lib.bts_mlp_param_count(C.byref(cfg))
    assert lib.bts_mlp_color_param_count(C.byref(cfg)) == base + 3 * hd + 3
    assert native.FieldSpec(C=C_, d_hidden=hd, n_blocks=nb, mlp_color=True).mlp_param_count() == base + 3 * hd + 3
    assert lib.bts_mlp_color_param_count(None) == -1


@pytest.mark.parametrize("nb", [0, 1])
def test_packed_four_output_mlp_round_trips(nb):
    from behindthescenes_amd.mlp import ResnetFC
    torch.manual_seed(0)
    m = ResnetFC(32 + 39, d_out=4, n_blocks=nb, d_hidden=32)
    for p in m.parameters():
        torch.nn.init.normal_(p)
    v = m.packed().detach()
    spec = native.FieldSpec(C=32, d_hidden=32, n_blocks=nb, mlp_color=True)
    assert v.numel() == spec.mlp_param_count()
    hd, d_in = 32, 32 + 39
    assert torch.equal(v[:hd * d_in].view(hd, d_in), m.lin_in.weight.detach())
    tail = v[-(4 * hd + 4):]
    assert torch.equal(tail[:4 * hd].view(4, hd), m.lin_out.weight.detach())
    assert torch.equal(tail[4 * hd:], m.lin_out.bias.detach())


def _cfg(nv=1, C_=64, hd=64, nb=0, enc_view=-1):
    cfg = native._spec_cfg(native.FieldSpec(C=C_, d_hidden=hd, n_blocks=nb), n=1, H=8, W=16, nv=nv)
    cfg.enc_render_view = enc_view
    return cfg


def _tensors():
    p = C.c_void_p(16)   # never dereferenced: every call below fails its host-side checks first
    return _lib.BtsFieldTensors(feat_nhwc=None, proj_nhwc=p, K_enc=p, w2c_enc=p, imgs_nhwc4=None, K_r=None, w2c_r=None, empty_feature=p,
                                mlp_params=p)


def _args(K=16, **kw):
    p = C.c_void_p(16)
    base = dict(rays_per_sample=4, K=K, rays=p, z_samp=p, rgb=p, depth=p, sigma_raw=p, trans=p, reserved_=0)
    base.update(kw)
    return _lib.BtsRenderArgs(**base)


def test_host_side_errors_are_codes_with_messages(lib):
    t, a = _tensors(), _args()
    # NULL
    assert lib.bts_render_fwd_mlp_color(None, None, None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_field_query_mlp_color(None, None, None, 0, 0, None, None, None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_render_bwd_mlp_color(C.byref(_cfg()), C.byref(t), C.byref(a), None, None, 0, None) == -1
    assert b"NULL" in lib.bts_last_error()
    # nv != 1
    for nv in (0, 2):
        assert lib.bts_render_fwd_mlp_color(C.byref(_cfg(nv=nv)), C.byref(t), C.byref(a), None) == -1
        assert b"nv=" in lib.bts_last_error()
    assert lib.bts_render_fwd_mlp_color(C.byref(_cfg(enc_view=0)), C.byref(t), C.byref(a), None) == -1
    assert b"enc_render_view" in lib.bts_last_error()
    # unsupported shape
    bad = _cfg(C_=48)
    assert lib.bts_render_fwd_mlp_color(C.byref(bad), C.byref(t), C.byref(a), None) == -2
    assert b"envelope" in lib.bts_last_error()
    assert lib.bts_field_query_mlp_color(C.byref(bad), C.byref(t), C.c_void_p(16), 4, 0, C.c_void_p(16), None, C.c_void_p(16), None) == -2
    # the lean per-ray reductions are not produced in this mode
    lean = _args(invalid_wsum=C.c_void_p(16))
    assert lib.bts_render_fwd_mlp_color(C.byref(_cfg()), C.byref(t), C.byref(lean), None) == -2
    assert b"invalid_wsum" in lib.bts_last_error()
    # short workspace
    g = _lib.BtsRenderGrads()
    need = lib.bts_render_bwd_mlp_color_workspace(C.byref(_cfg()), C.byref(a))
    assert need >= 4 * 16 * 4 * 65
    assert lib.bts_render_bwd_mlp_color(C.byref(_cfg()), C.byref(t), C.byref(a), C.byref(g), C.c_void_p(16), need - 1, None) == -4
    assert b"workspace" in lib.bts_last_error()


def test_config_key_switches_torch_mode():
    plain = bts.BTSNet(_conf())
    assert plain.torch_mode and not plain.spec.mlp_color
    native_net = bts.BTSNet(_conf(native_mlp_color=True))
    assert not native_net.torch_mode and native_net.spec.mlp_color and native_net._d_out == 4
    assert native_net.spec.mlp_param_count() == native_net.mlp_coarse.packed().numel()
    # sampled colours ignore the key
    assert not bts.BTSNet(_conf(sample_color=True, native_mlp_color=True)).spec.mlp_color


def test_fused_paths_refuse_a_native_mlp_color_net():
    """The one-call training step and evaluation frame serve sampled colours only; with native_mlp_color their why_not() says so."""
    net = bts.BTSNet(_conf(native_mlp_color=True)).train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=64, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).train()
    sampler = bts.PatchRaySampler(ray_batch_size=256, z_near=3.0, z_far=80.0, patch_size=8)
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_edge_aware_smoothness": 0.001})
    step = bts.FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit)
    assert "sample_color=False" in step.why_not(None, ids_encoder=[0], ids_render=[2, 3], ids_loss=[0, 1])
    net.eval(), renderer.eval()
    frame = bts.FusedEvalFrame(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16))
    assert "sample_color=False" in frame.why_not(None, ids_encoder=[0], ids_render=[0])
