"""GPU: the evaluation frame's hand-over launch (eval_handover_kernel inside bts_eval_frame_gt): cameras, inverse intrinsics, rgb0 packing,
rays and rgb_gt as work-group ranges of ONE dispatch.  Every role against the single entry point that wrote the same bytes before, bit for
bit; the fused frame against the entry-by-entry frame; the NULL rgb_gt form; the number of dispatches of a frame.

Shapes: n = 2, v = 3 at 12 x 20 (1 440 pixels: several 256-thread work-groups per role and a ragged last one; 3 * 1 440 floats of rgb_gt are
whole float4s) and at 11 x 19 (1 254 pixels; 3 * 1 254 = 3 762 floats are not: the ragged end of the float4 role)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMETRIES = [(12, 20), (11, 19)]
N, V = 2, 3
GUARD, SENTINEL = 256, -7.25          # floats behind the end of every buffer; a value no role writes
Z_NEAR, Z_FAR = 3.0, 80.0


def _net(H, W, K):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    dev = torch.device("cuda")
    scene = S.synthetic_scene(N, V, H, W, 64, seed=9, intrinsics=S.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=N)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to(dev).eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to(dev)
    inputs = [scene[k].to(dev).float().contiguous() for k in ("images", "projs", "poses")]
    return net, wrapped, inputs


def _guarded(numel, dev):
    return torch.full((numel + GUARD,), SENTINEL, device=dev, dtype=torch.float32)


def _guard_ok(buf, numel):
    return bool((buf[numel:] == SENTINEL).all())


def _struct(net, inputs, ids_render, norm_dir, K, to_z=True):
    """A BtsEvalFrame over guarded buffers of this test's own (FusedEvalFrame.forward's fill, with id_encoder = 0) -> (fr, buffers, sizes)."""
    from behindthescenes_amd import _lib, native
    images, projs, poses = inputs
    n, v, _, H, W = images.shape
    dev, nv, B = images.device, len(ids_render), n * v * H * W
    sizes = dict(cams=n * (25 + nv * 25), imgs_nhwc4=n * nv * H * W * 4, proj_nhwc=n * H * W * net.spec.d_hidden, inv_K=n * v * 9, rays=B * 8, rgb=B * nv * 3,
                 depth=B, depth_z=B, weights=B * K, alphas=B * K, invalid=B * K * nv, rgb_gt=B * 3)
    buf = {k: _guarded(s, dev) for k, s in sizes.items()}
    torch.manual_seed(11)
    keep = dict(feat=net.encoder(images[:, 0])[0].detach(), params=net.mlp_coarse.packed().detach(), jitter=torch.rand((B, K), device=dev))
    fr = _lib.BtsEvalFrame()
    fr.cfg = native._spec_cfg(net.spec, n, H, W, nv, 0, ids_render.index(0) if 0 in ids_render else -1)
    fr.v, fr.id_encoder = v, 0
    for j, i in enumerate(ids_render):
        fr.ids_render[j] = i
    fr.K, fr.lindisp, fr.hard_alpha_cap, fr.norm_dir = K, 1, 1, int(norm_dir)
    fr.z_near, fr.z_far, fr.img_scale, fr.img_shift = Z_NEAR, Z_FAR, 0.5, 0.5
    fr.feat_channels_last = 0
    fr.images, fr.Ks, fr.poses_c2w = images.data_ptr(), projs.data_ptr(), poses.data_ptr()
    fr.feat_nchw, fr.mlp_params, fr.jitter = keep["feat"].data_ptr(), keep["params"].data_ptr(), keep["jitter"].data_ptr()
    for k in sizes:
        if k != "rgb_gt" and (to_z or k != "depth_z"):
            setattr(fr, k, buf[k].data_ptr())
    return fr, buf, sizes, keep


@pytest.mark.parametrize("norm_dir", [0, 1])
@pytest.mark.parametrize("ids_render", [[2, 0], [1, 2]], ids=["enc_is_slot1", "enc_not_rendered"])
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_roles_equal_the_single_entry_points(H, W, ids_render, norm_dir):
    from behindthescenes_amd import native
    net, _, inputs = _net(H, W, 64)
    images, projs, poses = inputs
    nv = len(ids_render)
    fr, buf, sizes, keep = _struct(net, inputs, ids_render, norm_dir, 64)
    gt = buf["rgb_gt"][:sizes["rgb_gt"]].view(N, V, 3, H, W)
    native.eval_frame(fr, native._stream(images), rgb_gt=gt)
    torch.cuda.synchronize()
    cams = buf["cams"][:sizes["cams"]]
    K_enc, w2c_enc, K_r, w2c_r = cams.split([N * 9, N * 16, N * nv * 9, N * nv * 16])
    assert torch.equal(K_enc.view(N, 3, 3), projs[:, 0]) and torch.equal(K_r.view(N, nv, 3, 3), projs[:, ids_render])
    assert torch.equal(w2c_enc.view(N, 4, 4), native.invert_small(poses[:, 0]))
    assert torch.equal(w2c_r.view(N, nv, 4, 4), native.invert_small(poses[:, ids_render]))
    assert torch.equal(buf["inv_K"][:sizes["inv_K"]].view(N, V, 3, 3), native.invert_small(projs))
    assert torch.equal(buf["imgs_nhwc4"][:sizes["imgs_nhwc4"]].view(N, nv, H, W, 4), native.pack_rgb(images[:, ids_render].contiguous(), 0.5, 0.5))
    rays = native.gen_rays(poses.view(N * V, 4, 4), projs.view(N * V, 3, 3), H, W, Z_NEAR, Z_FAR, bool(norm_dir))
    assert torch.equal(buf["rays"][:sizes["rays"]].view(N * V, H, W, 8), rays)
    assert torch.equal(gt, images * .5 + .5)
    for k, s in sizes.items():
        assert _guard_ok(buf[k], s), f"{k}: written behind its end"
    del keep


@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_null_rgb_gt_skips_the_role_and_changes_nothing_else(H, W):
    from behindthescenes_amd import native
    net, _, inputs = _net(H, W, 64)
    fr, buf, sizes, keep = _struct(net, inputs, [2, 0], 1, 64)
    native.eval_frame(fr, native._stream(inputs[0]))
    torch.cuda.synchronize()
    assert bool((buf["rgb_gt"] == SENTINEL).all())
    fr2, buf2, _, keep2 = _struct(net, inputs, [2, 0], 1, 64)
    native.eval_frame(fr2, native._stream(inputs[0]), rgb_gt=buf2["rgb_gt"][:sizes["rgb_gt"]].view(N, V, 3, H, W))
    torch.cuda.synchronize()
    for k in sizes:
        if k != "rgb_gt":
            assert torch.equal(buf[k], buf2[k]), k
    del keep, keep2


@pytest.mark.parametrize("to_z", [True, False])
@pytest.mark.parametrize("ids_render", [[0], [1, 2]], ids=["nv1", "nv2"])
@pytest.mark.parametrize("K", [64, 16])
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_fused_frame_equals_the_entry_by_entry_frame(H, W, K, ids_render, to_z):
    import behindthescenes_amd as bts
    net, wrapped, inputs = _net(H, W, K)
    outs = []
    for fused in (False, True):
        frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(Z_NEAR, Z_FAR), fused=fused)
        if fused and not to_z:      # the scratch of this shape exists after one frame: a second one must leave its inv_K alone
            frame(*inputs, ids_encoder=[0], ids_render=ids_render, to_z=False)
            for sc in frame._scratch.values():
                sc["inv_K"].fill_(SENTINEL)
        torch.manual_seed(21)
        outs.append(frame(*inputs, ids_encoder=[0], ids_render=ids_render, to_z=to_z))
        assert frame.last_path == ("fused" if fused else "entries: switched off (fused=False)")
    torch.cuda.synchronize()
    if not to_z:
        assert frame._scratch and all(bool((sc["inv_K"] == SENTINEL).all()) for sc in frame._scratch.values())
    a, b = outs
    assert set(a) == set(b) == {"coarse", "fine", "rgb_gt", "rays"}
    assert a["rays"].shape == b["rays"].shape and torch.equal(a["rays"], b["rays"])
    assert a["rgb_gt"].shape == b["rgb_gt"].shape and torch.equal(a["rgb_gt"], b["rgb_gt"])
    for part in ("coarse", "fine"):
        assert set(a[part][0]) == set(b[part][0])
        for k in a[part][0]:
            assert a[part][0][k].shape == b[part][0][k].shape, (part, k)
            assert torch.equal(a[part][0][k], b[part][0][k]), (part, k)


@pytest.mark.parametrize("to_z", [True, False])
def test_a_fused_frame_is_four_library_dispatches(to_z):
    """One fused frame under torch.profiler after a warm-up frame: hand-over, projection, render [, distance_to_z] and none of the kernels
    the hand-over replaced; of torch's own kernels the jitter draw and at most one more (the torch.cat of the MLP's parameters behind
    invalidate_packed())."""
    import behindthescenes_amd as bts
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    net, wrapped, inputs = _net(12, 20, 64)
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(Z_NEAR, Z_FAR))
    frame(*inputs, ids_encoder=[0], ids_render=[0], to_z=to_z)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        frame(*inputs, ids_encoder=[0], ids_render=[0], to_z=to_z)
        torch.cuda.synchronize()
    assert frame.last_path == "fused"
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset"))]
    ours = [k for k in names if "bts::" in k or "_ZN3bts" in k]      # (demangled, or mangled where the tracer does not demangle)
    other = [k for k in names if k not in ours]
    print("bts kernels:", [k[:60] for k in ours], "\nother kernels:", [k[:90] for k in other])
    assert len(ours) == (4 if to_z else 3), ours
    assert sum("eval_handover_kernel" in k for k in ours) == 1 and sum("distance_to_z_kernel" in k for k in ours) == int(to_z)
    for gone in ("camera_prep_kernel", "pack_rgb_kernel", "gen_rays_kernel", "invert_small_kernel"):
        assert not any(gone in k for k in names), gone
    assert 1 <= len(other) <= 2, other
