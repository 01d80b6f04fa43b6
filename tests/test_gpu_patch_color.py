"""Patch colours (``image_processor: {type: patch}``: 27 channels per render view) on the HIP kernels -- ``native_patch_color: true``,
csrc/bts_patch_color.hip behind the unchanged render, csrc/bts_loss_pixel_c.hip for the l1 / l2 criteria on 27 channels -- against the REAL
reference (tests/golden/patch_color.npz, tests/golden/gen_golden_patch_color.py: fp32 and fp64), against the 3-channel render of the same
net, and against the CPU oracle of tests/_patch_color_oracle.py in fp64 at the shapes where the kernels take another path."""
import types

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import native
from oracle import bts_oracle as O
from tests import _patch_color_oracle as PC
from tests._hip_helpers import make_conf
from tests._multi_view_fixture import walsh_rows
from tests.test_patch_color_cpu import LOSSES, load

pytestmark = pytest.mark.gpu


def _near(got, ref32, ref64, atol, name):
    """within atol of the fp32 reference, or -- where the reference's own fp32 rounding exceeds that -- no further from the fp64 reference than
    the fp32 reference is (x 1.5 + atol), in max-norm: the rule of tests/test_gpu_multi_view.py"""
    got, ref32, ref64 = (x.detach().cpu().double() for x in (got, ref32, ref64))
    e, e_n, e_t = (got - ref32).abs().max().item(), (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    print(f"  {name}: max err vs reference {e:.2e}; vs fp64 {e_n:.2e} (fp32 reference {e_t:.2e})")
    assert e <= atol or e_n <= 1.5 * e_t + atol, name


def _grad(a, b, c, what):
    """within 1e-4 of the largest entry, or no further from fp64 than the fp32 reference is (x 1.5 + 2e-5) in max-norm and L2"""
    a, b, c = (x.detach().cpu().double() for x in (a, b, c))
    scale, err = b.abs().max().item(), (a - b).abs().max().item()
    e_n, e_t, l_n, l_t = (a - c).abs().max().item(), (b - c).abs().max().item(), (a - c).norm().item(), (b - c).norm().item()
    print(f"  d{what}: max err {err:.2e} of max |g| {scale:.2e}; vs fp64 {e_n:.2e} / L2 {l_n:.2e} (reference {e_t:.2e} / {l_t:.2e})")
    assert err <= 1e-4 * scale or (e_n <= 1.5 * e_t + 2e-5 and l_n <= 1.5 * l_t + 2e-5), what


def _net(t, meta, patch=True, train=False):
    cfg = O.FieldConfig(code_mode=meta["code_mode"], learn_empty=meta["learn_empty"], empty_empty=meta["empty_empty"])
    conf = dict(make_conf(cfg, meta["C"], meta["Hd"], meta["n_blocks"], meta["H"], meta["W"]), native_patch_color=True)
    conf["encoder"] = dict(conf["encoder"], num_views=meta["n"])
    net = bts.BTSNet(conf)
    with torch.no_grad():
        net.encoder.feats[0].data = t["feats"].float().clone()
        for k, p in net.mlp_coarse.named_parameters():
            p.copy_(t["p_" + k.replace(".", "_")])
        if meta["learn_empty"]:
            net.empty_feature.copy_(t["empty"])
    net = net.cuda().train(train)
    images = t["images"].float().cuda()
    net.encode(images, t["projs"].cuda(), t["poses"].cuda(), ids_encoder=meta["ids_encoder"], ids_render=meta["ids_render"],
               images_alt=bts.PatchProcessor(3)(images) if patch else None)
    return net


def _renderer(meta, **kw):
    return bts.NeRFRenderer(n_coarse=meta["K"], lindisp=True, hard_alpha_cap=meta["hard_alpha_cap"], white_bkgd=meta["white_bkgd"], **kw).cuda().eval()


# ---- against the reference fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_render_and_gradients_vs_reference_golden(name):
    t, meta = load(name)
    net = _net(t, meta)
    n, nv, C = meta["n"], len(meta["ids_render"]), meta["C"]
    assert net._patch == 3 and net.grid_c_imgs.shape[2] == 27
    r = _renderer(meta)
    w, rgb, depth, _, inv, _, rgbs = r.composite(net, t["rays"].reshape(-1, 8).cuda(), t["z"].cuda(), coarse=True, sb=n)
    assert rgb.shape == t["rgb"].shape == (n * meta["B"], nv * 27) and rgbs.shape == (n * meta["B"], meta["K"], nv * 27)
    assert torch.equal(inv.cpu(), t["invalid"]), "every flag, nothing set aside"
    rel = ((depth.detach().cpu() - t["depth"]).abs() / t["depth"].abs().clamp_min(1e-6)).max().item()
    print(f"render {name}: depth max rel err {rel:.2e}")
    assert rel <= 1e-4
    _near(rgb, t["rgb"], t["f64_rgb"], 1e-5, "rgb")
    _near(w, t["weights"], t["f64_weights"], 1e-5, "weights")
    _near(rgbs[t["pick"].cuda()], t["rgb_samps"], t["f64_rgb_samps"], 1e-5, "rgb_samps")
    assert not rgbs.requires_grad
    params = list(net.mlp_coarse.parameters()) + [net.encoder.feats[0]] + ([net.empty_feature] if meta["learn_empty"] else [])
    names = [k for k, _ in net.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if meta["learn_empty"] else [])
    grads = torch.autograd.grad((rgb * t["gin_rgb"].cuda()).sum() + (depth * t["gin_depth"].cuda()).sum(), params)
    for k, a in zip(names, grads):
        key = "g_" + k.replace(".", "_")
        if k == "feats":      # as the fixture stores it: its product with C / 4 Walsh functions of the channel index
            a = torch.einsum("rc,mchw->mrhw", walsh_rows(C), a.detach().cpu().double())
        _grad(a, t[key], t["f64_" + key], k)
    # the field query's colours are the per-sample colours at the same points, its flags the render's
    rays = t["rays"].reshape(-1, 8).cuda()
    pts = (rays[:, None, :3] + t["z"].cuda().unsqueeze(2) * rays[:, None, 3:6]).reshape(n, -1, 3).contiguous()
    with torch.no_grad():
        q_rgb, q_inv, _ = net(pts)
        q_none, q_inv1, _ = net(pts, only_density=True)
    assert q_rgb.shape == (n, pts.shape[1], nv * 27) and torch.equal(q_rgb.reshape(rgbs.shape), rgbs)
    assert torch.equal(q_inv.reshape(inv.shape), inv) and q_none.shape == (n, pts.shape[1], nv * 3) and not bool(q_none.any())


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("crit,policy", LOSSES)
def test_channel_loss_vs_reference_golden(name, crit, policy):
    t, meta = load(name)
    n, nv, K, sel = meta["n"], len(meta["ids_render"]), meta["K"], t["sel"]
    x = t["rgb"][sel].reshape(n, 1, 8, 8, nv, 27).cuda().requires_grad_(True)
    level = dict(rgb=x, depth=t["depth"][sel].reshape(n, 1, 8, 8).cuda(), weights=t["weights"][sel].reshape(n, 1, 8, 8, K).cuda(),
                 invalid=t["invalid"][sel].reshape(n, 1, 8, 8, K, nv).cuda())
    crit_ = bts.ReconstructionLoss(dict(criterion=crit, invalid_policy=policy, native_pixel_loss=True))
    loss, ld = crit_(dict(coarse=[level], fine=[dict(level)], rgb_gt=t["loss_gt"].cuda()))
    g, = torch.autograd.grad(loss, x)
    ref, ref_g = t[f"loss_{crit}_{policy}"], t[f"lossg_{crit}_{policy}"]
    e_l, e_g = abs(loss.item() - ref[0].item()), (g.reshape(ref_g.shape).cpu() - ref_g).abs().max().item()
    print(f"loss {name} {crit} {policy}: {loss.item():.6f} vs {ref[0].item():.6f} (err {e_l:.2e}); gradient err {e_g:.2e} of {ref_g.abs().max().item():.2e}")
    assert e_l <= 1e-5 and e_g <= 1e-4 * ref_g.abs().max().item()
    assert abs(ld["loss_invalid_ratio"] - ref[1].item()) <= 1e-6 and set(ld) == set(bts.ReconstructionLoss._KEYS)
    assert abs(ld["loss"] - loss.item()) <= 1e-6 and abs(ld["loss_rgb_coarse"] + ld["loss_rgb_fine"] - loss.item()) <= 1e-6


@pytest.mark.parametrize("name", ["a", "b"])
def test_training_step_entry_by_entry_vs_reference_golden(name):
    """PatchProcessor -> encode -> RandomRaySampler(channels=27) on injected rays -> renderer -> l2 -> backward"""
    t, meta = load(name)
    n, nv, K, sel = meta["n"], len(meta["ids_render"]), meta["K"], t["sel"]
    net = _net(t, meta)
    for p in net.parameters():
        p.grad = None
    r = _renderer(meta)
    r.sample_coarse = lambda rays, u=None: t["z"][sel].cuda()        # (the reference's extension point: the fixture's depths)
    sampler = bts.RandomRaySampler(64, 3.0, 80.0, channels=27)
    rays = t["rays"].reshape(-1, 8)[sel].reshape(n, 64, 8).cuda()
    rd = r.bind_parallel(net)(rays, want_weights=True, want_alphas=True, want_rgb_samps=True)
    rd["fine"] = dict(rd["coarse"])
    rd["rgb_gt"] = t["loss_gt"].reshape(n, 64, 27).cuda()
    rd = sampler.reconstruct(rd)
    assert rd["coarse"]["rgb"].shape == (n, 64, nv, 27) and rd["coarse"]["rgb_samps"].shape == (n, 64, K, nv, 27)
    # the loss takes the patch layout (n, patches, h, w, ...): a random ray is a 1 x 1 patch
    as_patches = lambda d: {k: x.unflatten(1, (64, 1, 1)) for k, x in d.items()}
    data = dict(coarse=[as_patches(rd["coarse"])], fine=[as_patches(rd["fine"])], rgb_gt=rd["rgb_gt"].unflatten(1, (64, 1, 1)))
    loss, _ = bts.ReconstructionLoss(dict(criterion="l2", invalid_policy="weight_guided", native_pixel_loss=True))(data)
    loss.backward()
    e = abs(loss.item() - t["step_loss"].item())
    print(f"step {name}: loss {loss.item():.6f} vs {t['step_loss'].item():.6f}")
    assert e <= 1e-5
    for k, p in list(net.mlp_coarse.named_parameters()) + ([("empty", net.empty_feature)] if meta["learn_empty"] else []):
        key = "step_g_" + k.replace(".", "_")
        _grad(p.grad, t[key], t["f64_" + key], k)
    assert net.encoder.feats[0].grad is not None and bool(net.encoder.feats[0].grad.abs().sum() > 0)


# ---- against the 3-channel render ---------------------------------------------------------------------------------------------------------------
def _pair(shape, size, n, v, ids_render, seed, n_scales=1, **extra):
    """(net with patch colours, the same net rendering three channels, scene)"""
    (C, Hd, nb), (H, W) = shape, size
    conf = dict(make_conf(O.FieldConfig(learn_empty=True), C, Hd, nb, H, W), native_patch_color=True, **extra)
    conf["encoder"] = dict(conf["encoder"], num_views=n, n_scales=n_scales, pyramid=n_scales > 1)
    scene = O.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    nets = [bts.BTSNet(conf), bts.BTSNet(conf)]
    with torch.no_grad():
        for mlp in (nets[0].mlp_coarse, nets[0].mlp_fine):
            for p in (mlp.parameters() if mlp is not None else ()):
                p.copy_(torch.randn(p.shape, generator=g) * (0.15 if p.dim() > 1 else 0.05))
        for f in nets[0].encoder.feats:
            f.copy_(torch.nn.functional.avg_pool2d(torch.randn(f.shape, generator=g), 5, 1, 2) * 3)
        nets[0].empty_feature.copy_(torch.randn(C, generator=g))
    nets[1].load_state_dict(nets[0].state_dict())
    images = scene["images"].cuda()
    for net, alt in ((nets[0], bts.PatchProcessor(3)(images)), (nets[1], None)):
        net.cuda().eval()
        net.encode(images, scene["projs"].cuda(), scene["poses"].cuda(), ids_encoder=[0], ids_render=ids_render, images_alt=alt)
    return nets[0], nets[1], scene


def _rays(scene, H, W, count, seed):
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, 3.0, 80.0)
    n = rays.shape[0]
    rays = rays.reshape(n, -1, 8)
    pick = torch.randperm(rays.shape[1], generator=torch.Generator().manual_seed(seed))[:count].sort().values
    return rays[:, pick].reshape(-1, 8).contiguous().cuda()


def _oracle_of(net, rays, z, weights, white, dt=torch.float64):
    """the CPU oracle on what the net's last encode left: -> rgb_samps, rgb"""
    imgs = net.grid_c_imgs[:, :, 12:15].detach().cpu().to(dt)
    w2c, Ks = net.grid_c_poses_w2c.detach().cpu().to(dt), net.grid_c_Ks.detach().cpu().to(dt)
    samps = PC.sample_colours(imgs, w2c, Ks, rays.detach().cpu().to(dt), z.detach().cpu().to(dt))
    return samps, PC.composite(weights.detach().cpu().to(dt), samps, white)


def test_centre_triple_is_the_3_channel_render():
    H, W, n, K = 16, 32, 2, 24
    patch, plain, scene = _pair((64, 64, 0), (H, W), n, 4, [1, 3], seed=11)
    rays = _rays(scene, H, W, 75, 1)
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    z = r.sample_coarse(rays)
    with torch.no_grad():
        a = r.composite(patch, rays, z, coarse=True, sb=n)
        b = r.composite(plain, rays, z, coarse=True, sb=n)
    assert a[1].shape == (n * 75, 2 * 27) and b[1].shape == (n * 75, 6)
    centre = a[1].reshape(-1, 2, 27)[..., 12:15].reshape(-1, 6)
    assert (centre - b[1]).abs().max().item() <= 1e-5
    assert (a[6].reshape(-1, K, 2, 27)[..., 12:15].reshape(-1, K, 6) - b[6]).abs().max().item() <= 1e-5
    for i in (0, 2, 3, 4):      # weights, depth, alphas, invalid: the render itself is untouched
        assert torch.equal(a[i], b[i]), i


# ---- the kernels against the oracle in fp64 --------------------------------------------------------------------------------------------------------
def _raw_case(H, W, nv, K, Bp, seed, n=2):
    """random frames, cameras of a synthetic scene, rays of view 0, sorted random depths, random weights; in batch element 1 the last view
    looks the other way: every ray misses it"""
    g = torch.Generator().manual_seed(seed)
    scene = O.synthetic_scene(n, nv + 1, H, W, 4, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    imgs = torch.nn.functional.avg_pool2d(torch.rand(n * nv, 3, H, W, generator=g), 3, 1, 1, count_include_pad=False).reshape(n, nv, 3, H, W)
    poses = scene["poses"][:, 1:].clone()
    poses[1, nv - 1, :3, :3] = poses[1, nv - 1, :3, :3] @ torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    w2c, Ks = torch.inverse(poses), scene["projs"][:, 1:].contiguous()
    rays = O.image_rays(scene["poses"][:, :1], scene["projs"][:, :1], H, W, 3.0, 80.0).reshape(n, -1, 8)
    rays = rays[:, torch.randint(0, rays.shape[1], (Bp,), generator=g)].reshape(-1, 8).contiguous()
    z = (3.0 + 60.0 * torch.rand(n * Bp, K, generator=g) ** 2).sort(-1).values
    weights = torch.rand(n * Bp, K, generator=g) / K
    ft = types.SimpleNamespace(n=n, nv=nv, H=H, W=W, imgs_nhwc4=native.pack_rgb(imgs.cuda()), K_r=Ks.cuda(), w2c_r=w2c.contiguous().cuda())
    return ft, imgs, w2c, Ks, rays, z, weights, g


RAW = [(5, 7, 3, 16, 37, False), (5, 7, 1, 1, 300, True), (5, 7, 3, 200, 3, True), (16, 32, 3, 48, 37, True), (16, 32, 1, 200, 5, False),
       (16, 32, 3, 1, 37, False), (16, 32, 1, 16, 37, True), (5, 7, 1, 48, 11, False), (16, 32, 3, 300, 2, True)]


@pytest.mark.parametrize("H,W,nv,K,Bp,white", RAW)
def test_kernels_vs_oracle_fp64(H, W, nv, K, Bp, white):
    ft, imgs, w2c, Ks, rays, z, weights, g = _raw_case(H, W, nv, K, Bp, seed=100 + K + nv)
    d = torch.float64
    s64 = PC.sample_colours(imgs.to(d), w2c.to(d), Ks.to(d), rays.to(d), z.to(d))
    s32 = PC.sample_colours(imgs, w2c, Ks, rays, z)
    # in batch element 1 every sample misses the last view: all that is read there is a border texel's patch
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(ft.n, -1, 3)
    assert bool(O.project(pts.to(d), w2c.to(d), Ks.to(d))[3][1, nv - 1].all())
    cr, cz, cw = rays.cuda(), z.cuda(), weights.cuda()
    rgb, samps = native.patch_color_fwd(ft, cr, cz, cw, white_bkgd=white, want_rgb_samps=True)
    rgb2, none = native.patch_color_fwd(ft, cr, cz, cw, white_bkgd=white)
    assert none is None and torch.equal(rgb, rgb2)
    _near(samps, s32, s64, 1e-5, "rgb_samps")
    _near(rgb, PC.composite(weights, s32, white), PC.composite(weights.to(d), s64, white), 1e-5, "rgb")
    # g_weights alone
    g_rgb = torch.randn(rgb.shape, generator=g)
    gw = native.patch_color_bwd(ft, cr, cz, g_rgb.cuda(), white_bkgd=white)
    gw64, gw32 = PC.g_weights(g_rgb.to(d), s64, white), PC.g_weights(g_rgb, s32, white)
    err, scale = (gw.cpu().double() - gw64).abs().max().item(), gw64.abs().max().item()
    print(f"  g_weights: max err {err:.2e} of max |g| {scale:.2e} (fp32 oracle {(gw32.double() - gw64).abs().max().item():.2e})")
    assert gw.shape == (ft.n * Bp, K) and (err <= 1e-4 * scale or err <= 1.5 * (gw32.double() - gw64).abs().max().item() + 2e-5)
    assert torch.equal(gw, native.patch_color_bwd(ft, cr, cz, g_rgb.cuda(), white_bkgd=white))
    # the query entry: the same colours at the same points (o + z d, multiply then add, as the kernels form it)
    cp = (cr[:, None, :3] + cz.unsqueeze(2) * cr[:, None, 3:6]).reshape(ft.n, -1, 3).contiguous()
    assert torch.equal(native.patch_color_query(ft, cp).reshape(samps.shape), samps)


def test_other_patch_sizes_are_refused_by_name():
    ft, *_ = _raw_case(5, 7, 1, 1, 4, seed=1)
    with pytest.raises(bts.BtsNativeError, match="BTS_E_UNSUPPORTED.*patch=5, but the compiled patch size is 3"):
        native.patch_color_query(ft, torch.zeros(2, 4, 3).cuda(), patch=5)


# ---- the renderer around them ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_jitter_form_agrees():
    t, meta = load("a")
    net = _net(t, meta)
    r = _renderer(meta)
    rays, u = t["rays"].reshape(-1, 8).cuda(), t["u"].float().cuda()
    runs = []
    for _ in range(2):
        w, rgb, depth, _, _, _, rgbs = r.composite(net, rays, t["z"].cuda(), coarse=True, sb=meta["n"])
        # (the gradient in the render's weights: what the colour kernels hand to bts_render_bwd, whose own passes add with float atomics)
        g_w, = torch.autograd.grad((rgb * t["gin_rgb"].cuda()).sum(), w, retain_graph=True)
        runs.append([w, rgb, depth, rgbs, g_w])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():     # sample_coarse inside the render kernel: the depths come back for the colour kernels
        c = r._composite(net, rays, None, True, meta["n"], False, False, True, True, False, jitter=u)
        e = r.composite(net, rays, native.sample_coarse(rays, u, True), coarse=True, sb=meta["n"])
    assert torch.equal(c[1], e[1]) and torch.equal(c[6], e[6]) and c[0] is None


def test_lean_outputs_and_the_sparse_projection_name_patch_colours():
    t, meta = load("a")
    net = _net(t, meta, train=True)
    r = bts.NeRFRenderer(n_coarse=meta["K"], lindisp=True, hard_alpha_cap=True, lean_training_outputs=True).cuda().train()
    rays = t["rays"].reshape(meta["n"], -1, 8).cuda()
    with pytest.raises(bts.BtsNativeError, match="patch colours"):
        r(net, rays)
    flat = rays.reshape(-1, 8)
    with pytest.raises(bts.BtsNativeError, match="lean_training_outputs returns no weights.*patch colours"):
        r._composite(net, flat, t["z"].cuda(), True, meta["n"], False, False, True, False, True)
    with pytest.raises(bts.BtsNativeError, match="sparse one-shot projection.*patch colours"):
        net.native_field(sampled=(flat, t["z"].cuda(), None, True))


def test_two_pass_render_colours_follow_the_returned_samples():
    H, W, n = 16, 32, 2
    patch, _, scene = _pair((32, 32, 1), (H, W), n, 4, [2, 3], seed=12)
    rays = _rays(scene, H, W, 40, 2)
    r = bts.NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, lindisp=True, white_bkgd=True, native_fine_sampling=True).cuda().eval()
    with torch.no_grad():
        out = r(patch, rays.reshape(n, -1, 8), want_weights=True, want_z_samps=True, want_rgb_samps=True)
    for part, K in (("coarse", 16), ("fine", 24)):
        o = out[part]
        assert o["rgb"].shape == (n, 40, 2 * 27) and o["z_samps"].shape == (n, 40, K) and o["rgb_samps"].shape == (n, 40, K, 2 * 27)
        z, w = o["z_samps"].reshape(-1, K), o["weights"].reshape(-1, K)
        s64, rgb64 = _oracle_of(patch, rays, z, w, True)
        s32, rgb32 = _oracle_of(patch, rays, z, w, True, torch.float32)
        _near(o["rgb_samps"].reshape(s64.shape), s32, s64, 1e-5, part + " rgb_samps")
        _near(o["rgb"].reshape(rgb64.shape), rgb32, rgb64, 1e-5, part + " rgb")


def test_a_coarser_scale_reads_the_same_colours():
    H, W, n, K = 16, 32, 2, 16
    patch, plain, scene = _pair((64, 64, 0), (H, W), n, 4, [1, 2, 3], seed=13, n_scales=2)
    rays = _rays(scene, H, W, 50, 3)
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    z = r.sample_coarse(rays)
    outs = []
    for scale in (0, 1):
        patch.set_scale(scale), plain.set_scale(scale)
        with torch.no_grad():
            a = r.composite(patch, rays, z, coarse=True, sb=n)
            b = r.composite(plain, rays, z, coarse=True, sb=n)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        s64, rgb64 = _oracle_of(patch, rays, z, a[0], False)
        s32, rgb32 = _oracle_of(patch, rays, z, a[0], False, torch.float32)
        _near(a[1], rgb32, rgb64, 1e-5, f"scale {scale} rgb")
        outs.append(a)
    assert torch.equal(outs[0][6], outs[1][6]), "the per-sample colours do not depend on the scale"
    assert not torch.equal(outs[0][0], outs[1][0]), "the two scales are different fields"


# ---- the C-channel loss against bts_pixel_loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("policy", ["none", "strict", "weight_guided"])
def test_three_channels_match_bts_pixel_loss(crit, policy):
    g = torch.Generator().manual_seed(7)
    B, nv, K = 2 * 3 * 64 + 0, 3, 8
    rgb = torch.rand(B, nv * 3, generator=g).cuda()
    rgb[:40, 3:6] = rgb[:40, 0:3]                      # ties between two views
    gt = torch.rand(B, 3, generator=g).cuda()
    gt[40:60] = rgb[40:60, 6:9]                        # exact zeros: sign(0) = 0
    weights = (torch.rand(B, K, generator=g) / K * 2).cuda()
    invalid = (torch.rand(B, K, nv, generator=g) > 0.9).float().cuda()
    invalid[::5] = 1.0
    out_c, g_c = native.pixel_loss_channels(rgb, gt, weights, invalid, crit, policy, scale_rgb=0.7)
    out_3, _, _, g_3, _ = native.pixel_loss(rgb, None, weights, invalid, gt, 2, 8, 8, crit, policy, False, False, scale_rgb=0.7)
    print(f"  {crit} {policy}: {out_c.tolist()} vs {out_3.tolist()}")
    assert abs(out_c[0].item() - out_3[0].item()) <= 1e-6 and out_c[2].item() == out_3[2].item() and out_c[3].item() == out_3[3].item() == 3 * B
    assert (g_c - g_3).abs().max().item() <= 1e-6 * max(1.0, g_3.abs().max().item())
    if policy != "none":
        assert 0 < out_c[2].item() < B


@pytest.mark.parametrize("C", [1, 5, 27])
def test_channel_loss_vs_oracle(C):
    g = torch.Generator().manual_seed(8 + C)
    B, nv, K = 777, 2, 6                               # more than one work-group, not a multiple of its rays
    rgb, gt = torch.rand(B, nv, C, generator=g), torch.rand(B, C, generator=g)
    weights = torch.rand(B, K, generator=g) / K * 2
    invalid = (torch.rand(B, K, nv, generator=g) > 0.3).float()
    for crit, policy in LOSSES:
        lo, go, bad = PC.pixel_loss(rgb.double(), gt.double(), crit, policy, invalid.double(), weights.double())
        out, gr = native.pixel_loss_channels(rgb.reshape(B, -1).cuda(), gt.cuda(), weights.cuda(), invalid.cuda(), crit, policy)
        assert abs(out[0].item() - lo.item()) <= 1e-5 and out[2].item() == bad and out[3].item() == B * C and out[1].item() == 0.0
        assert (gr.cpu().double().reshape(go.shape) - go).abs().max().item() <= 1e-4 * go.abs().max().item()
        again, gr2 = native.pixel_loss_channels(rgb.reshape(B, -1).cuda(), gt.cuda(), weights.cuda(), invalid.cuda(), crit, policy)
        assert torch.equal(out, again) and torch.equal(gr, gr2)
