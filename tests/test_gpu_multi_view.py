"""Merged encoder views (``combine_ids`` / several ``ids_encoder``) on the HIP kernels (``native_multi_view: true``) against the REAL
reference -- tests/golden/multi_view.npz (tests/golden/gen_golden_multi_view.py: the imported reference at (64, 64, 0) and (32, 32, 1), in
fp32 and in fp64) -- and against the PyTorch composition of the same tree on the GPU (a coarser decoder scale, a separate fine MLP, whole
rays of 256 samples, white background with density noise, one training step entry by entry)."""
import ast
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from oracle import bts_oracle as O
from tests._hip_helpers import make_conf
from tests._multi_view_fixture import walsh_rows

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_view.npz")
_CACHE = {}


def _load(name):
    """the fixture's arrays (read once, never modified): fp64 results rebuilt from their scaled differences, the depths from the jitter"""
    if name not in _CACHE:
        z = np.load(GOLDEN)
        t = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "_") and not k.endswith("_meta")}
        meta = ast.literal_eval(str(z[name + "_meta"]))
        for k in [k for k in t if k.startswith("f64_")]:
            t[k] = t[k[4:]].double() + t[k].double() / meta["diff_scale"]
        t["z"] = O.sample_coarse(t["rays"].reshape(-1, 8), meta["K"], True, t["u"].float())
        _CACHE[name] = (t, meta)
    return _CACHE[name]


def _view_major(f, n, V):
    """rows b * V + v (the reference's encoder batch) -> rows v * n + b (this package's, with native_multi_view)"""
    return f.view(n, V, *f.shape[1:]).transpose(0, 1).reshape(f.shape).contiguous()


def _batch_major(f, n, V):
    return f.view(V, n, *f.shape[1:]).transpose(0, 1).reshape(f.shape).contiguous()


def _net(t, meta):
    cfg = O.FieldConfig(code_mode=meta["code_mode"], learn_empty=meta["learn_empty"], empty_empty=meta["empty_empty"])
    n, V = meta["n"], len(meta["ids_encoder"])
    conf = dict(make_conf(cfg, meta["C"], meta["Hd"], meta["n_blocks"], meta["H"], meta["W"]), native_multi_view=True)
    conf["encoder"] = dict(conf["encoder"], num_views=n * V)
    net = bts.BTSNet(conf)
    with torch.no_grad():
        net.encoder.feats[0].data = _view_major(t["feats"].float(), n, V)
        for k, p in net.mlp_coarse.named_parameters():
            p.copy_(t["p_" + k.replace(".", "_")])
        if meta["learn_empty"]:
            net.empty_feature.copy_(t["empty"])
    net = net.cuda().eval()
    net.encode(t["images"].float().cuda(), t["projs"].cuda(), t["poses"].cuda(), ids_encoder=meta["ids_encoder"], ids_render=meta["ids_render"],
               combine_ids=meta["combine_ids"])
    assert not net.torch_mode and net.multi_view
    return net


def _near(got, ref32, ref64, atol, rtol, name):
    """The bar (atol + rtol |ref|), or -- where fp32 rounding of the reference itself exceeds it -- no further from the fp64 reference than
    the fp32 reference is (x 1.5 + atol), in max-norm (the rule of tests/test_gpu_mlp_color_golden.py)."""
    got, ref32, ref64 = (x.detach().cpu().double() for x in (got, ref32, ref64))
    e = (got - ref32).abs()
    e_n, e_t = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    print(f"  {name}: max err vs reference {e.max().item():.2e}; vs fp64 {e_n:.2e} (fp32 reference {e_t:.2e})")
    assert bool((e <= atol + rtol * ref32.abs()).all()) or e_n <= 1.5 * e_t + atol, name


@pytest.mark.parametrize("name", ["a", "b"])
def test_field_query_vs_reference_golden(name):
    t, meta = _load(name)
    net = _net(t, meta)
    rays = t["rays"].reshape(-1, 8)
    pts = (rays[:, None, :3] + t["z"].unsqueeze(2) * rays[:, None, 3:6]).reshape(meta["n"], -1, 3).contiguous()
    with torch.no_grad():
        rgb, inv, sig = net(pts.cuda())
    nvp = t["invalid"].shape[-1]
    assert rgb.shape == (meta["n"], pts.shape[1], 3 * nvp) and inv.shape == (meta["n"], pts.shape[1], nvp) and sig.shape == (meta["n"], pts.shape[1], 1)
    assert torch.equal(inv.cpu().reshape(t["invalid"].shape), t["invalid"]), "every flag, nothing set aside"
    err = (rgb.cpu().reshape(t["rgb_samps"].shape) - t["rgb_samps"]).abs().max().item()
    print(f"query {name}: rgb max err {err:.2e}")
    assert err <= 1e-5
    _near(sig, t["q_sigma"], t["f64_q_sigma"], 1e-6, 1e-4, "sigma")
    with pytest.raises(NotImplementedError):
        net(pts.cuda(), only_density=True)


@pytest.mark.parametrize("name", ["a", "b"])
def test_render_and_gradients_vs_reference_golden(name):
    t, meta = _load(name)
    net = _net(t, meta)
    n, K, V, C = meta["n"], meta["K"], len(meta["ids_encoder"]), meta["C"]
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    w, rgb, depth, alphas, inv, _, rgbs = r.composite(net, t["rays"].reshape(-1, 8).cuda(), t["z"].cuda(), coarse=True, sb=n)
    assert torch.equal(inv.cpu(), t["invalid"]), "every flag, nothing set aside"
    rel = ((depth.detach().cpu() - t["depth"]).abs() / t["depth"].abs().clamp_min(1e-6)).max().item()
    print(f"render {name}: depth max rel err {rel:.2e}")
    assert rel <= 1e-4
    for got, key in ((rgb, "rgb"), (w, "weights"), (alphas, "alphas")):
        assert got.shape == t[key].shape, key
        _near(got, t[key], t["f64_" + key], 1e-5, 0.0, key)
    err = (rgbs.detach().cpu() - t["rgb_samps"]).abs().max().item()       # (bilinear taps of frames in [0, 1]: the absolute bar alone)
    print(f"  rgb_samps: max err {err:.2e}")
    assert rgbs.shape == t["rgb_samps"].shape and err <= 1e-5
    params = list(net.mlp_coarse.parameters()) + [net.encoder.feats[0]] + ([net.empty_feature] if meta["learn_empty"] else [])
    names = [k for k, _ in net.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if meta["learn_empty"] else [])
    grads = torch.autograd.grad((rgb * t["gin_rgb"].cuda()).sum() + (depth * t["gin_depth"].cuda()).sum(), params)

    def check(a, b, c, what):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        e_n, e_t = (a - c).abs().max().item(), (b - c).abs().max().item()
        l_n, l_t = (a - c).norm().item(), (b - c).norm().item()
        print(f"  d{what}: max err {err:.2e} of max |g| {scale:.2e}; vs fp64 {e_n:.2e} / L2 {l_n:.2e} (reference {e_t:.2e} / {l_t:.2e})")
        if scale == 0.0:      # (case a: empty_empty zeroes the density of every sample that reads the empty feature -- no gradient reaches it)
            assert what == "empty" and meta["empty_empty"] and err == 0.0, what
            return
        assert err <= 1e-4 * scale or (e_n <= 1.5 * e_t + 2e-5 and l_n <= 1.5 * l_t + 2e-5), what

    for k, a in zip(names, grads):
        key = "g_" + k.replace(".", "_")
        a, b, c = a.detach().cpu().double(), t[key].double(), t["f64_" + key]
        if k != "feats":
            check(a, b, c, k)
            continue
        # the maps' gradient, per encoder view: in the reference's row order, and as the fixture stores it (its product with C / 4 Walsh
        # functions of the channel index, tests/golden/gen_golden_multi_view.py)
        a = torch.einsum("rc,mchw->mrhw", walsh_rows(C), _batch_major(a, n, V))
        for v in range(V):
            check(a[v::V], b[v::V], c[v::V], f"feats of encoder view {v}")


def test_jitter_form_and_reruns_are_bit_identical():
    t, meta = _load("b")
    net = _net(t, meta)
    r = bts.NeRFRenderer(n_coarse=meta["K"], lindisp=True, hard_alpha_cap=True).cuda().eval()
    rays, u = t["rays"].reshape(-1, 8).cuda(), t["u"].float().cuda()
    with torch.no_grad():
        a = r._composite(net, rays, None, True, meta["n"], True, True, True, True, False, jitter=u, want_z=True)
        b = r.composite(net, rays, a[5], coarse=True, sb=meta["n"])
        c = r.composite(net, rays, a[5], coarse=True, sb=meta["n"])
    assert torch.equal(a[5].cpu(), bts.native.sample_coarse(rays, u, True).cpu())
    for i in (0, 1, 2, 3, 4, 6):
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(b[i], c[i]), i


# ---- against the PyTorch composition of the same tree, on the GPU ---------------------------------------------------------------------
def _pair(shape, size, n, v, enc, seed, cfg=None, train=False, **extra):
    """(composition, native): the same parameters, maps, frames and cameras; the encoder's batch in each one's row order"""
    (C, Hd, nb), (H, W) = shape, size
    cfg = cfg or O.FieldConfig(learn_empty=True)
    V = len(enc["ids_encoder"])
    conf = dict(make_conf(cfg, C, Hd, nb, H, W), **{k: x for k, x in extra.items() if k != "encoder"})
    conf["encoder"] = dict(conf["encoder"], num_views=n * V, **extra.get("encoder", {}))
    scene = O.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    comp = bts.BTSNet(conf)
    with torch.no_grad():
        for mlp in (comp.mlp_coarse, comp.mlp_fine):
            for p in (mlp.parameters() if mlp is not None else ()):
                p.copy_(torch.randn(p.shape, generator=g) * (0.15 if p.dim() > 1 else 0.05))
        for f in comp.encoder.feats:
            f.copy_(torch.nn.functional.avg_pool2d(torch.randn(f.shape, generator=g), 5, 1, 2) * 3)
        if cfg.learn_empty:
            comp.empty_feature.copy_(torch.randn(C, generator=g))
    nat = bts.BTSNet(dict(conf, native_multi_view=True))
    nat.load_state_dict(comp.state_dict())
    with torch.no_grad():
        for f in nat.encoder.feats:
            f.copy_(_view_major(f.detach().clone(), n, V))
    nets = []
    for net in (comp, nat):
        net = net.cuda().train(train)
        net.encode(scene["images"].cuda(), scene["projs"].cuda(), scene["poses"].cuda(), **enc)
        nets.append(net)
    assert nets[0].torch_mode and not nets[1].torch_mode
    return nets[0], nets[1], scene


def _interior_rays(scene, views, H, W, count, seed):
    rays = O.image_rays(scene["poses"][:, views], scene["projs"][:, views], H, W, 3.0, 80.0)
    n = rays.shape[0]
    rays = rays.reshape(n, len(views), H, W, 8)[:, :, 1:-1, 1:-1].reshape(n, -1, 8)
    pick = torch.randperm(rays.shape[1], generator=torch.Generator().manual_seed(seed))[:count].sort().values
    return rays[:, pick].reshape(-1, 8).contiguous().cuda()


def _grad_rule(a, b, what, allow_zero=False):
    """within 1e-4 of the largest entry, or within 2e-5 in max-norm and L2 (then no further from fp64 than the composition is, x 1.5 + 2e-5,
    whatever fp64 is: the rule of the mlp_color step test)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, l2, scale = (a - b).abs().max().item(), (a - b).norm().item(), b.abs().max().item()
    print(f"  grad {what}: max err {err:.2e} (L2 {l2:.2e}) of max |g| {scale:.2e}")
    if scale == 0.0 and allow_zero:     # (a map, or the empty feature, that none of three rays reaches: exactly nothing on both sides)
        assert err == 0.0, what
        return
    assert scale > 0 and (err <= 1e-4 * scale or (err <= 2e-5 and l2 <= 2e-5)), what


def _render_both(comp, nat, renderer, rays, z, n, V, coarse=True, scale=0, seed=None, few_rays=False):
    """composite + the gradients of a seeded scalar through both fields -> prints and asserts; the maps' gradient per view"""
    res = []
    for net in (comp, nat):
        mlp = net.mlp(coarse)
        if seed is not None:
            torch.cuda.manual_seed(seed)          # the density noise (nerf.py:279-280): the same draw for both
        w, rgb, depth, alphas, inv, _, rgbs = renderer.composite(net, rays, z, coarse=coarse, sb=n)
        g = torch.Generator().manual_seed(11)
        loss = (rgb * torch.randn(rgb.shape, generator=g).cuda()).sum() + (depth * (torch.randn(depth.shape, generator=g) * 0.1).cuda()).sum() \
            + (w * torch.randn(w.shape, generator=g).cuda()).sum() + (alphas * torch.randn(alphas.shape, generator=g).cuda()).sum()
        params = list(mlp.parameters()) + [net.encoder.feats[scale]] + ([net.empty_feature] if net.learn_empty else [])
        grads = list(torch.autograd.grad(loss, params))
        res.append((w, rgb, depth, alphas, inv, rgbs, grads))
    (w_c, rgb_c, dep_c, al_c, inv_c, rgbs_c, g_c), (w_n, rgb_n, dep_n, al_n, inv_n, rgbs_n, g_n) = res
    assert inv_n.shape == inv_c.shape and rgb_n.shape == rgb_c.shape
    assert torch.equal(inv_n, inv_c.float()), f"{int((inv_n != inv_c).sum())} flags differ"
    rel = ((dep_n - dep_c).abs() / dep_c.abs().clamp_min(1e-6)).max().item()
    errs = {k: (a - b).abs().max().item() for k, a, b in (("rgb", rgb_n, rgb_c), ("weights", w_n, w_c), ("alphas", al_n, al_c), ("rgb_samps", rgbs_n, rgbs_c))}
    print(f"  depth rel {rel:.2e}; " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    # both sides are fp32 with their own summation orders: the composition's GPU bars of tests/test_torch_modes.py
    assert rel <= 1e-4 and errs["rgb"] <= 2e-5 and errs["weights"] <= 5e-5 and errs["alphas"] <= 5e-5 and errs["rgb_samps"] <= 1e-5
    names = [k for k, _ in comp.mlp(coarse).named_parameters()] + ["feats"] + (["empty"] if comp.learn_empty else [])
    for k, a, b in zip(names, g_n, g_c):
        if k == "feats":
            a = _batch_major(a, n, V)
            for v in range(V):
                _grad_rule(a[v::V], b[v::V], f"feats of encoder view {v}", allow_zero=few_rays)
        else:
            _grad_rule(a, b, k, allow_zero=few_rays and k == "empty")


ENC3 = dict(ids_encoder=[4, 2, 0], ids_render=[5, 3, 1], combine_ids=[(4, 2), (5, 3)])


def test_scale_1_of_a_two_scale_pyramid_vs_composition():
    comp, nat, scene = _pair((64, 64, 0), (32, 64), 2, 6, ENC3, seed=21, encoder=dict(n_scales=2, pyramid=True))
    comp.set_scale(1), nat.set_scale(1)
    rays = _interior_rays(scene, [0, 3], 32, 64, 40, 1)
    z = bts.native.sample_coarse(rays, torch.rand((rays.shape[0], 24), generator=torch.Generator().manual_seed(2)).cuda(), True)
    r = bts.NeRFRenderer(n_coarse=24, lindisp=True, hard_alpha_cap=True).cuda().eval()
    _render_both(comp, nat, r, rays, z, 2, 3, scale=1)


def test_separate_fine_mlp_vs_composition():
    comp, nat, scene = _pair((32, 32, 1), (24, 40), 2, 4, dict(ids_encoder=[2, 0], ids_render=[1, 3]), seed=22,
                             mlp_fine=dict(type="resnet", n_blocks=0, d_hidden=32))
    rays = _interior_rays(scene, [0, 3], 24, 40, 37, 3)
    z = bts.native.sample_coarse(rays, torch.rand((rays.shape[0], 16), generator=torch.Generator().manual_seed(4)).cuda(), True)
    r = bts.NeRFRenderer(n_coarse=16, lindisp=True, hard_alpha_cap=True).cuda().eval()
    _render_both(comp, nat, r, rays, z, 2, 2, coarse=False)


def test_whole_rays_of_256_samples_vs_composition():
    comp, nat, scene = _pair((32, 32, 0), (16, 32), 1, 6, ENC3, seed=23)
    rays = _interior_rays(scene, [0, 3], 16, 32, 3, 5)
    z = bts.native.sample_coarse(rays, torch.rand((3, 256), generator=torch.Generator().manual_seed(6)).cuda(), True)
    r = bts.NeRFRenderer(n_coarse=256, lindisp=True, hard_alpha_cap=True).cuda().eval()
    _render_both(comp, nat, r, rays, z, 1, 3, few_rays=True)


def test_second_group_per_work_group_vs_composition():
    """K = 96: work-group iterations of R = 2 rays, 23 of them for 45 rays (the last of one ray) on a grid of 16 work-groups, so that pass A's
    persistent loop runs twice in some: its tiles accumulate, its activations are zeroed again.  The block path (32, 32, 1)."""
    comp, nat, scene = _pair((32, 32, 1), (16, 32), 1, 6, ENC3, seed=26)
    rays = _interior_rays(scene, [0, 3], 16, 32, 45, 9)
    B, K = rays.shape[0], 96
    groups, grid = -(-B // (256 // K)), -(-(-(-B // 4)) // 8) * 8     # render_grid: a work-group per 4 rays, rounded up to 8
    assert B == 45 and groups > max(8, -(-B // 4)) and groups > grid, (B, groups, grid)
    z = bts.native.sample_coarse(rays, torch.rand((B, K), generator=torch.Generator().manual_seed(10)).cuda(), True)
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    _render_both(comp, nat, r, rays, z, 1, 3)


def test_white_background_and_density_noise_vs_composition():
    comp, nat, scene = _pair((64, 64, 0), (16, 32), 2, 6, ENC3, seed=24, train=True)
    rays = _interior_rays(scene, [0, 3], 16, 32, 45, 7)
    z = bts.native.sample_coarse(rays, torch.rand((rays.shape[0], 20), generator=torch.Generator().manual_seed(8)).cuda(), True)
    r = bts.NeRFRenderer(n_coarse=20, lindisp=True, hard_alpha_cap=False, white_bkgd=True, noise_std=0.3).cuda().train()
    _render_both(comp, nat, r, rays, z, 2, 3, seed=9)


def test_training_step_entry_by_entry_vs_composition():
    """PatchRaySampler -> NeRFRenderer (density noise from a fixed seed) -> ReconstructionLoss -> backward, 8 x 8 patches, three encoder
    views with combine_ids: the native field against the composition with the same draws."""
    results = []
    n, V = 2, 3
    for which in (0, 1):
        net = _pair((64, 64, 0), (32, 64), n, 6, ENC3, seed=25, cfg=O.FieldConfig(learn_empty=False), train=True)[which]
        scene = O.synthetic_scene(n, 6, 32, 64, 64, seed=25, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
        imgs, projs, poses = scene["images"].cuda(), scene["projs"].cuda(), scene["poses"].cuda()
        renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=32, lindisp=True, hard_alpha_cap=True, noise_std=0.3)).cuda().train()
        wrapped = renderer.bind_parallel(net).train()
        sampler = bts.PatchRaySampler(ray_batch_size=8 * 8 * 8, z_near=3.0, z_far=80.0, patch_size=8)
        torch.manual_seed(5)
        rays, rgb_gt = sampler.sample(imgs[:, [0, 3]] * .5 + .5, poses[:, [0, 3]], projs[:, [0, 3]])
        torch.cuda.manual_seed(7)     # the jitter (nerf.py:112) and the density noise (nerf.py:279-280): the same draws for both
        rd = wrapped(rays, want_weights=True, want_alphas=True, want_rgb_samps=True)
        rd["fine"] = dict(rd["coarse"])
        rd["rgb_gt"] = rgb_gt
        rd = sampler.reconstruct(rd)
        crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "none", "lambda_edge_aware_smoothness": 0.001})
        loss, _ = crit(dict(coarse=[rd["coarse"]], fine=[rd["fine"]], rgb_gt=rd["rgb_gt"]))
        loss.backward()
        feats = net.encoder.feats[0].grad
        results.append((loss.item(), [p.grad for p in net.mlp_coarse.parameters()] + [_batch_major(feats, n, V) if which else feats]))
    (l_t, g_t), (l_n, g_n) = results
    print(f"training step: loss {l_n:.6f} vs composition {l_t:.6f}")
    assert abs(l_n - l_t) <= 1e-5
    for i, (a, b) in enumerate(zip(g_n, g_t)):
        _grad_rule(a, b, i)


def test_only_density_with_several_views_still_raises():
    t, meta = _load("b")
    net = _net(t, meta)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(meta["n"], 4, 3, device="cuda"), only_density=True)
    with pytest.raises(bts.BtsNativeError, match="more than one encoder view"):
        net.occupancy_profile(torch.zeros(meta["n"], 8, 3, device="cuda"), 2)
