"""MLP-predicted colour (``sample_color: false``, ``native_mlp_color: true``) against the REAL reference: tests/golden/mlp_color.npz
(tests/golden/gen_golden_mlp_color.py runs the imported reference at (64, 64, 0) and (32, 32, 1), in fp32 and in fp64), plus a
training step entry by entry (PatchRaySampler -> renderer -> ReconstructionLoss -> backward) against the same step through the PyTorch
composition, and the separate fine MLP."""
import ast
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from oracle import bts_oracle as O
from tests._hip_helpers import make_conf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_color.npz")


def _load(name):
    z = np.load(GOLDEN)
    t = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "_") and not k.endswith("_meta")}
    return t, ast.literal_eval(str(z[name + "_meta"]))


def _net(t, meta):
    cfg = O.FieldConfig(code_mode=meta["code_mode"], learn_empty=meta["learn_empty"], empty_empty=meta["empty_empty"])
    conf = dict(make_conf(cfg, meta["C"], meta["Hd"], meta["n_blocks"], meta["H"], meta["W"]), sample_color=False, native_mlp_color=True)
    net = bts.BTSNet(conf)
    with torch.no_grad():
        net.encoder.feats[0].data = t["feats"].float().clone()
        for k, p in net.mlp_coarse.named_parameters():
            p.copy_(t["p_" + k.replace(".", "_")])
        if meta["learn_empty"]:
            net.empty_feature.copy_(t["empty"])
    net = net.cuda().eval()
    images = torch.zeros((meta["n"], meta["v"], 3, meta["H"], meta["W"]), device="cuda")     # (this head reads no frames)
    net.encode(images, t["projs"].cuda(), t["poses"].cuda(), ids_encoder=[0], ids_render=meta["ids_render"])
    return net


def _near(got, ref32, ref64, mask, atol, rtol, name):
    """The issue's bar (atol + rtol |ref|), or -- where fp32 rounding of the reference itself exceeds it -- no further from the fp64
    reference than the fp32 reference is (x 1.5 + atol), in max-norm."""
    got, ref32, ref64 = (x.detach().cpu().double()[mask] for x in (got, ref32, ref64))
    e = (got - ref32).abs()
    e_n, e_t = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    print(f"  {name}: max err vs reference {e.max().item():.2e}; vs fp64 {e_n:.2e} (fp32 reference {e_t:.2e})")
    assert bool((e <= atol + rtol * ref32.abs()).all()) or e_n <= 1.5 * e_t + atol, name


@pytest.mark.parametrize("name", ["a", "b"])
def test_field_query_vs_reference_golden(name):
    t, meta = _load(name)
    net = _net(t, meta)
    n = meta["n"]
    rays, z = t["rays"].reshape(-1, 8), t["z"]
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(n, -1, 3).contiguous()
    with torch.no_grad():
        rgb, inv, sig = net(pts.cuda())
        d_rgb, d_inv, d_sig = net(pts.cuda(), only_density=True)
    same = (inv.cpu() == t["q_invalid"]).squeeze(-1)
    print(f"query {name}: {int((~same).sum())} of {same.numel()} points with a flipped frustum flag")
    assert same.float().mean().item() > 0.995
    _near(rgb, t["q_rgb"], t["f64_q_rgb"], same, 1e-5, 0.0, "rgb")
    _near(sig, t["q_sigma"], t["f64_q_sigma"], same, 1e-6, 1e-4, "sigma")
    assert torch.count_nonzero(d_rgb) == 0
    _near(d_sig, t["qd_sigma"], t["f64_qd_sigma"], same, 1e-6, 1e-4, "sigma (only_density)")
    assert torch.equal(d_inv.cpu().reshape(-1), t["qd_invalid"].reshape(-1).float()) or (d_inv.cpu().reshape(-1) == t["qd_invalid"].reshape(-1)).float().mean() > 0.995


@pytest.mark.parametrize("name", ["a", "b"])
def test_render_and_gradients_vs_reference_golden(name):
    t, meta = _load(name)
    net = _net(t, meta)
    n, K = meta["n"], meta["K"]
    dead = t["dead"]
    print(f"golden {name}: dead-density share {dead.float().mean().item():.2f}, {int(t['dead_only_texels'].sum())} texels reached by dead samples only")
    assert dead.float().mean().item() >= 0.10 and t["dead_only_texels"].any()
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    w, rgb, depth, alphas, inv, _, rgbs = r.composite(net, t["rays"].reshape(-1, 8).cuda(), t["z"].cuda(), coarse=True, sb=n)
    ok = (inv.cpu() == t["invalid"]).all(-1).all(-1)
    print(f"render {name}: {int((~ok).sum())} of {ok.numel()} rays set aside (flipped frustum flag)")
    assert ok.float().mean().item() > 0.98
    rel = ((depth.detach().cpu() - t["depth"]).abs() / t["depth"].abs().clamp_min(1e-6))[ok].max().item()
    print(f"  depth: max rel err {rel:.2e}")
    assert rel <= 1e-4
    for got, key in ((rgb, "rgb"), (w, "weights"), (alphas, "alphas")):
        _near(got, t[key], t["f64_" + key], ok, 1e-5, 0.0, key)
    _near(rgbs, t["rgb_samps"], t["f64_q_rgb"].reshape(t["rgb_samps"].shape), ok, 1e-5, 0.0, "rgb_samps")
    assert torch.equal(inv.cpu()[ok], t["invalid"][ok])
    assert ok.all(), "the gradient golden covers every ray"
    params = list(net.mlp_coarse.parameters()) + [net.encoder.feats[0]] + ([net.empty_feature] if meta["learn_empty"] else [])
    names = [k for k, _ in net.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if meta["learn_empty"] else [])
    grads = torch.autograd.grad((rgb * t["gin_rgb"].cuda()).sum() + (depth * t["gin_depth"].cuda()).sum(), params)
    for k, a in zip(names, grads):
        key = "g_" + k.replace(".", "_")
        b = t[key]
        c = b.double() + t["f64_" + key].double() if k == "feats" else t["f64_" + key].double()
        scale = b.abs().max().item()
        a = a.detach().cpu().double()
        err = (a - b.double()).abs().max().item()
        e_n, e_t = (a - c).abs().max().item(), (b.double() - c).abs().max().item()
        l_n, l_t = (a - c).norm().item(), (b.double() - c).norm().item()
        print(f"  d{k}: max err {err:.2e} of max |g| {scale:.2e}; vs fp64 {e_n:.2e} / L2 {l_n:.2e} (reference {e_t:.2e} / {l_t:.2e})")
        assert err <= 1e-4 * scale or (e_n <= 1.5 * e_t + 2e-5 and l_n <= 1.5 * l_t + 2e-5), k
        if k == "feats":
            # the texels only dead-density samples reach: their gradient is all colour (a liveness slot holding dL/do0 would drop it)
            m = t["dead_only_texels"].unsqueeze(1).expand_as(b)
            sub, sub_ref = a[m], b.double()[m]
            err_d = (sub - sub_ref).abs().max().item()
            print(f"  dfeats on dead-only texels: max err {err_d:.2e} of max |g| {sub_ref.abs().max().item():.2e}")
            assert sub_ref.abs().max().item() > 0 and err_d <= 1e-4 * scale + (1.5 * (b.double() - c)[m].abs().max().item() + 2e-5)


def _step_nets(mode, seed=3, n=2, H=32, W=64, C=64, Hd=64):
    cfg = O.FieldConfig(learn_empty=False)
    conf = dict(make_conf(cfg, C, Hd, 0, H, W), sample_color=False, native_mlp_color=(mode == "native"))
    conf["encoder"] = dict(conf["encoder"], n_scales=2, pyramid=True)
    torch.manual_seed(seed)
    net = bts.BTSNet(conf)
    g = torch.Generator().manual_seed(seed)
    scene = O.synthetic_scene(n, 3, H, W, C, seed=seed, smooth=True)
    with torch.no_grad():
        net.encoder.feats[0].data = scene["feat"].clone()
        net.encoder.feats[1].data = torch.nn.functional.avg_pool2d(scene["feat"], 2).clone()
        for p in net.mlp_coarse.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.15 if p.dim() > 1 else 0.05))
    return net.cuda().train(), scene


@pytest.mark.parametrize("scale", [0, 1])
def test_training_step_entry_by_entry_vs_composition(scale):
    """PatchRaySampler -> NeRFRenderer (density noise from a fixed seed) -> ReconstructionLoss -> backward; scale 1 renders the half-size
    decoder map through feat_shift 1.  The same step through the PyTorch composition on the GPU: the same jitter and noise draws."""
    results = []
    for mode in ("torch", "native"):
        net, scene = _step_nets(mode)
        imgs, projs, poses = scene["images"].cuda(), scene["projs"].cuda(), scene["poses"].cuda()
        net.encode(imgs, projs, poses, ids_encoder=[0], ids_render=[1, 2])
        net.set_scale(scale)
        renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=32, lindisp=True, hard_alpha_cap=True, noise_std=0.3)).cuda().train()
        wrapped = renderer.bind_parallel(net).train()
        sampler = bts.PatchRaySampler(ray_batch_size=8 * 8 * 8, z_near=3.0, z_far=80.0, patch_size=8)
        torch.manual_seed(5)
        rays, rgb_gt = sampler.sample(imgs[:, 1:] * .5 + .5, poses[:, 1:], projs[:, 1:])
        torch.cuda.manual_seed(7)     # the jitter (nerf.py:112) and the density noise (nerf.py:279-280): the same draws for both modes
        rd = wrapped(rays, want_weights=True, want_alphas=True, want_rgb_samps=True)
        rd["fine"] = dict(rd["coarse"])
        rd["rgb_gt"] = rgb_gt
        rd = sampler.reconstruct(rd)
        crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "none", "lambda_edge_aware_smoothness": 0.001})
        loss, _ = crit(dict(coarse=[rd["coarse"]], fine=[rd["fine"]], rgb_gt=rd["rgb_gt"]))
        loss.backward()
        results.append((loss.item(), [p.grad.detach().cpu().double() for p in
                                      list(net.mlp_coarse.parameters()) + [net.encoder.feats[scale]]]))
    (l_t, g_t), (l_n, g_n) = results
    print(f"training step, scale {scale}: loss {l_n:.6f} vs composition {l_t:.6f}")
    assert abs(l_n - l_t) <= 1e-5
    # the rule of tests/test_gpu_fused_anchor.py::_check_grads: within 1e-4 of the largest entry, or no further from fp64 than the fp32
    # composition is (x 1.5 + 2e-5, max-norm and L2).  This step has no fp64 twin (the fused loss pass is fp32), but the second branch
    # holds whatever fp64 is whenever |native - composition| <= 2e-5 in both norms (triangle inequality): that is what is checked
    for i, (a, b) in enumerate(zip(g_n, g_t)):
        err, l2, scale_ = (a - b).abs().max().item(), (a - b).norm().item(), b.abs().max().item()
        print(f"  grad {i}: max err {err:.2e} (L2 {l2:.2e}) of max |g| {scale_:.2e}")
        assert scale_ > 0 and (err <= 1e-4 * scale_ or (err <= 2e-5 and l2 <= 2e-5)), i


def test_separate_fine_mlp_through_the_same_entries():
    """`mlp_fine: {type: resnet}`: coarse=False renders with THAT four-output MLP (its own packed vector and projected map)."""
    cfg = O.FieldConfig()
    outs = []
    for native in (False, True):
        conf = dict(make_conf(cfg, 32, 32, 1, 24, 40), sample_color=False, native_mlp_color=native,
                    mlp_fine=dict(type="resnet", n_blocks=0, d_hidden=32))
        torch.manual_seed(0)
        net = bts.BTSNet(conf)
        scene = O.synthetic_scene(2, 3, 24, 40, 32, seed=4, smooth=True)
        with torch.no_grad():
            net.encoder.feats[0].data = scene["feat"].clone()
        net = net.cuda().eval()
        net.encode(scene["images"].cuda(), scene["projs"].cuda(), scene["poses"].cuda(), ids_encoder=[0], ids_render=[1, 2])
        assert net.torch_mode != native
        rays = O.image_rays(scene["poses"], scene["projs"], 24, 40, 3.0, 80.0)[:, ::9].reshape(-1, 8).contiguous().cuda()
        z = bts.native.sample_coarse(rays, torch.rand((rays.shape[0], 16), generator=torch.Generator().manual_seed(1)).cuda(), True)
        r = bts.NeRFRenderer(n_coarse=16, lindisp=True, hard_alpha_cap=True).cuda().eval()
        w, rgb, depth, _, inv, _, _ = r.composite(net, rays, z, coarse=False, sb=2)
        g = torch.autograd.grad(rgb.sum() + depth.sum(), [net.mlp_fine.lin_out.weight])[0]
        outs.append((rgb.detach(), depth.detach(), inv, g))
    (rgb_t, dep_t, inv_t, g_t), (rgb_n, dep_n, inv_n, g_n) = outs
    ok = (inv_t == inv_n).all(-1).all(-1)
    assert ok.float().mean().item() > 0.95
    assert (rgb_t - rgb_n)[ok].abs().max().item() < 1e-4 and ((dep_t - dep_n).abs() / dep_t.abs())[ok].max().item() < 1e-4
    if ok.all():
        assert (g_t - g_n).abs().max().item() <= 1e-4 * g_t.abs().max().item()


def test_full_eval_frame_vs_composition():
    """The eval_depth frame: 1 x 192 x 640 rays, K = 64, (64, 64, 0), through NeRFRenderer against torch_modes.composite on the CPU
    (in ray chunks).  In-kernel sampling (jitter) is bit-identical to the explicit-z_samp form."""
    n, H, W, C, K = 1, 192, 640, 64, 64
    cfg = O.FieldConfig(learn_empty=True)
    scene = O.synthetic_scene(n, 2, H, W, C, seed=9, smooth=True)
    nets = {}
    for native, dt in ((False, torch.float32), (False, torch.float64), (True, torch.float32)):
        conf = dict(make_conf(cfg, C, 64, 0, H, W), sample_color=False, native_mlp_color=native)
        net = bts.BTSNet(conf)
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            net.encoder.feats[0].data = scene["feat"].clone()
            for p in net.mlp_coarse.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.15 if p.dim() > 1 else 0.05))
            net.empty_feature.copy_(torch.randn(C, generator=g))
        dev = "cuda" if native else "cpu"
        net = net.to(dev, dt).eval()
        net.encode(scene["images"].to(dev, dt), scene["projs"].to(dev, dt), scene["poses"].to(dev, dt), ids_encoder=[0], ids_render=[0])
        nets[True if native else dt] = net
    rays = O.image_rays(scene["poses"][:, :1], scene["projs"][:, :1], H, W, 3.0, 80.0).reshape(-1, 8).contiguous()
    u = torch.rand((rays.shape[0], K), generator=torch.Generator().manual_seed(3))
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
    with torch.no_grad():
        a = r._composite(nets[True], rays.cuda(), None, True, n, True, True, True, True, False, jitter=u.cuda(), want_z=True)
        z = a[5]
        b = r.composite(nets[True], rays.cuda(), z, coarse=True, sb=n)
    for i in (0, 1, 2, 3, 4, 6):
        assert torch.equal(a[i], b[i]), i
    z = z.cpu()
    depth_t, inv_t, depth_64, inv_64 = [], [], [], []
    with torch.no_grad():
        for s in range(0, rays.shape[0], 8192):
            out = bts.torch_modes.composite(r, nets[torch.float32], rays[s:s + 8192], z[s:s + 8192], coarse=True, sb=1)
            depth_t.append(out[2]), inv_t.append(out[4])
            out = bts.torch_modes.composite(r, nets[torch.float64], rays[s:s + 8192].double(), z[s:s + 8192].double(), coarse=True, sb=1)
            depth_64.append(out[2]), inv_64.append(out[4])
    depth_t, inv_t, depth_64, inv_64 = torch.cat(depth_t), torch.cat(inv_t), torch.cat(depth_64), torch.cat(inv_64)
    ok = (b[4].cpu() == inv_t).all(-1).all(-1)
    # gen_rays (util.py:244-273) places the outermost pixel rows and columns at x, y = +-1 EXACTLY: their points lie on the frustum border,
    # where the `< -1` / `> 1` tests are decided by the last bit of the projection (any other summation order flips them)
    row, col = torch.arange(rays.shape[0]) // W, torch.arange(rays.shape[0]) % W
    tie = (row == 0) | (row == H - 1) | (col == 0) | (col == W - 1)
    print(f"full frame: {int((~ok).sum())} of {ok.numel()} rays set aside at the frustum border, {int((~ok & ~tie).sum())} of them off the "
          f"{int(tie.sum())} rays that lie on it")
    assert (~ok & ~tie).float().mean().item() <= 0.005
    ok = ok & (inv_64 == inv_t).all(-1).all(-1)
    d_n, d_t = b[2].cpu().double(), depth_t.double()
    rel = ((d_n - d_t).abs() / d_t.abs().clamp_min(1e-6))[ok].max().item()
    # the bar, or -- where fp32 rounding of the composition itself exceeds it -- no further from fp64 than the composition is (x 1.5)
    rel_n = ((d_n - depth_64).abs() / depth_64.abs())[ok].max().item()
    rel_t = ((d_t - depth_64).abs() / depth_64.abs())[ok].max().item()
    print(f"  depth: max rel err {rel:.2e}; vs fp64 {rel_n:.2e} (fp32 composition {rel_t:.2e})")
    assert rel <= 1e-4 or rel_n <= 1.5 * rel_t + 1e-6
