"""GPU: auto-masking -- the error map (bts_automask_errors, csrc/bts_automask.hip) and the per-pixel bound in the three loss kernels
(bts_photometric_loss_automask, bts_photometric_loss_tiled_automask, bts_pixel_loss_automask) -- against tests/golden/automask.npz (the
REAL reference: compute_errors_l1ssim inside trainer.py:203-206, ReconstructionLoss(cfg, True)) and the CPU restatement
tests/_automask_oracle.py (pinned to that golden in tests/test_automask_cpu.py).

Bars.  Loss 1e-5 absolute, gradients 1e-4 of the largest entry: the project's bars against the reference's goldens.  Map: the kernel's
largest distance to the stored fp64 map may be at most 2 x the fp32 reference's own largest distance to it on that case (stored in the
golden, printed by its generator: 6.3e-6 / 5.5e-6 / 5.5e-6 / 9.1e-7 on the four cases, so the bars are 1.3e-5 / 1.1e-5 / 1.1e-5 /
1.8e-6) -- a different but equally valid fp32 order of operations gets the allowance the reference took, and no more (measured on MI355X:
6.1e-6 / 5.7e-6 / 5.8e-6 / 1.45e-6).  The golden's
generator asserts that outside the constructed tie block no compared value is within 1e-4 of its bound, so no rounding difference flips
a choice and no value is set aside anywhere."""

import numpy as np
import pytest
import torch

from tests import _automask_oracle as AO

pytestmark = pytest.mark.gpu
KEYS = {"native_automask": True, "native_pixel_loss": True}
_CACHE = {}


def _z():
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(AO.GOLDEN)
    return _CACHE["z"]


def _golden(layout):
    """the layout's inputs (CPU tensors), loaded once and left unchanged"""
    if layout not in _CACHE:
        _CACHE[layout] = AO.load_inputs(_z(), layout)
    return _CACHE[layout]


# ---- the map ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(AO.MAP_CASES))
def test_the_map_vs_the_real_reference(case):
    import behindthescenes_amd as bts
    z = _z()
    n, v, H, W, ids = AO.MAP_CASES[case]
    x = AO.map_frames(z, case).cuda()
    errors = bts.automask_errors(x, ids, n_render=len(ids))
    four = bts.automask_images(x, ids)
    assert errors.shape == (n, v, 1, H, W) and four.shape == (n, v, 4, H, W)
    m64, bar = torch.from_numpy(z[f"map_{case}_ref64"]), 2 * z[f"map_{case}_dist"].item()
    dist = (errors[:, :, 0].cpu().double() - m64).abs().max().item()
    d32 = (errors[:, :, 0].cpu() - torch.from_numpy(z[f"map_{case}_ref32"])).abs().max().item()
    print(case, "kernel to fp64:", dist, "bar (2 x the fp32 reference's):", bar, "| kernel to the fp32 reference:", d32)
    assert dist <= bar, (dist, bar)
    assert torch.equal(four[:, :, :3], x) and torch.equal(four[:, :, 3], errors[:, :, 0])
    again, four2 = bts.automask_errors(x, ids), bts.automask_images(x, ids)
    assert torch.equal(again, errors) and torch.equal(four2, four)                  # reruns are bit-identical


def test_the_map_reads_its_partners_in_any_order_and_says_no_to_unequal_counts():
    import behindthescenes_amd as bts
    x = AO.map_frames(_z(), "repeat").cuda()
    a, b = bts.automask_errors(x, [3, 0, 3, 5]), bts.automask_errors(x, torch.tensor([3, 0, 3, 5]))
    assert torch.equal(a, b)
    # another order of the same partners: the same four terms per pixel, added in another order (a few ulp of a mean below 0.5)
    assert (bts.automask_errors(x, [0, 5, 3, 3]) - a).abs().max().item() <= 1e-6
    assert (bts.automask_errors(x, [0, 5, 3]) - a).abs().max().item() > 1e-3                # the repeat counts twice in the mean
    with pytest.raises(ValueError):
        bts.automask_images(x, [3, 0, 3, 5], n_render=3)


# ---- the loss through ReconstructionLoss ------------------------------------------------------------------------------
def _hip(level_cpu, gt4, config, lean=False, grad=True):
    import behindthescenes_amd as bts
    r1, d1 = level_cpu["rgb"].detach().cuda().requires_grad_(grad), level_cpu["depth"].detach().cuda().requires_grad_(grad)
    if lean:
        w, i = level_cpu["weights"], level_cpu["invalid"]
        level = dict(invalid_wsum=(i * w.unsqueeze(-1)).sum(-2).cuda(), invalid_any=i.amax(-2).cuda())
    else:
        level = {k: v.cuda() for k, v in level_cpu.items() if k not in ("rgb", "depth")}
    level.update(rgb=r1, depth=d1)
    crit = bts.ReconstructionLoss(dict(config, **KEYS), use_automasking=True)
    loss, parts = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt4.cuda()))
    if grad:
        loss.backward()
    return loss, parts, r1.grad, d1.grad


@pytest.mark.parametrize("cname", list(AO.CONFIGS))
@pytest.mark.parametrize("layout", list(AO.LAYOUTS))
def test_loss_vs_the_real_reference(layout, cname):
    z = _z()
    level, gt = _golden(layout)
    thresh = AO.load_thresh(z, layout, cname)
    key = f"am_{layout}_{cname}"
    want = dict(zip(AO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    loss, parts, g_r, g_d = _hip(level, torch.cat((gt, thresh.unsqueeze(-1)), -1), AO.config_of(cname), lean=cname.endswith("_lean"))
    assert list(parts) == ["loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_eas",
                           "loss_depth_smoothness", "loss_invalid_ratio", "loss"]
    ref, ref_gr, ref_gd = z[f"{key}_loss"].item(), torch.from_numpy(z[f"{key}_g_rgb"]), torch.from_numpy(z[f"{key}_g_depth"])
    errs = {name: (got.cpu() - w).abs().max().item() / w.abs().max().clamp_min(1e-20).item() for got, w, name in ((g_r, ref_gr, "rgb"), (g_d, ref_gd, "depth"))}
    print(key, "loss", loss.item(), ref, "eas", parts["loss_eas"], want["loss_eas"], "invalid", parts["loss_invalid_ratio"], want["loss_invalid_ratio"],
          "gradient errors", errs)
    assert abs(loss.item() - ref) <= 1e-5 and abs(parts["loss"] - ref) <= 1e-5
    assert abs(parts["loss_invalid_ratio"] - want["loss_invalid_ratio"]) <= 1e-6
    assert abs(parts["loss_eas"] - want["loss_eas"]) <= 1e-5 * max(1.0, abs(want["loss_eas"]))
    for k in ("loss_rgb_coarse", "loss_rgb_fine"):
        assert abs(parts[k] - want[k]) <= 1e-5, k
    for name, err in errs.items():
        assert err <= 1e-4, (name, err)
    if AO.crit_key(cname) != "ssim":
        # the constructed block: e == thresh exactly, the blue channel of view 0 alone attains the minimum -> HALF of the full gradient
        c = AO.CONFIGS[cname]
        block = torch.from_numpy(z[f"am_{layout}_tie_block"])
        sel = block & (AO.PO.invalid_rays(level, c["invalid_policy"]).squeeze(-1) == 0)
        _, o = AO.reconstruction_loss(level, torch.cat((gt, thresh.unsqueeze(-1)), -1), AO.config_of(cname))
        count = o["kept"] if o["kept"] is not None else 3 * level["depth"].numel()
        full = 2.0 / count * (1.0 if c["criterion"] == "l1" else 2 * 0.125)      # (lambda_coarse + lambda_fine) / count * d crit / d rgb at +1/8
        got = g_r.cpu()[sel][:, 0, 2]
        print(key, "tie block:", int(sel.sum()), "rays, gradient", got[0].item(), "half of", full)
        assert sel.any() and torch.allclose(got, torch.full_like(got, 0.5 * full), rtol=1e-5, atol=0)


# ---- the three entry points directly ----------------------------------------------------------------------------------
def _flat(level, gt):
    n, pc, h, w, nv, _ = level["rgb"].shape
    K = level["weights"].shape[-1]
    f = lambda t, *tail: t.reshape((-1,) + tail).float().contiguous().cuda()
    return dict(rgb=f(level["rgb"], nv * 3), depth=f(level["depth"]), weights=f(level["weights"], K), invalid=f(level["invalid"], K, nv),
                rgb_samps=f(level["rgb_samps"], K, nv, 3), rgb_gt=f(gt, 3)), (n, h, w)


def _photometric(layout, thresh):
    from behindthescenes_amd import native
    level, gt = _golden(layout)
    t, (n, h, w) = _flat(level, gt)
    return native.photometric_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], h, w, "weight_guided", True, 1.0, 1.0, thresh=thresh)


def _pixel(layout, cname, thresh):
    from behindthescenes_amd import native
    level, gt = _golden(layout)
    t, (n, h, w) = _flat(level, gt)
    c = AO.CONFIGS[cname]
    out, thr, kept, g_rgb, g_depth = native.pixel_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], n, h, w, c["criterion"], c["invalid_policy"],
                                                       c.get("median_thresholding", False), True, 1.0, 1.0, rgb_samps=t["rgb_samps"], thresh=thresh)
    return out, g_rgb, g_depth


@pytest.mark.parametrize("layout", ["p8", "p16", "ragged"])
def test_an_infinite_bound_is_the_base_entry_point_bit_for_bit_ssim(layout):
    """p8: the wave kernel; p16 / ragged: the tiled passes"""
    B = _golden(layout)[0]["depth"].numel()
    inf = torch.full((B,), float("inf"), device="cuda")
    a, b = _photometric(layout, None), _photometric(layout, inf)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[1].abs().max() > 0 and a[2].abs().max() > 0
    bound = _photometric(layout, AO.load_thresh(_z(), layout, "ssim_wg").reshape(-1).cuda())
    assert not torch.equal(bound[0], a[0]) and not torch.equal(bound[1], a[1]) and torch.equal(bound[2], a[2])     # (the bound does not touch depth)


@pytest.mark.parametrize("cname", ["l2", "l1_median", "l2_diverse"])
def test_an_infinite_bound_is_the_base_entry_point_bit_for_bit_pixel(cname):
    B = _golden("median")[0]["depth"].numel()
    a, b = _pixel("median", cname, None), _pixel("median", cname, torch.full((B,), float("inf"), device="cuda"))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[1].abs().max() > 0
    bound = _pixel("median", cname, AO.load_thresh(_z(), "median", cname).reshape(-1).cuda())
    assert not torch.equal(bound[0], a[0]) and torch.equal(bound[2], a[2])


def test_small_patches_through_the_tiled_entry_agree_with_the_wave_entry():
    """HIP against HIP, with the bound: the 8 x 8 layout through bts_photometric_loss_tiled_automask and bts_photometric_loss_automask"""
    from behindthescenes_amd import _lib, native
    level, gt = _golden("p8")
    t, (n, h, w) = _flat(level, gt)
    thresh = AO.load_thresh(_z(), "p8", "ssim_wg").reshape(-1).contiguous().cuda()
    wave = native.photometric_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], h, w, "weight_guided", True, 1.0, 1.0, thresh=thresh)
    B, nv, K = t["rgb_gt"].shape[0], level["rgb"].shape[-2], level["weights"].shape[-1]
    parts = torch.empty(B // (h * w), 4, device="cuda")
    g_rgb, g_depth = torch.empty_like(t["rgb"]), torch.empty_like(t["depth"])
    a = _lib.BtsLossArgs(rgb=t["rgb"].data_ptr(), depth=t["depth"].data_ptr(), weights=t["weights"].data_ptr(), invalid=t["invalid"].data_ptr(),
                         rgb_gt=t["rgb_gt"].data_ptr(), parts=parts.data_ptr(), g_rgb=g_rgb.data_ptr(), g_depth=g_depth.data_ptr(),
                         n_patches=B // (h * w), patch_h=h, patch_w=w, nv=nv, K=K, invalid_policy=2, edge_aware_smoothness=1, scale_rgb=1.0,
                         scale_eas=1.0, invalid_wsum=None, invalid_any=None)
    native.photometric_loss_tiled(a, parts, g_rgb, g_depth, native._stream(t["rgb"]), thresh)
    d = [(x - y).abs().max().item() for x, y in zip(wave, (parts, g_rgb, g_depth))]
    print("tiled vs wave with the bound: parts", d[0], "g_rgb", d[1], "g_depth", d[2])
    assert (wave[0][:, :3] - parts[:, :3]).abs().max().item() <= 1e-6 * max(1.0, wave[0][:, :3].abs().max().item())
    assert d[1] <= 1e-6 * max(1.0, wave[1].abs().max().item()) and d[2] <= 1e-6 * max(1.0, wave[2].abs().max().item())
    assert wave[1].abs().max() > 0


def test_no_grad_runs_the_forward_only():
    level, gt = _golden("p16")
    gt4 = torch.cat((gt, AO.load_thresh(_z(), "p16", "ssim_wg").unsqueeze(-1)), -1)
    with torch.no_grad():
        l0, p0, _, _ = _hip(level, gt4, AO.config_of("ssim_wg"), grad=False)
    l1, p1, g_r, _ = _hip(level, gt4, AO.config_of("ssim_wg"))
    assert not l0.requires_grad and torch.equal(l0, l1.detach()) and dict(p0) == dict(p1) and g_r is not None


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_end_to_end_map_encode_sample_render_loss_backward():
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    n, V, H, W, K = 2, 4, 24, 40, 8
    ids_loss, ids_render = [0, 1], [2, 3]
    scene = S.synthetic_scene(n, V, H, W, 64, seed=5, baseline=0.4, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to("cuda").train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).to("cuda").train()
    wrapped = renderer.bind_parallel(net).train()
    sampler = bts.PatchRaySampler(ray_batch_size=128, z_near=3.0, z_far=80.0, patch_size=8, channels=4)
    images, projs, poses = (scene[k].cuda() for k in ("images", "projs", "poses"))
    images_ip = images * .5 + .5
    patches = (torch.tensor([[0, 1], [1, 0]]), torch.tensor([[3, 16], [0, 9]]), torch.tensor([[5, 32], [17, 0]]))       # view, y0, x0 per sample
    take = lambda t, ids: t[:, ids].contiguous()

    def step(alt):
        net.encode(images, projs, poses, ids_encoder=[0], ids_render=ids_render, images_alt=alt)
        rays, gt = sampler.sample(take(images4, ids_loss), take(poses, ids_loss), take(projs, ids_loss), patches=patches)
        torch.manual_seed(11)                                      # the jitter of sample_coarse
        rd = wrapped(rays, want_weights=True, want_alphas=True, want_rgb_samps=True)
        rd["fine"] = dict(rd["coarse"])
        rd["rgb_gt"] = gt
        return sampler.reconstruct(rd)

    images4 = bts.automask_images(images_ip, ids_loss, len(ids_render))
    rd = step(images4)
    c = rd["coarse"]
    nv = len(ids_render)
    assert c["rgb"].shape == (2, 2, 8, 8, nv, 3) and rd["rgb_gt"].shape == (2, 2, 8, 8, 4) and c["rgb_samps"].shape == (2, 2, 8, 8, K, nv, 3)
    assert net.grid_c_imgs.shape == (n, nv, 4, H, W)             # what the reference would hold
    # the bound the sampler hands on IS the map at the patches' pixels
    want_map = AO.error_map(images_ip.cpu(), ids_loss)[:, :, 0][:, ids_loss]
    for s in range(n):
        for p in range(2):
            v, y0, x0 = (int(t[s, p]) for t in patches)
            assert (rd["rgb_gt"][s, p, :, :, 3].cpu() - want_map[s, v, y0:y0 + 8, x0:x0 + 8]).abs().max().item() <= 1.3e-5
            assert torch.equal(rd["rgb_gt"][s, p, :, :, :3].cpu(), images_ip[s, ids_loss[v], :, y0:y0 + 8, x0:x0 + 8].permute(1, 2, 0).cpu())
    c["rgb"].retain_grad()
    cfg = dict(criterion="l1+ssim", invalid_policy="weight_guided", lambda_edge_aware_smoothness=AO.LAMBDA_EAS)
    crit = bts.ReconstructionLoss(dict(cfg, native_automask=True), use_automasking=True)
    loss, parts = crit(dict(coarse=[c], fine=[rd["fine"]], rgb_gt=rd["rgb_gt"]))
    loss.backward()
    level = {k: c[k].detach().cpu() for k in ("rgb", "depth", "weights", "invalid")}
    level["rgb"].requires_grad_(True)
    gt4 = rd["rgb_gt"].detach().cpu()
    ref, o = AO.reconstruction_loss(level, gt4, cfg)
    ref_g, = torch.autograd.grad(ref, [level["rgb"]])
    e0 = AO.errors_before_bound(level, gt4[..., :3], cfg).detach()
    err_g = (c["rgb"].grad.cpu() - ref_g).abs().max().item() / ref_g.abs().max().item()
    print("end to end: loss", loss.item(), ref.item(), "gradient error", err_g, "bound share", o["bound"], "closest e to its bound",
          (e0 - gt4[..., 3:]).abs().min().item())
    assert abs(loss.item() - ref.item()) <= 1e-5 and abs(parts["loss"] - ref.item()) <= 1e-5
    assert err_g <= 1e-4 and 0 < o["bound"] < 1
    grads = [p.grad for p in net.mlp_coarse.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all().item() for g in grads) and any(g.abs().max().item() > 0 for g in grads)
    # the fourth channel changes nothing on the render side
    rd3 = step(images_ip)
    assert torch.equal(rd3["coarse"]["rgb"], c["rgb"]) and torch.equal(rd3["coarse"]["depth"], c["depth"])
    assert net.grid_c_imgs.shape == (n, nv, 3, H, W)
